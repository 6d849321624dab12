"""-m gpu: a context whose conversion side has a history gives the bytes of a fresh one.

The conversion side keeps per lane a record buffer, a look-back chain and a multi-pass work set (offsets, slice starts, TriSetup
records, counter).  Lane 0's record pool grows; lane 1's buffer and slice-start table follow it at lane 1's next use; what is sized by
the scene is released with it.  A buffer that is not replaced when it should be, or replaced while a conversion still uses it, shows
only in a context that has run another size before, so this test runs the same sequence of conversions - blocking and on two lanes,
single-pass and multi-pass - through ONE Converter at a small configuration, a large one and the small one again, and compares every
array it keeps, byte for byte, with the same sequence in a fresh Converter at that configuration alone.

Every pipeline writes the same bytes (held to the oracle by the parity tests): equality is exact."""
import numpy as np
import pytest

from mesh2splat_amd import synth
from mesh2splat_amd.converter import Converter

pytestmark = pytest.mark.gpu

#        cube_sphere, R of the single-pass conversions, R of the multi-pass ones: 12 n^2 triangles of about 0.195 (R / n)^2 fragments,
#        i.e. about 3 per triangle at the first R and 28 at the second
SMALL = (8, 32, 96)
LARGE = (48, 192, 576)
SINGLE_PASS = ("team", "lean", "sparse")


def two_lanes(conv, R, total, records, out, tag):
    """Three submissions in flight, nine wait / submit rounds, drain: every conversion gives the blocking one's counter and bytes, and
    the records waited for alternate between the two lanes' buffers."""
    conv.set_async_lanes(2)
    totals, where = [], set()
    for _ in range(3):
        conv.submit(R)
    for i in range(12):
        totals.append(conv.wait())
        where.add(conv.device_records)
        assert totals[-1] == total, (tag, i, totals[-1], total)
        assert np.array_equal(conv.download().view(np.uint32), records.view(np.uint32)), (tag, i)
        if i < 9:
            conv.submit(R)
    assert len(where) >= 2, (tag, where)          # the second lane really ran
    conv.set_async_lanes(1)
    out[f"{tag}_async_totals"] = np.array(totals, np.uint64)
    out[f"{tag}_async_last"] = conv.download()


def run_sequence(conv, cfg):
    n_sphere, R_single, R_multi = cfg
    out = {}
    conv.upload_scene(synth.cube_sphere(n_sphere))
    conv.set_max_gaussians(0)
    total = conv.convert(R_single)
    assert conv.last_pipeline in SINGLE_PASS, conv.last_pipeline
    out["single_total"], out["single_records"] = np.array([total], np.uint64), conv.download()
    two_lanes(conv, R_single, total, out["single_records"], out, "single")
    total = conv.convert(R_multi)                  # grows the record pool: lane 1's buffer and slice starts have to follow
    assert conv.last_pipeline == "multipass", conv.last_pipeline
    out["multi_total"], out["multi_records"] = np.array([total], np.uint64), conv.download()
    assert len(out["multi_records"]) == total > len(out["single_records"])
    two_lanes(conv, R_multi, total, out["multi_records"], out, "multi")
    return out


@pytest.fixture(scope="module")
def runs(hiplib):
    fresh = {}
    for name, cfg in (("small", SMALL), ("large", LARGE)):
        with Converter(0) as c:
            fresh[name] = run_sequence(c, cfg)
    with Converter(0) as c:
        reused = [(name, run_sequence(c, cfg)) for name, cfg in (("small", SMALL), ("large", LARGE), ("small", SMALL))]
    assert len(fresh["large"]["multi_records"]) > 4 * len(fresh["small"]["multi_records"])   # the context really grows, then runs below capacity
    return fresh, reused


@pytest.mark.parametrize("step", [0, 1, 2], ids=["small_first", "large_after_small", "small_after_large"])
def test_reused_context_equals_fresh_context(runs, step):
    fresh, reused = runs
    name, got = reused[step]
    want = fresh[name]
    assert sorted(got) == sorted(want)
    bad = []
    for key in sorted(want):
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        same = a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
        if not same:
            bad.append(f"{key}: shape {a.shape} / {b.shape}, bytes that differ "
                       f"{int((a.view(np.uint8) != b.view(np.uint8)).sum()) if a.shape == b.shape else 'n/a'}")
    print(f"{name} (step {step}): {len(want)} outputs, {sum(np.asarray(v).nbytes for v in want.values())} bytes compared, "
          f"{len(want['single_records'])} + {len(want['multi_records'])} records")
    assert not bad, "; ".join(bad)
