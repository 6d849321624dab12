"""-m gpu: m2s_records_to_world_units (Converter.to_world_units) against its numpy restatement (tests/worldunits_ref.py), bit for bit; what
it does to the context; that the viewer and the exports do not notice it for a power-of-two R; and what it is for: a level-of-detail
tree over a conversion whose cuts are mixed (tests/lod_ref.py, tests/merge_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import camera
import lod_ref as lr
import merge_ref as mr
import worldunits_ref as wr
from mesh2splat_amd import synth
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.prepass import PrepassParams

pytestmark = pytest.mark.gpu
F = np.float32
RS = (2, 48, 64, 100, 1024, 4095)
CHAIN = (4, 5, 6, 7, 8, 9, 10)
FOCAL = 154.51
TINY = np.finfo(F).tiny                                                     # the smallest normal: every quotient of it is subnormal
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, TINY, -TINY * F(1.2345678), F(2.0) ** -120, F(7e-45), F(3.4e38)], F)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def owner(hiplib):
    c = Converter(0)
    yield c
    c.close()


def crafted(n, seed):
    """merge_ref's records (a NaN position, a zero quaternion and a negative scale among them) with the special values written over
    scale words — all three columns, and scale[3] too, which must keep its bits"""
    rec = mr.crafted_records(n, seed, invalid=True)
    for i, v in enumerate(SPECIALS):
        if n:
            rec[(7 * i) % n, 8 + i % 3] = v
    if n > 3:
        rec[3, 11] = np.nan
        rec[2, 11] = TINY
    return rec


def pool_ptr(c):
    return c.reserve_records(max(c.num_stored, 1))


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 257, 4099))
def test_crafted_records_out_of_place_then_in_place(conv, owner, hiplib, n):
    rec = crafted(n, n)
    owner.upload_records(rec)
    for R in RS:
        conv.set_records(owner.device_records, n, R)
        out = conv.to_world_units()
        assert out["records"] == n and out["previous_R"] == R and out["ms"] >= 0.0
        want = wr.to_world_units(rec, R)
        got = conv.download() if n else np.zeros((0, 24), F)
        assert np.array_equal(bits(got), bits(want)), (n, R)
        assert conv.resolution == hiplib.m2s_last_resolution(conv._h) == 1
        assert conv.device_records != owner.device_records and conv.device_records == pool_ptr(conv)
        assert np.array_equal(bits(owner.download() if n else rec), bits(rec))           # the adopted buffer is not written
        # the records are in the pool now: declared to be at another R they take the in-place kernel
        conv.set_records(conv.device_records, n, 3)
        ptr = conv.device_records
        assert conv.to_world_units()["previous_R"] == 3 and conv.device_records == ptr and conv.resolution == 1
        assert np.array_equal(bits(conv.download() if n else got), bits(wr.to_world_units(want, 3))), (n, R, "in place")
    if n:                                                                   # the words that must survive: everything but columns 8..10
        keep = [k for k in range(24) if k not in (8, 9, 10)]
        assert np.array_equal(bits(conv.download()[:, keep]), bits(rec[:, keep]))


def test_more_lanes_than_the_grid_stride_cap(conv, owner):
    """600 001 records: 3.6 M 16-byte words against 2048 x 256 lanes out of place, 600 001 records against them in place"""
    n = 600001
    rng = np.random.default_rng(3)
    rec = crafted(4099, 5)[rng.integers(0, 4099, n)]
    owner.upload_records(rec)
    conv.set_records(owner.device_records, n, 100)
    assert conv.to_world_units() == {"records": n, "previous_R": 100, "ms": 0.0}      # (profiling is off)
    want = wr.to_world_units(rec, 100)
    assert np.array_equal(bits(conv.download()), bits(want))
    conv.set_records(conv.device_records, n, 48)
    conv.to_world_units()
    assert np.array_equal(bits(conv.download()), bits(wr.to_world_units(want, 48)))


def test_no_op_cases_change_nothing(conv, owner, hiplib):
    rec = crafted(300, 2)
    owner.upload_records(rec)
    conv.set_records(owner.device_records, 300, 64)
    assert conv.to_world_units()["previous_R"] == 64
    conv.merge(3, 4, 0.5)                                                   # leaves a map that lives as long as the records epoch
    conv.contrib_begin()
    conv.refit_begin()
    ptr, n, after = conv.device_records, conv.num_stored, conv.download()
    assert conv.device_merge_map and conv.device_contrib(0) and conv.device_refit(0)
    again = conv.to_world_units()
    assert again == {"records": n, "previous_R": 1, "ms": 0.0}
    assert conv.device_records == ptr and conv.num_stored == n and conv.resolution == 1
    assert conv.device_merge_map and conv.device_contrib(0) and conv.device_refit(0)      # the epoch did not advance
    assert np.array_equal(bits(conv.download()), bits(after))
    # uploaded records carry R = 0 and are taken as world units
    conv.upload_records(rec)
    conv.contrib_begin()
    ptr = conv.device_records
    assert conv.to_world_units() == {"records": 300, "previous_R": 0, "ms": 0.0}
    assert conv.device_records == ptr and conv.device_contrib(0) and conv.resolution == 0
    assert np.array_equal(bits(conv.download()), bits(rec))
    # adopted at R = 1: the caller's memory stays the context's
    conv.set_records(owner.device_records, 300, 1)
    assert conv.to_world_units()["previous_R"] == 1 and conv.device_records == owner.device_records
    prev = C.c_uint32(9)
    assert hiplib.m2s_records_to_world_units(conv._h, None) == 0 and hiplib.m2s_records_to_world_units(conv._h, C.byref(prev)) == 0 and prev.value == 1


def test_what_the_pass_invalidates(conv):
    conv.upload_scene(synth.cube_sphere(6, tex_size=16))
    conv.convert(32)
    conv.merge(2, 4, 0.5)
    conv.bake_light(BakeParams(n_theta=4, n_phi=8, use_shadows=False), LightParams(light_position=(1.5, 2.0, 2.5)))
    conv.contrib_begin()
    conv.refit_begin()
    pp = PrepassParams(view_mat=camera.look_at((1.6, 1.1, 2.3), (0.0, 0.0, 0.0)), proj_mat=camera.perspective(45.0, 16 / 9, 0.01, 100.0),
                       renderer_resolution=(320, 180), resolution_target=conv.resolution)
    assert conv.prepass_sorted(pp, download=False) > 0
    assert conv.device_merge_map and conv.device_contrib(0) and conv.device_refit(0) and conv.device_sh and conv.device_sorted_sources
    assert conv.to_world_units()["previous_R"] == 32
    assert conv.device_merge_map == 0 and conv.device_contrib(0) == 0 and conv.device_refit(0) == 0 and conv.device_sh == 0
    assert conv.device_sorted_sources == 0 and not conv.positions_ready
    with pytest.raises(M2SError):
        conv.download_contrib()


def ply_scales(path, fmt):
    """the three scale floats of every row of a .ply written by export_ply: (n, 3) float32"""
    raw = open(path, "rb").read()
    body = raw[raw.index(b"end_header\n") + len(b"end_header\n"):]
    row, off = {0: (248, 220), 1: (76, 48), 2: (48, 32)}[fmt]
    assert len(body) % row == 0
    rows = np.frombuffer(body, np.uint8).reshape(-1, row)
    return np.ascontiguousarray(rows[:, off:off + 12]).view(F)


def frame_of(conv, rec):
    """the prepass of the context's records through a camera that looks at their centre from 1.5 diagonals away"""
    lo, hi = rec[:, 0:3].min(0).astype(np.float64), rec[:, 0:3].max(0).astype(np.float64)
    at = tuple((lo + hi) / 2)
    eye = tuple((lo + hi) / 2 + 1.5 * np.linalg.norm(hi - lo) * np.array([0.5, 0.35, 0.79]))
    pp = PrepassParams(view_mat=camera.look_at(eye, at), proj_mat=camera.perspective(45.0, 16 / 9, 0.01, 100.0), renderer_resolution=(320, 180),
                       resolution_target=conv.resolution)
    vis, quads, depths = conv.prepass(pp)
    assert vis > 0
    return vis, bits(quads).copy(), bits(depths).copy()


@pytest.mark.parametrize("name, R", (("quad", 64), ("quad", 48), ("spheres", 128)))
def test_in_place_on_conversions_and_what_the_viewer_and_the_exports_see(conv, tmp_path, name, R):
    """Power-of-two R: s / R and std / R are exact scalings, so s * fl(std / R) and fl(s / R) * std are the same float and every consumer
    that takes its divisor from `resolution` writes the same bytes.  R = 48: before, the file holds fl(log(a)) with a = fl(s * fl(std / 48)),
    afterwards fl(log(b)) with b = fl(fl(s / 48) * std).  a and b are two roundings each away from s * std / 48: |a - b| <= 4 u |a| with
    u = 2^-24, so log a and log b differ by at most 4 u = 2.4e-7.  The stored logarithms here lie beyond -4 (std / 48 = 0.0135 times
    an edge of 1.0 or 1e-7), where a unit in the last place is 4.8e-7 or more: the two true logarithms are at most half a unit apart
    and their roundings at most one.  That is the bar."""
    scene = synth.unit_quad() if name == "quad" else synth.sphere_grid(2, n=6, tex_size=64)
    conv.upload_scene(scene)
    n = conv.convert(R)
    rec = conv.download()
    ptr = conv.device_records
    assert conv.resolution == R and ptr == pool_ptr(conv)
    before = frame_of(conv, rec)
    files = {}
    for fmt in (0, 1, 2):
        path = str(tmp_path / f"before{fmt}.ply")
        conv.export_ply(path, fmt, 0.65)
        files[fmt] = open(path, "rb").read()
    out = conv.to_world_units()
    assert out["records"] == n and out["previous_R"] == R
    assert conv.device_records == ptr and conv.resolution == 1
    assert np.array_equal(bits(conv.download()), bits(wr.to_world_units(rec, R)))
    after = frame_of(conv, rec)
    pow2 = R & (R - 1) == 0
    if pow2:
        assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    for fmt in (0, 1, 2):
        path = str(tmp_path / f"after{fmt}.ply")
        conv.export_ply(path, fmt, 0.65)
        got = open(path, "rb").read()
        if pow2:
            assert got == files[fmt], fmt
        else:
            (tmp_path / "b.ply").write_bytes(files[fmt])
            a, b = ply_scales(str(tmp_path / "b.ply"), fmt), ply_scales(path, fmt)
            assert a.shape == b.shape == (n, 3) and np.isfinite(a).all() and (np.abs(a) >= 4).all()
            ulps = np.abs(a.astype(np.float64) - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)
            print(f"R={R} format {fmt}: exported log-scales differ by at most {ulps.max()} ulp, {np.count_nonzero(ulps)} of {ulps.size} differ")
            assert ulps.max() <= 1.0
            assert len(got) == len(files[fmt])


def chain_one_by_one(ref, rec, levels, max_group, dot):
    """the steps as single merges on another context (as tests/test_gpu_lod.py) -> (levels' records, the maps between tree levels)"""
    ref.upload_records(rec)
    out, maps, pending = [rec], [], None
    for lv in levels:
        before = ref.num_stored
        after = ref.merge(lv, max_group, dot)["after"]
        m = ref.download_merge_map()
        m = m if pending is None else m[pending]
        if after == before:
            pending = m
            continue
        pending = None
        maps.append(m)
        out.append(ref.download())
    return out, maps


def test_the_purpose_a_tree_over_a_conversion_with_mixed_cuts(conv, owner):
    R, h = 64, F(1) / F(64)
    conv.upload_scene(synth.unit_quad())
    n = conv.convert(R)
    assert n == R * R
    # without the pass: every cut draws the leaves
    conv.lod_build(CHAIN, 4, 0.5)
    for cam in ((-1.0, 0.5, 0.3), (0.5, 0.5, 8.0)):
        got = conv.lod_select(cam, FOCAL, 4.0, dry_run=True)
        assert got["per_level"][0] == got["selected"] == n, got
    conv.convert(R)
    conv.to_world_units()
    rec = conv.download()
    out = conv.lod_build(CHAIN, 4, 0.5)
    tree, parent, b, first = conv.download_lod(0), conv.download_lod(1), conv.download_lod(2), conv.lod_levels()
    want_levels, maps = chain_one_by_one(owner, rec, CHAIN, 4, 0.5)
    counts = [len(v) for v in want_levels]
    print(f"world units: lod build {out}")
    assert out["leaves"] == n and out["nodes"] == sum(counts) and out["levels"] == len(counts) >= 3
    for l, want in enumerate(want_levels):
        assert np.array_equal(bits(tree[first[l]:first[l + 1]]), bits(want)), ("level", l)
    wparent, wfirst = lr.link(maps, counts)
    assert wfirst == first and np.array_equal(parent, wparent) and np.array_equal(bits(b), bits(lr.bounds(tree)))
    # the quadtree: 2h and 4h on levels 1 and 2, within merge_ref's bar for a scalar field (4 fp32 ulps of its magnitude)
    for l, e in ((1, F(2) * h), (2, F(4) * h)):
        longest = float(b[first[l]:first[l + 1], 3].max())
        print(f"level {l}: longest edge {longest!r} against {float(e)!r}")
        assert abs(longest - float(e)) <= mr.SCALAR_ULPS_BAR * float(np.spacing(e))
    mixed = {}
    for cam in ((0.0, 0.0, 0.3), (0.5, 0.5, 2.0), (0.5, 0.5, 8.0), (-1.0, 0.5, 0.3)):
        for tau in (1.0, 2.0, 4.0):
            want = lr.select(b, parent, first, cam, FOCAL, tau)
            got = conv.lod_select(cam, FOCAL, tau)
            per = got.pop("per_level")
            print(f"world units cut cam={cam} tau={tau}: per level {per}")
            assert got == want["counts"] and per == want["per_level"]
            ids = conv.download_lod_nodes()
            assert np.array_equal(ids, want["nodes"]) and np.array_equal(bits(conv.download()), bits(tree[ids]))
            assert lr.cut_ok(parent, first, want["flags"]) and conv.resolution == 1
            mixed[(cam, tau)] = sum(1 for v in per if v) >= 2
    assert mixed[((-1.0, 0.5, 0.3), 4.0)]
    assert all(any(mixed[(cam, tau)] for tau in (1.0, 2.0, 4.0)) for cam in ((0.0, 0.0, 0.3), (0.5, 0.5, 2.0), (0.5, 0.5, 8.0), (-1.0, 0.5, 0.3)))
    # A single merge of the world-unit records.  The chain's first level comes from its SECOND step: the cells of merge level 4 (64 per
    # axis over the quad's box) hold one record each at R = 64, so merge(4) only sorts — the restatement says so too, and `skipped` above
    # counts that step — and merge(5) is the one whose 2 x 2 blocks give 1088 records with a longest edge of 2h, within merge_ref's bar.
    assert out["skipped"] == 1
    conv.upload_records(rec)
    merged = conv.merge(4, 4, 0.5)
    want4, _, counts4, _ = mr.merge(rec, 4, 4, 0.5)
    assert merged == counts4 and merged["after"] == n and np.array_equal(bits(conv.download()), bits(want4))
    conv.upload_records(rec)
    merged = conv.merge(5, 4, 0.5)
    after = conv.download()
    e = lr.bounds(after)[:, 3].max()
    print(f"merge(5) over the world-unit records: {merged}, longest edge {e!r}")
    assert merged["after"] == counts[1] == 1088 and np.array_equal(bits(after), bits(want_levels[1]))
    assert abs(float(e) - float(F(2) * h)) <= mr.SCALAR_ULPS_BAR * float(np.spacing(F(2) * h)), e


def test_context_state_round_the_pass(conv, hiplib):
    scene = synth.unit_quad()
    conv.upload_scene(scene)
    n = conv.convert(64)
    rec = conv.download()
    counts = conv.download_triangle_counts()
    assert counts.sum() == n
    conv.lod_build((3, 4, 5), 4, 0.5)                                       # a tree of stored-unit leaves
    tree = conv.download_lod(0)
    cam = (0.5, 0.5, 2.0)
    before = conv.lod_select(cam, FOCAL, 75.0, dry_run=True)               # (stored edges of 1.0: the pin's pixels are R-ths of the screen's)
    assert sum(1 for v in before["per_level"] if v) >= 2
    assert conv.to_world_units()["previous_R"] == 64 and conv.resolution == 1
    assert np.array_equal(conv.download_triangle_counts(), counts)          # still the conversion's R
    assert conv.lod_select(cam, FOCAL, 75.0, dry_run=True) == before        # the tree is a copy
    assert np.array_equal(bits(conv.download_lod(0)), bits(tree)) and conv.resolution == 1
    got = conv.lod_select(cam, FOCAL, 75.0)
    assert got == before and conv.resolution == 64                          # its cut hands the leaves' R back
    assert np.array_equal(bits(conv.download()), bits(tree[conv.download_lod_nodes()]))
    assert np.array_equal(conv.download_triangle_counts(), counts)
    # a conversion afterwards is a conversion: stored units, its own R
    assert conv.convert(64) == n and conv.resolution == 64 and np.array_equal(bits(conv.download()), bits(rec))
    conv.to_world_units()
    assert conv.convert(32) == 32 * 32 and conv.resolution == 32 and conv.download_triangle_counts().sum() == 32 * 32
    conv.lod_release()


def test_errors(hiplib):
    assert hiplib.m2s_records_to_world_units(None, None) == 1 and hiplib.m2s_last_world_units_ms(None) == 0.0
    c = Converter(0)
    try:
        prev = C.c_uint32(9)
        assert hiplib.m2s_records_to_world_units(c._h, C.byref(prev)) == 7 and prev.value == 0       # no records
        with pytest.raises(M2SError):
            c.to_world_units()
        c.upload_scene(synth.cube_sphere(6, tex_size=16))
        c.submit(48)
        total = c.wait()
        c.submit(48)
        assert hiplib.m2s_records_to_world_units(c._h, C.byref(prev)) == 7 and b"in flight" in hiplib.m2s_last_error(c._h)
        assert c.wait() == total and c.resolution == 48
        assert c.to_world_units() == {"records": total, "previous_R": 48, "ms": 0.0} and c.resolution == 1
    finally:
        c.close()


def test_profiled_time_and_run_to_run(conv, owner):
    rec = crafted(4099, 9)
    owner.upload_records(rec)
    runs = []
    conv.set_profiling(True)
    try:
        for _ in range(2):
            conv.set_records(owner.device_records, 4099, 100)
            out = conv.to_world_units()
            assert out["ms"] > 0.0
            first = conv.download()
            conv.set_records(conv.device_records, 4099, 48)
            assert conv.to_world_units()["ms"] > 0.0
            runs.append((first, conv.download()))
    finally:
        conv.set_profiling(False)
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
