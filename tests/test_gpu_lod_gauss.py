"""-m gpu: m2s_lod_build and the cut on a tree built under M2S_MERGE_MODEL_GAUSSIAN (pin 4g): every level byte-identical to single merges
under the same model on a second context, the bounds equal to tests/merge_gauss_ref.bounds bit for bit, the cut equal to lod_ref's on
those bounds with every leaf once; m2s_lod_blend refuses such a tree and blends a footprint tree built afterwards as before."""
import numpy as np
import pytest

import lod_ref as lr
import merge_gauss_ref as mg
import merge_ref as mr
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.converter import Converter

pytestmark = pytest.mark.gpu
F = np.float32
CHAINS = ((3, 10), tuple(range(1, 11)))
TAUS = (0.0, 0.5, 4.0, 1e9)
FOCAL, NEAR = 600.0, 0.05


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(hiplib):
    c = Converter(0)
    yield c
    c.close()


def chain_one_by_one(ref, rec, levels, max_group, dot):
    """tests/test_gpu_lod.py's: the steps as single merges on another context; a step that merges nothing only permutes"""
    ref.upload_records(rec)
    out, maps, pending, skipped = [rec], [], None, 0
    for lv in levels:
        before = ref.num_stored
        after = ref.merge(lv, max_group, dot)["after"]
        m = ref.download_merge_map()
        m = m if pending is None else m[pending]
        if after == before:
            skipped += 1
            pending = m
            continue
        pending = None
        maps.append(m)
        out.append(ref.download())
    return out, maps, skipped


def cameras(b, first):
    """far, between, inside a cluster, at a leaf's own position, at a node's own position of the last level, the origin"""
    ok = np.flatnonzero(np.isfinite(b[:, 0:3]).all(1))
    leaf = ok[ok < first[1]]
    top = ok[ok >= first[-2]]
    mid = b[leaf[len(leaf) // 2], 0:3]
    return [(50.0, 40.0, 30.0), (3.0, 0.5, -2.0), tuple(float(v) for v in mid + F(0.02)), tuple(float(v) for v in b[leaf[0], 0:3]),
            tuple(float(v) for v in b[top[0], 0:3]), (0.0, 0.0, 0.0)]


@pytest.mark.parametrize("sigma", (1.0, 0.65))
@pytest.mark.parametrize("n", (65, 4099))
def test_tree_levels_bounds_and_cuts(conv, ref, n, sigma):
    rec = mg.gauss_records(n, n)
    conv.set_merge_model("gaussian", sigma)
    ref.set_merge_model("gaussian", sigma)
    mixed = 0
    for levels in CHAINS:
        want_levels, maps, skipped = chain_one_by_one(ref, rec, levels, 4, 0.5)
        counts = [len(v) for v in want_levels]
        conv.upload_records(rec)
        out = conv.lod_build(levels, 4, 0.5)
        first = conv.lod_levels()
        tree, parent, b = conv.download_lod(0), conv.download_lod(1), conv.download_lod(2)
        print(f"gauss lod build n={n} chain={levels} sigma={sigma}: {out}")
        assert out["leaves"] == n and out["nodes"] == sum(counts) == first[-1] and out["levels"] == len(counts) >= 2 and out["skipped"] == skipped
        for l, want in enumerate(want_levels):
            assert np.array_equal(bits(tree[first[l]:first[l + 1]]), bits(want)), ("level", l)
        wparent, wfirst = lr.link(maps, counts)
        assert wfirst == first and np.array_equal(parent, wparent)
        assert np.array_equal(bits(b), bits(mg.bounds(tree, sigma)))                 # pin 4g, bit for bit
        assert not np.array_equal(bits(b), bits(lr.bounds(tree)))                    # ... and not the footprint's longer edge
        for cam in cameras(b, first):
            for tau in TAUS:
                want = lr.select(b, parent, first, cam, FOCAL, tau, NEAR)
                got = conv.lod_select(cam, FOCAL, tau, NEAR)
                per = got.pop("per_level")
                assert got == want["counts"] and per == want["per_level"], (got, want["counts"], per, want["per_level"])
                ids = conv.download_lod_nodes()
                assert np.array_equal(ids, want["nodes"])
                assert conv.num_stored == len(ids) and np.array_equal(bits(conv.download()), bits(tree[ids]))
                flags = np.zeros(first[-1], bool)
                flags[ids] = True
                assert lr.cut_ok(parent, first, flags)                               # every leaf once
                mixed += sum(1 for v in per if v) >= 2
    assert mixed > 0                                                                 # (cuts through more than one level were among them)


def test_the_restatement_builds_the_same_tree(conv):
    """the chain of merge_gauss_ref.merge: the same level sizes and links, fields within the merge's bars level by level"""
    rec = mg.gauss_records(257, 3)
    conv.set_merge_model("gaussian", 0.65)
    conv.upload_records(rec)
    conv.lod_build((3, 10), 4, 0.5)
    first = conv.lod_levels()
    tree, parent = conv.download_lod(0), conv.download_lod(1)
    wrecs, wparent, wfirst = mg.chain(rec, (3, 10), 4, 0.5, 0.65)
    assert wfirst == first and np.array_equal(parent, wparent)
    # level 1 is one merge of the leaves (the levels above merge the DEVICE's level below: compared in test_gpu_merge_gauss's way there)
    want, _, _, info = mg.merge(rec, 3, 4, 0.5, 0.65)
    err = mg.compare(tree[first[1]:first[2]], want, info, 0.65)
    assert err["scalar_ulps"] <= mg.SCALAR_ULPS_BAR and err["cov_rel"] <= mg.COV_REL_BAR, err


def test_blend_refuses_a_gaussian_tree_and_takes_a_footprint_tree_built_afterwards(conv, hiplib):
    rec = mr.crafted_records(4099, 5)
    cam, tau = (3.0, 0.5, -2.0), 4.0
    conv.set_merge_model("footprint")
    conv.upload_records(rec)
    conv.lod_build((3, 6, 10), 4, 0.5)
    conv.lod_select(cam, FOCAL, tau, NEAR)
    before_counts = conv.lod_blend(cam, FOCAL, tau, NEAR)
    before = conv.download()
    assert before_counts["blended"] > 0
    conv.set_merge_model("gaussian", 0.65)
    # the switch alone does not touch the footprint tree: it remembers its model
    conv.lod_select(cam, FOCAL, tau, NEAR)
    assert conv.lod_blend(cam, FOCAL, tau, NEAR) == before_counts and np.array_equal(bits(conv.download()), bits(before))
    conv.upload_records(rec)
    conv.lod_build((3, 6, 10), 4, 0.5)
    cut = conv.lod_select(cam, FOCAL, tau, NEAR)
    kept = conv.download()
    with pytest.raises(M2SError) as e:
        conv.lod_blend(cam, FOCAL, tau, NEAR)
    assert e.value.status == 7 and b"GAUSSIAN" in hiplib.m2s_last_error(conv._h)
    assert conv.num_stored == cut["selected"] and np.array_equal(bits(conv.download()), bits(kept))   # refused: nothing touched
    conv.set_merge_model("footprint")
    conv.lod_select(cam, FOCAL, tau, NEAR)
    with pytest.raises(M2SError):
        conv.lod_blend(cam, FOCAL, tau, NEAR)                                       # still the Gaussian tree, whatever the switch says now
    conv.upload_records(rec)
    conv.lod_build((3, 6, 10), 4, 0.5)
    conv.lod_select(cam, FOCAL, tau, NEAR)
    assert conv.lod_blend(cam, FOCAL, tau, NEAR) == before_counts
    assert np.array_equal(bits(conv.download()), bits(before))
