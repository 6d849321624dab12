"""-m gpu: m2s_lod_build / m2s_lod_select (Converter.lod_build / .lod_select) against the same merges run one by one on a second context
and against the numpy restatement of links, bounds and cut (tests/lod_ref.py).  Everything is compared for equality: the tree's levels
byte for byte, parents, bounds, selected nodes, counts, record bytes and their order.  The restatement of a merge itself is
tests/test_gpu_merge.py's business."""
import ctypes as C

import numpy as np
import pytest

import lod_ref as lr
import merge_ref as mr
from mesh2splat_amd import lod, synth
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.score import orbit_cameras

pytestmark = pytest.mark.gpu
F = np.float32
CHAINS = ((0,), (3, 10), (3, 3, 6, 10), tuple(range(1, 11)))
TAUS = (0.0, 0.5, 4.0, 1e9)
FOCAL, NEAR = 600.0, 0.05
SEEN = {"mixed": 0, "gated": 0, "skipped": 0, "cuts": 0}               # over the module: asserted by the last test


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
    """the steps as single merges on another context -> (levels' records, the maps between tree levels, steps that merged nothing).  A step
    that merges nothing only permutes: its map is composed into the next one's."""
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


def download_tree(conv):
    first = conv.lod_levels()
    return conv.download_lod(0), conv.download_lod(1), conv.download_lod(2), first


def cameras(tree, b, first):
    """far, between, inside a cluster, at a leaf's own position, at a node's own position of the last level (d2 clamps to near^2), the origin"""
    ok = np.flatnonzero(np.isfinite(b[:, 0:3]).all(1))
    leaf = ok[ok < first[1]]
    top = ok[ok >= first[-2]]
    mid = b[leaf[len(leaf) // 2], 0:3]
    return [(50.0, 40.0, 30.0), (3.0, 0.5, -2.0), tuple(float(v) for v in mid + F(0.02)), tuple(float(v) for v in b[leaf[0], 0:3]),
            tuple(float(v) for v in b[top[0], 0:3]), (0.0, 0.0, 0.0)]


def check_select(conv, tree, parent, b, first, cam, tau, focal=FOCAL, near=NEAR):
    want = lr.select(b, parent, first, cam, focal, tau, near)
    got = conv.lod_select(cam, focal, tau, near)
    per = got.pop("per_level")
    print(f"lod select nodes={first[-1]} cam={tuple(round(v, 3) for v in cam)} tau={tau}: {got} per level {per}")
    assert got == want["counts"] and per == want["per_level"], (got, want["counts"], per, want["per_level"])
    ids = conv.download_lod_nodes()
    assert ids.dtype == np.uint32 and np.array_equal(ids, want["nodes"])
    assert conv.num_stored == len(ids) and np.array_equal(bits(conv.download()), bits(tree[ids]))
    flags = np.zeros(first[-1], bool)
    flags[ids] = True
    assert lr.cut_ok(parent, first, flags)
    SEEN["cuts"] += 1
    SEEN["mixed"] += sum(1 for v in per if v) >= 2
    SEEN["gated"] += len(lr.gated(parent, first, want)) > 0
    return want


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257, 4099))
def test_build_and_select_against_single_merges_and_the_restatement(conv, ref, n):
    rec = mr.crafted_records(n, n)
    for levels in CHAINS:
        for max_group in (2, 4, 64):
            for dot in (-2.0, 0.5):
                want_levels, maps, skipped = chain_one_by_one(ref, rec, levels, max_group, dot)
                counts = [len(v) for v in want_levels]
                conv.upload_records(rec)
                out = conv.lod_build(levels, max_group, dot)
                tree, parent, b, first = download_tree(conv)
                print(f"lod build n={n} chain={levels} group={max_group} dot={dot}: {out}")
                assert out["leaves"] == n and out["nodes"] == sum(counts) == first[-1] and out["levels"] == len(counts) and out["skipped"] == skipped
                assert out["first"] == first == [int(v) for v in np.concatenate([[0], np.cumsum(counts)])]
                for l, want in enumerate(want_levels):
                    assert np.array_equal(bits(tree[first[l]:first[l + 1]]), bits(want)), ("level", l)
                wparent, wfirst = lr.link(maps, counts)
                assert wfirst == first and np.array_equal(parent, wparent)
                assert np.array_equal(bits(b), bits(lr.bounds(tree)))
                assert conv.num_stored == counts[-1] and np.array_equal(bits(conv.download()), bits(want_levels[-1]))
                SEEN["skipped"] += skipped
                if max_group == 4 and dot == 0.5:                                    # two builds give the same bytes
                    conv.upload_records(rec)
                    assert conv.lod_build(levels, max_group, dot) == out
                    again = download_tree(conv)
                    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(again[:3], (tree, parent, b)))
                for cam in cameras(tree, b, first):
                    for tau in TAUS:
                        check_select(conv, tree, parent, b, first, cam, tau)


def test_a_tree_that_outgrows_its_first_reservation(ref):
    """A fresh context (the module's has planes that only ever grew): 1031 leaves under the chain 1..10 in pairs make the levels that
    tests/merge_ref.py gives for this input, 8921 nodes against a first reservation of 1031 + 515 — the planes grow at 1910, 3544 and
    6888 nodes, every time with the levels linked so far kept."""
    n, levels, sizes = 1031, tuple(range(1, 11)), [1031, 879, 830, 804, 791, 780, 773, 764, 762, 754, 753]
    rec = mr.crafted_records(n, n)
    want_levels, maps, skipped = chain_one_by_one(ref, rec, levels, 2, 0.5)
    counts = [len(v) for v in want_levels]
    conv = Converter(0)
    try:
        conv.upload_records(rec)
        out = conv.lod_build(levels, 2, 0.5)
        tree, parent, b, first = download_tree(conv)
        print(f"lod build n={n} chain={levels} group=2 dot=0.5 on a fresh context: {out}")
        assert out["nodes"] > n + n // 2
        assert out["nodes"] == 8921 and counts == sizes
        assert out["leaves"] == n and out["nodes"] == sum(counts) == first[-1] and out["levels"] == len(counts) and out["skipped"] == skipped == 0
        assert out["first"] == first == [int(v) for v in np.concatenate([[0], np.cumsum(counts)])]
        for l, want in enumerate(want_levels):
            assert np.array_equal(bits(tree[first[l]:first[l + 1]]), bits(want)), ("level", l)
        wparent, wfirst = lr.link(maps, counts)
        assert wfirst == first and np.array_equal(parent, wparent)
        assert np.array_equal(bits(b), bits(lr.bounds(tree)))
        assert conv.num_stored == counts[-1] and np.array_equal(bits(conv.download()), bits(want_levels[-1]))
        check_select(conv, tree, parent, b, first, cameras(tree, b, first)[2], 0.5)
    finally:
        conv.close()


def test_steps_that_merge_nothing_add_no_level(conv):
    rec = mr.crafted_records(65, 0)
    conv.upload_records(rec)
    out = conv.lod_build(tuple(range(1, 11)), 4, 0.5)
    sizes = list(np.diff(out["first"]))
    assert out["skipped"] == 10 - (out["levels"] - 1) > 0 and all(a > b for a, b in zip(sizes, sizes[1:])) and sizes[0] == 65
    assert conv.lod_build((0,) * 16, 4, 0.5)["skipped"] >= 15                        # (what level 0 merges, it merges once)


def test_grid_quadtree_table_on_the_device(conv):
    conv.upload_records(mr.grid_records(8))
    out = conv.lod_build(levels=(8, 9, 10))
    assert out["first"] == [0, 64, 80, 84, 85] and out["skipped"] == 0
    tree, parent, b, first = download_tree(conv)
    assert [float(b[first[l], 3]) for l in range(4)] == [0.125, 0.25, 0.5, 1.0]
    for D, want, level in ((100, 64, 0), (200, 16, 1), (300, 4, 2), (512, 1, 3), (511, 4, 2)):
        got = check_select(conv, tree, parent, b, first, (0.5, 0.5, float(D)), 1.0, 512.0, 1.0)
        assert got["per_level"] == [want if l == level else 0 for l in range(4)]
    assert check_select(conv, tree, parent, b, first, (0.5, 0.5, 3.0), 0.0, 512.0, 1.0)["per_level"] == [64, 0, 0, 0]
    assert check_select(conv, tree, parent, b, first, (0.5, 0.5, 3.0), 1e9, 512.0, 1.0)["per_level"] == [0, 0, 0, 1]


def test_more_than_one_workgroup_per_level_and_multi_block_scans(conv):
    """300 003 records, chain 1..10: 1 172 workgroups in the leaves' sweep (more than the grid-stride cap), levels of every size below"""
    n = 300003
    rng = np.random.default_rng(5)
    base = mr.crafted_records(4099, 77)
    rec = base[rng.integers(0, len(base), n)]
    rec[:, 0:3] = rng.normal(0, 1, (n, 3)).astype(F)
    conv.upload_records(rec)
    out = conv.lod_build(tuple(range(1, 11)), 4, -2.0)
    tree, parent, b, first = download_tree(conv)
    print(f"lod build n={n}: {out} in {conv.last_lod_build_ms:.2f} ms")
    assert out["levels"] >= 4 and np.array_equal(bits(tree[:n]), bits(rec)) and np.array_equal(bits(b), bits(lr.bounds(tree)))
    assert (parent[:first[-2]] < first[-1]).all() and (parent[first[-2]:] == lod.NO_PARENT).all()
    for l in range(out["levels"] - 1):
        p = parent[first[l]:first[l + 1]]
        assert p.min() == first[l + 1] and p.max() == first[l + 2] - 1 and len(np.unique(p)) == first[l + 2] - first[l + 1]
    mixed = 0
    for cam, tau in (((0.3, -0.2, 0.1), 1.0), ((4.0, 3.0, 5.0), 0.5), ((4.0, 3.0, 5.0), 8.0), ((0.0, 0.0, 0.0), 0.0)):
        mixed += sum(1 for v in check_select(conv, tree, parent, b, first, cam, tau)["per_level"] if v) >= 2
    assert mixed >= 2


def test_dry_run_and_what_select_invalidates(conv):
    rec = mr.crafted_records(300, 11)
    conv.upload_records(rec)
    conv.lod_build((3, 10), 4, 0.5)
    tree, parent, b, first = download_tree(conv)
    conv.upload_records(rec)                                                         # the tree survives other records
    conv.merge(2, 4, 0.5)
    rec2 = conv.download()
    sh = conv.bake_light(BakeParams(n_theta=4, n_phi=8, use_shadows=False), LightParams(light_position=(1.5, 2.0, 2.5)))
    conv.contrib_begin()
    conv.refit_begin()
    ptr, n2 = conv.device_records, conv.num_stored
    cam = (0.4, 0.1, -0.3)
    want = lr.select(b, parent, first, cam, FOCAL, 0.5, NEAR)
    dry = conv.lod_select(cam, FOCAL, 0.5, NEAR, dry_run=True)
    assert dry.pop("per_level") == want["per_level"] and dry == want["counts"]
    assert conv.device_records == ptr and conv.num_stored == n2 and np.array_equal(bits(conv.download()), bits(rec2))
    assert conv.device_contrib(0) and conv.device_refit(0) and conv.device_sh and conv.device_merge_map and conv.device_lod_nodes == 0
    assert np.array_equal(bits(conv.download_sh()), bits(sh))
    with pytest.raises(M2SError):
        conv.download_lod_nodes()
    real = conv.lod_select(cam, FOCAL, 0.5, NEAR)
    assert real.pop("per_level") == want["per_level"] and real == want["counts"] and conv.num_stored == want["counts"]["selected"]
    assert conv.device_contrib(0) == 0 and conv.device_refit(0) == 0 and conv.device_sh == 0 and conv.device_merge_map == 0
    assert not conv.positions_ready and conv.device_lod_nodes != 0
    with pytest.raises(M2SError):
        conv.download_contrib()
    assert np.array_equal(conv.download_lod_nodes(), want["nodes"])
    conv.merge(10, 4, 0.5)                                                           # the records change: the node indices go
    assert conv.device_lod_nodes == 0
    for x, y in zip(download_tree(conv)[:3], (tree, parent, b)):                     # ... the tree does not
        assert np.array_equal(bits(x), bits(y))


def test_adopted_memory_is_not_written_and_the_leaves_resolution_is_kept(conv, hiplib):
    rec = mr.crafted_records(1000, 13)
    owner = Converter(0)
    try:
        owner.upload_records(rec)
        conv.set_records(owner.device_records, len(rec), 48)
        out = conv.lod_build((2, 5, 10), 4, 0.5)
        assert out["levels"] > 1 and conv.device_records != owner.device_records
        tree, parent, b, first = download_tree(conv)
        assert np.array_equal(bits(tree[:1000]), bits(rec))
        conv.set_records(owner.device_records, len(rec), 99)                         # other current records, another resolutionTarget
        check_select(conv, tree, parent, b, first, (0.2, 0.2, 0.2), 0.5)
        assert conv.device_records != owner.device_records and hiplib.m2s_last_resolution(conv._h) == 48
        assert np.array_equal(bits(owner.download()), bits(rec))
    finally:
        owner.close()


def test_tree_survives_a_conversion_and_release_ends_it(conv, hiplib):
    rec = mr.crafted_records(500, 3)
    conv.upload_records(rec)
    conv.lod_build((3, 10), 4, 0.5)
    tree, parent, b, first = download_tree(conv)
    conv.upload_scene(synth.unit_quad())
    assert conv.convert(32) > 0
    check_select(conv, tree, parent, b, first, (0.1, 0.0, 0.2), 0.5)
    assert conv.device_lod(0) and conv.device_lod(1) and conv.device_lod(2) and conv.device_lod(3) == 0
    conv.lod_release()
    conv.lod_release()                                                               # (twice is fine)
    assert conv.device_lod(0) == 0
    sp = lod.select_to_c((0, 0, 0), FOCAL)
    assert hiplib.m2s_lod_select(conv._h, C.byref(sp), None) == 7
    assert hiplib.m2s_lod_levels(conv._h, None, None) == 7 and hiplib.m2s_download_lod(conv._h, 0, None, 0) == 7
    with pytest.raises(M2SError):
        conv.lod_levels()


def test_errors(hiplib):
    c = Converter(0)
    try:
        out = (C.c_uint64 * 4)()

        def build(levels=(1, 2), max_group=4, dot=0.5, reserved=0, n_steps=None, tail=None):
            p = lod.build_to_c(levels, max_group, dot)
            p.reserved = reserved
            if n_steps is not None:
                p.n_steps = n_steps
            if tail is not None:
                p.levels[15] = tail
            return hiplib.m2s_lod_build(c._h, C.byref(p), out)

        def select(cam=(0.0, 0.0, 0.0), focal=500.0, tau=1.0, near=0.1, flags=0, reserved=0):
            p = lod.select_to_c(cam, focal, tau, near)
            p.flags, p.reserved = flags, reserved
            return hiplib.m2s_lod_select(c._h, C.byref(p), out)

        assert build() == 7 and select() == 7                                        # no records; no tree
        rec = mr.crafted_records(40, 1)
        c.upload_records(rec)
        nan, inf = float("nan"), float("inf")
        for bad in (dict(n_steps=0), dict(n_steps=17), dict(levels=(11,)), dict(levels=(3, 2)), dict(levels=(1, 5, 4)), dict(tail=1), dict(max_group=1),
                    dict(max_group=65), dict(dot=nan), dict(reserved=1)):
            assert build(**bad) == 1, bad
        assert hiplib.m2s_lod_build(c._h, None, None) == 1 and hiplib.m2s_lod_select(c._h, None, None) == 1
        assert c.num_stored == 40 and np.array_equal(bits(c.download()), bits(rec)) and select() == 7
        assert build(levels=(10,) * 16, max_group=64, dot=-inf) == 0 and out[0] == 40 and out[2] == 2 and out[3] == 15
        nodes = int(out[1])
        for bad in (dict(cam=(nan, 0, 0)), dict(cam=(0, inf, 0)), dict(cam=(0, 0, -inf)), dict(focal=0.0), dict(focal=-1.0), dict(focal=nan), dict(focal=inf),
                    dict(tau=-1.0), dict(tau=nan), dict(tau=inf), dict(near=0.0), dict(near=-1.0), dict(near=nan), dict(near=inf), dict(flags=2),
                    dict(flags=3), dict(reserved=1)):
            assert select(**bad) == 1, bad
        before = c.download()
        assert select(flags=1) == 0 and np.array_equal(bits(c.download()), bits(before))
        small = np.empty(10, np.uint8)
        for which, unit in ((0, 96), (1, 4), (2, 16)):
            assert hiplib.m2s_download_lod(c._h, which, small.ctypes.data, nodes * unit - 1) == 5
        assert hiplib.m2s_download_lod(c._h, 3, small.ctypes.data, 10) == 1
        assert select() == 0
        k = C.c_uint64()
        assert hiplib.m2s_download_lod_nodes(c._h, small.ctypes.data, 0, C.byref(k)) == 5 and k.value == c.num_stored
        # zero records build an empty tree, and its cut is empty
        c.upload_records(np.zeros((0, 24), F))
        assert c.lod_build((1,)) == {"leaves": 0, "nodes": 0, "levels": 1, "skipped": 1, "first": [0, 0]}
        got = c.lod_select((0, 0, 0), 500.0)
        assert got == {"nodes": 0, "selected": 0, "selected_leaves": 0, "refine": 0, "per_level": [0]} and c.num_stored == 0
        # conversions in flight: both refused, the conversion still delivered
        c.upload_records(rec)
        assert build() == 0
        c.upload_scene(synth.cube_sphere(6, tex_size=16))
        c.submit(48)
        total = c.wait()
        c.submit(48)
        assert build() == 7 and select() == 7 and select(flags=1) == 7 and b"in flight" in hiplib.m2s_last_error(c._h)
        assert c.wait() == total
        assert select() == 0
    finally:
        c.close()


def test_a_cut_renders_and_tau_zero_is_the_full_frame(conv):
    """the unit quad at R = 64: the frame of a cut runs; with tau_px = 0 the cut is the leaves in node order, and its frame is the frame of
    those records uploaded.  A conversion stores scale = (|Ju|, |Jv|) = (1, 1) here, in units the viewer divides by the resolutionTarget,
    and that is the edge the pin reads: at 1.88 .. 2.0 from the eye with focal 144.85 it projects to 72 .. 77 of the pin's pixels, so
    tau_px = 75 cuts through the middle of the tree (the restatement on the CPU: 2592 / 40 / 35 / 10 / 37 nodes per level)."""
    scene = synth.unit_quad()
    conv.upload_scene(scene)
    n = conv.convert(64)
    rec = conv.download()
    cam = orbit_cameras(scene, 1, 160, 120)[0]
    pp, lp = cam.frame_params(64, (1.0, 2.0, 3.0), 30.0, shadow_resolution=128)
    out = conv.lod_build()
    assert out["leaves"] == n and out["levels"] > 2
    eye, focal = lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, 120)
    cut = conv.lod_select(eye, focal, 75.0, cam.near)
    assert 0 < cut["selected"] < n and sum(1 for v in cut["per_level"] if v) >= 2
    tree, parent, b, first = download_tree(conv)
    assert cut["per_level"] == lr.select(b, parent, first, eye, focal, 75.0, cam.near)["per_level"]
    frame = conv.render_frame(pp, lp)
    assert frame.any()
    full = conv.lod_select(eye, focal, 0.0, cam.near)
    assert full["per_level"][0] == full["selected"] == n and np.array_equal(conv.download_lod_nodes(), np.arange(n, dtype=np.uint32))
    a = np.array(conv.render_frame(pp, lp), copy=True)
    conv.upload_records(rec)
    b = np.array(conv.render_frame(pp, lp), copy=True)
    assert np.array_equal(a, b)


def test_zz_the_cases_exercise_mixed_cuts_gating_and_skipped_steps():
    """Runs last in this module: over the cuts above, some took nodes of two levels or more, some had nodes gated by an ancestor, and some
    chains had steps that merged nothing."""
    print(f"lod, over the module: {SEEN}")
    assert SEEN["cuts"] > 1000 and SEEN["mixed"] > 0 and SEEN["gated"] > 0 and SEEN["skipped"] > 0
