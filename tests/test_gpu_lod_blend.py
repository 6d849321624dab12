"""-m gpu: m2s_lod_blend (Converter.lod_blend, lod_select(..., blend=), lod_select_budget(..., blend=)) against its numpy restatement
(tests/lod_blend_ref.py, held to what the blend is for by tests/test_lod_blend_ref.py).  Everything is compared for equality: the plane
of weights, every record byte, the four counts, the SH rows of a tree built with carry_sh, the node indices the cut left."""
import ctypes as C

import numpy as np
import pytest

import compact_ref as cr
import lod_blend_ref as br
import lod_budget_ref as lb
import lod_ref as lr
import merge_ref as mr
from mesh2splat_amd import lod
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.prepass import PrepassParams
from test_gpu_lod import cameras, download_tree
from test_gpu_lod_frustum import cameras as frustum_cameras

pytestmark = pytest.mark.gpu
F = np.float32
CHAINS = ((0,), (3, 10), (3, 3, 6, 10))
TAUS = (0.0, 0.5, 4.0, 1e9)
BANDS = (1.0, 0.25, 2.0 ** -20)
FOCAL, NEAR = 600.0, 0.05
# over the module, computed from the restatement alone: asserted by the last test
SEEN = {"blends": 0, "inside": 0, "saturated": 0, "turned": 0, "non_unit_parent": 0, "den_not_positive": 0, "invalid_record": 0}


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


def check_blend(conv, tree, parent, b, first, cam, tau, band, focal=FOCAL, near=NEAR, tree_sh=None, got=None):
    """the context holds a cut taken with (cam, focal, tau, near): blend it (or take `got`, the counts of a blend already run) and compare"""
    ids = conv.download_lod_nodes()
    want = br.blend(tree, parent, b, ids, cam, focal, tau, near, band, tree_sh)
    if got is None:
        got = conv.lod_blend(cam, focal, tau, near, band)
    assert got == want["counts"], (got, want["counts"])
    t = conv.download_lod_blend_t()
    assert t.dtype == F and np.array_equal(bits(t), bits(want["t"]))
    assert conv.num_stored == len(ids) and np.array_equal(bits(conv.download()), bits(want["records"]))
    assert np.array_equal(conv.download_lod_nodes(), ids) and (conv.device_lod_nodes != 0) == (len(ids) > 0) == (conv.device_lod_blend_t != 0)
    if tree_sh is not None:
        assert np.array_equal(bits(conv.download_sh()), bits(want["sh"]))
    on = want["t"] > 0
    par = tree[parent[ids[parent[ids] != lod.NO_PARENT]]]                           # (a parent that is a merge's result is unit: the ones
    SEEN["blends"] += 1                                                              #  that are not are copies of their child, den == 0)
    SEEN["inside"] += int(np.count_nonzero(on & (want["t"] < 1)))
    SEEN["saturated"] += want["counts"]["saturated"]
    SEEN["turned"] += want["counts"]["turned"]
    SEEN["non_unit_parent"] += int(np.count_nonzero(~br.is_unit(par[:, br.ROT])))
    with np.errstate(invalid="ignore"):
        SEEN["den_not_positive"] += int(np.count_nonzero(~np.isnan(want["den"]) & ~(want["den"] > 0)))
    SEEN["invalid_record"] += int(np.count_nonzero(~cr.valid_mask(tree[ids])))
    return want


def switch_taus(b, parent, first, cam, focal=FOCAL, near=NEAR):
    """two taus at which this camera's cut is about to change: one key below a switch, and a switch itself"""
    L, H, _ = lb.intervals(b, parent, first, cam, focal, near)
    keys = lb.endpoints(L, H)
    if len(keys) < 3:
        return []
    return [float(lb.tau_of(keys[len(keys) // 3] - 1)), float(lb.tau_of(keys[(2 * len(keys)) // 3]))]


def records_of(n):
    return mr.grid_records(8) if n == "grid" else mr.crafted_records(n, n)


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257, 4099, "grid"))
def test_blend_against_the_restatement(conv, n):
    rec = records_of(n)
    turn = 0
    for chain in (CHAINS if n != "grid" else ((8, 9, 10),)):
        for max_group, unsigned in ((2, False), (64, True)):
            conv.upload_records(rec)
            conv.lod_build(chain, max_group, 0.5, unsigned_axis=unsigned)
            tree, parent, b, first = download_tree(conv)
            cams = cameras(tree, b, first)
            for ci, cam in enumerate(cams):
                for tau in list(TAUS) + (switch_taus(b, parent, first, cam) if ci == 1 else []):
                    band = BANDS[turn % 3]
                    turn += 1
                    conv.lod_select(cam, FOCAL, tau, NEAR)
                    want = check_blend(conv, tree, parent, b, first, cam, tau, band)
                    if turn % 7 == 0:                                                # a second call: the same bytes; another band: that band's
                        check_blend(conv, tree, parent, b, first, cam, tau, band)
                        other = BANDS[(turn + 1) % 3]
                        assert check_blend(conv, tree, parent, b, first, cam, tau, other)["counts"]["records"] == want["counts"]["records"]
    print(f"lod blend n={n}: {SEEN}")


def test_the_children_one_key_below_every_switch_of_the_quadtree(conv):
    """what the blend is for, on the device: just below a parent's threshold its children are the parent (t within 2^-20 of 1)"""
    conv.upload_records(mr.grid_records(8))
    conv.lod_build((8, 9, 10))
    tree, parent, b, first = download_tree(conv)
    for cam in ((0.5, 0.5, 3.0), (3.0, 0.5, -2.0)):
        T = lb.thresholds(b, cam, 512.0, NEAR)
        n = 0
        for P in range(first[1], first[-1]):
            tau = float(lb.tau_of(int(T[P]) - 1))
            conv.lod_select(cam, 512.0, tau, NEAR)
            want = check_blend(conv, tree, parent, b, first, cam, tau, 1.0, focal=512.0)
            mine = parent[conv.download_lod_nodes()] == P
            n += int(mine.sum())
            assert (want["t"][mine] >= 1 - 2.0 ** -20).all()
        assert n == 84


@pytest.mark.parametrize("n", (65, 4099))
def test_the_sh_rows_of_a_tree_with_a_plane(hiplib, n):
    c = Converter(0)
    try:
        rec = mr.crafted_records(n, n + 1)
        rng = np.random.default_rng(n)
        c.carry_sh = True
        c.upload_records(rec)
        c.upload_sh(rng.normal(0, 1, (n, 48)).astype(F), 3)
        c.lod_build((3, 6, 10), 4, 0.5, unsigned_axis=True)
        tree, parent, b, first = download_tree(c)
        tree_sh, degree = c.download_lod_sh()
        cam = cameras(tree, b, first)[1]
        blended = 0
        for k, tau in enumerate([0.0, 4.0] + switch_taus(b, parent, first, cam)):
            c.lod_select(cam, FOCAL, tau, NEAR)
            want = check_blend(c, tree, parent, b, first, cam, tau, BANDS[k % 2], tree_sh=tree_sh)
            info = c.sh_plane_info()
            assert info["rows"] == len(want["t"]) and info["degree"] == degree == 3
            blended += want["counts"]["blended"]
        assert blended > 0
        c.carry_sh = False                                                           # a tree without a plane touches none
        c.upload_records(rec)
        c.lod_build((3, 6, 10), 4, 0.5, unsigned_axis=True)
        c.lod_select(cam, FOCAL, 4.0, NEAR)
        check_blend(c, *download_tree(c), cam, 4.0, 1.0)
        assert c.device_sh == 0
    finally:
        c.close()


def test_once_after_each_kind_of_cut(conv):
    rec = mr.crafted_records(600, 21, invalid=False)
    rec[:, 7] = 1.0
    conv.upload_records(rec)
    conv.lod_build((3, 6, 10), 4, 0.5, unsigned_axis=True)
    tree, parent, b, first = download_tree(conv)
    fcams = frustum_cameras(b, first)
    (frustum, cam), (away, cam_away) = fcams[0], fcams[4]
    tau = switch_taus(b, parent, first, cam)[0]
    # plain, through lod_select(..., blend=): the dict gains "blend", and without it is what it was
    plain = conv.lod_select(cam, FOCAL, tau, NEAR)
    got = conv.lod_select(cam, FOCAL, tau, NEAR, blend=0.25)
    assert set(got) == set(plain) | {"blend"} and {k: got[k] for k in plain} == plain
    check_blend(conv, tree, parent, b, first, cam, tau, 0.25, got=got["blend"])
    assert "blend" not in conv.lod_select(cam, FOCAL, tau, NEAR, dry_run=True, blend=0.25)
    # budget: the returned tau
    budget = max(first[-1] - first[-2], (first[1] + first[-1] - first[-2]) // 3)
    got = conv.lod_select_budget(cam, FOCAL, budget, near=NEAR, blend=1.0)
    assert set(got) == set(conv.lod_select_budget(cam, FOCAL, budget, near=NEAR, dry_run=True)) | {"blend"}
    check_blend(conv, tree, parent, b, first, cam, got["tau_px"], 1.0, got=got["blend"])
    assert got["blend"]["records"] == got["selected"]
    # frustum and occluded
    fc = lod.frustum_to_c(*frustum)
    got = conv.lod_select(cam, FOCAL, tau, NEAR, frustum=fc, blend=1.0)
    assert got["selected"] > 0
    check_blend(conv, tree, parent, b, first, cam, tau, 1.0, got=got["blend"])
    depth = np.ones((36, 64), F)
    depth[:, :32] = 0                                                                # the left half hides what is behind it
    got = conv.lod_select(cam, FOCAL, tau, NEAR, frustum=fc, occluder=lod.occluder_to_c(depth), blend=0.25)
    assert 0 < got["selected"] and got["occluded_leaves"] > 0
    check_blend(conv, tree, parent, b, first, cam, tau, 0.25, got=got["blend"])
    # a frustum cut that selects nothing: zero records, a valid no-op
    got = conv.lod_select(cam_away, FOCAL, tau, NEAR, frustum=lod.frustum_to_c(*away), blend=1.0)
    assert got["selected"] == 0 and got["blend"] == {"records": 0, "blended": 0, "saturated": 0, "turned": 0}
    assert conv.num_stored == 0 and len(conv.download_lod_blend_t()) == 0 and conv.device_lod_blend_t == 0
    assert len(conv.download_lod_nodes()) == 0


def test_the_prepass_runs_on_the_blended_records(conv, ref):
    rec = mr.crafted_records(600, 5, invalid=False)
    conv.upload_records(rec)
    conv.lod_build((3, 6, 10), 4, 0.5, unsigned_axis=True)
    tree, parent, b, first = download_tree(conv)
    (M, V, P, _), cam = frustum_cameras(b, first)[0]
    tau = switch_taus(b, parent, first, cam)[0]
    conv.lod_select(cam, FOCAL, tau, NEAR)
    want = check_blend(conv, tree, parent, b, first, cam, tau, 1.0)
    assert want["counts"]["blended"] > 0
    pp = PrepassParams(view_mat=V, proj_mat=P, model_mat=M, renderer_resolution=(160, 90), resolution_target=1)
    vis, quads, depths = conv.prepass(pp)
    ref.upload_records(want["records"])
    rvis, rquads, rdepths = ref.prepass(pp)
    assert vis == rvis > 0 and np.array_equal(bits(quads), bits(rquads)) and np.array_equal(bits(depths), bits(rdepths))
    assert conv.device_lod_blend_t != 0                                             # (the prepass does not change the records)


def test_a_tree_of_300_003_leaves(conv):
    n = 300003
    rng = np.random.default_rng(5)
    base = mr.crafted_records(4099, 77)
    rec = base[rng.integers(0, len(base), n)]
    rec[:, 0:3] = rng.normal(0, 1, (n, 3)).astype(F)
    conv.upload_records(rec)
    conv.lod_build(tuple(range(1, 11)), 4, -2.0)
    tree, parent, b, first = download_tree(conv)
    for cam, tau, band in (((0.3, -0.2, 0.1), 1.0, 1.0), ((4.0, 3.0, 5.0), 8.0, 0.25)):
        conv.lod_select(cam, FOCAL, tau, NEAR)
        want = check_blend(conv, tree, parent, b, first, cam, tau, band)
        print(f"lod blend n={n} tau={tau} band={band}: {want['counts']} in {conv.last_lod_blend_ms():.3f} ms {conv.last_lod_blend_stage_ms()}")
        assert want["counts"]["blended"] > 0 and conv.last_lod_blend_ms() > 0
    conv.lod_release()


def test_errors(hiplib):
    c = Converter(0)
    try:
        out = (C.c_uint64 * 4)(7, 7, 7, 7)

        def blend(cam=(0.3, 0.1, 0.2), focal=500.0, tau=1.0, near=0.1, band=1.0, reserved=0):
            p = lod.LodBlendParamsC()
            p.camera_position[:] = cam
            p.focal_px, p.tau_px, p.near, p.band, p.reserved = focal, tau, near, band, reserved
            return hiplib.m2s_lod_blend(c._h, C.byref(p), out)

        rec = mr.crafted_records(300, 9)
        c.upload_records(rec)
        assert blend() == 7 and list(out) == [0, 0, 0, 0]                            # no tree
        c.lod_build((3, 10), 4, 0.5)
        assert blend() == 7                                                          # a tree, no cut
        c.lod_select((0.3, 0.1, 0.2), 500.0, 1.0, 0.1, dry_run=True)
        assert blend() == 7 and b"last cut" in hiplib.m2s_last_error(c._h)            # only a dry run
        c.lod_select((0.3, 0.1, 0.2), 500.0, 1.0, 0.1)
        before = c.download()
        nan, inf = float("nan"), float("inf")
        for bad in (dict(band=0.0), dict(band=1.5), dict(band=nan), dict(band=-1.0), dict(band=inf), dict(cam=(nan, 0, 0)), dict(cam=(0, inf, 0)),
                    dict(focal=0.0), dict(focal=nan), dict(tau=-1.0), dict(tau=inf), dict(near=0.0), dict(near=nan), dict(reserved=1)):
            assert blend(**bad) == 1, bad
        assert hiplib.m2s_lod_blend(c._h, None, out) == 1
        assert np.array_equal(bits(c.download()), bits(before)) and c.device_lod_blend_t == 0
        with pytest.raises(M2SError):
            c.download_lod_blend_t()
        assert blend() == 0 and out[0] == c.num_stored and c.device_lod_blend_t != 0
        four = (C.c_uint64 * 4)()
        assert hiplib.m2s_last_lod_blend_counts(c._h, four) == 0 and list(four) == list(out)
        small = np.empty(1, F)
        k = C.c_uint64()
        assert hiplib.m2s_download_lod_blend_t(c._h, small.ctypes.data, 0, C.byref(k)) == 5 and k.value == c.num_stored
        c.upload_records(c.download())                                               # records uploaded since the cut
        assert blend() == 7 and c.device_lod_blend_t == 0
        c.lod_select((0.3, 0.1, 0.2), 500.0, 1.0, 0.1)
        c.merge(10, 4, 0.5)                                                          # ... or rewritten by another pass
        assert blend() == 7
        # another tree since the cut: a build that merges nothing leaves the records, but their node indices are the old tree's
        c.upload_records(rec[:1])
        c.lod_build((0,))
        c.lod_select((0.3, 0.1, 0.2), 500.0, 1.0, 0.1)
        assert blend() == 0
        c.lod_build((0,))
        assert blend() == 7
        c.lod_select((0.3, 0.1, 0.2), 500.0, 1.0, 0.1)
        c.lod_release()
        assert blend() == 7
    finally:
        c.close()


def test_zz_the_cases_exercise_every_class():
    """Runs last in this module: over the blends above there were weights strictly inside (0, 1), weights of exactly 1, frames that were
    turned, parents whose quaternion is not unit, parents that project no larger than their child, and invalid records."""
    print(f"lod blend, over the module: {SEEN}")
    assert SEEN["blends"] > 1000 and all(v > 0 for v in SEEN.values()), SEEN
