"""-m gpu: m2s_lod_select_frustum and m2s_lod_select_budget_frustum (Converter.lod_select / .lod_select_budget with frustum=) against
their numpy restatement (tests/lod_frustum_ref.py, held to the pin by tests/test_lod_frustum_ref.py), against each other on a second
context, and against the frame the prepass draws afterwards.  Everything is compared for equality: flags through node ids, record
bytes, counts, per-level counts, both frustum counts, the bits of tau_px, met, selected_finer."""
import ctypes as C

import numpy as np
import pytest

import camera
import lod_budget_ref as br
import lod_frustum_ref as fr
import lod_ref as lr
import merge_ref as mr
from mesh2splat_amd import lod
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.prepass import PrepassParams
from test_gpu_lod_budget import CHAINS, FOCAL, NEAR, bits, download_tree, special_records

pytestmark = pytest.mark.gpu
F = np.float32
PROJ = camera.perspective(45.0, 16 / 9, 0.01, 100.0)
EYE = np.eye(4, dtype=F)
# over the module, computed from the restatement alone: asserted by the last test
SEEN = {"cuts": 0, "all_inside": 0, "none_inside": 0, "partly_inside": 0, "inner_dropped": 0, "mean_passes_no_leaf": 0, "nan_leaf_inside": 0}


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


def to_c(frustum):
    return lod.frustum_to_c(*frustum)


def cameras(b, first):
    """-> [(frustum, camera_position)], derived from the downloaded bounds: far and looking at the centroid; inside a cluster, with the
    guard bands 1, 1.05 and 4; far and looking away; a model matrix that is not the identity, the camera carried into model space"""
    leaves = b[:first[1], 0:3].astype(np.float64)
    ok = np.isfinite(leaves).all(1)
    ctr = leaves[ok].mean(0) if ok.any() else np.zeros(3)
    r = max(float(np.linalg.norm(leaves[ok] - ctr, axis=1).max()) if ok.any() else 0.0, 0.5)
    far = ctr + np.array([0.3, 0.2, 1.0]) * 6.0 * r
    mid = leaves[ok][ok.sum() // 2] + 0.02 if ok.any() else np.array([0.02, 0.02, 0.02])
    target = ctr if np.linalg.norm(ctr - mid) > 1e-3 else ctr + np.array([0.0, 0.0, -1.0])

    def f32(v):
        return tuple(float(F(x)) for x in v)

    out = [((EYE, camera.look_at(far, ctr), PROJ, 1.05), f32(far))]
    out += [((EYE, camera.look_at(mid, target), PROJ, g), f32(mid)) for g in (1.0, 1.05, 4.0)]
    out.append(((EYE, camera.look_at(far, far + (far - ctr)), PROJ, 1.05), f32(far)))
    model = camera.trs((0.4, -0.3, 0.2), (1, 2, 3), 35.0, (1.25, 1.25, 1.25))
    Mm = model.T.astype(np.float64)                                                  # the math matrix: world = Mm @ model-space
    world_eye = (Mm @ np.append(mid, 1.0))[:3]
    world_target = (Mm @ np.append(target, 1.0))[:3]
    out.append(((model, camera.look_at(world_eye, world_target), PROJ, 1.05), f32(mid)))
    return out


def tally(b, first, frustum, vis, sel):
    n0 = first[1]
    ins = vis[:n0]
    SEEN["cuts"] += 1
    SEEN["all_inside"] += bool(ins.all())
    SEEN["none_inside"] += not ins.any()
    SEEN["partly_inside"] += bool(ins.any() and not ins.all())
    SEEN["inner_dropped"] += int((sel["plain"] & ~vis)[n0:].sum())
    SEEN["mean_passes_no_leaf"] += int(np.count_nonzero(fr.inside(b[n0:], *frustum) & ~vis[n0:]))
    SEEN["nan_leaf_inside"] += int(np.count_nonzero(np.isnan(b[:n0, 0:3]).any(axis=1) & ins))


def check_cut(conv, tree, parent, b, first, frustum, vis, cam, tau, got, focal=FOCAL, near=NEAR):
    """what `conv` holds after a frustum cut that returned `got`, against the restatement at tau"""
    sel = fr.select(b, parent, first, cam, focal, tau, near, frustum, vis)
    assert {k: got[k] for k in lod.SELECT_COUNTS} == sel["counts"] and got["per_level"] == sel["per_level"]
    assert got["visible_leaves"] == sel["visible_leaves"] and got["culled"] == sel["culled"]
    assert conv.num_stored == len(sel["nodes"])
    if len(sel["nodes"]):
        ids = conv.download_lod_nodes()
        assert ids.dtype == np.uint32 and np.array_equal(ids, sel["nodes"])
        assert np.array_equal(bits(conv.download()), bits(tree[ids]))
    else:
        assert conv.device_lod_nodes == 0 and conv.download().shape == (0, 24)
    tally(b, first, frustum, vis, sel)
    return sel


def check_select(conv, tree, parent, b, first, frustum, vis, cam, tau, focal=FOCAL, near=NEAR):
    got = conv.lod_select(cam, focal, tau, near, frustum=to_c(frustum))
    return got, check_cut(conv, tree, parent, b, first, frustum, vis, cam, tau, got, focal, near)


def check_budget(conv, ref, tree, parent, b, first, frustum, LHvis, cam, budget, tau_min, focal=FOCAL, near=NEAR):
    L, H, vis = LHvis
    want = fr.search(L, H, first, vis, budget, tau_min)
    got = conv.lod_select_budget(cam, focal, budget, tau_min, near, frustum=to_c(frustum))
    print(f"lod frustum budget nodes={first[-1]} guard={frustum[3]} budget={budget} floor={tau_min}: {got} want key {want['key']:#x}")
    assert br.key_of(got["tau_px"]) == want["key"] and got["met"] == want["met"] and got["selected_finer"] == want["selected_finer"]
    assert got["selected"] == want["selected"]
    sel = check_cut(conv, tree, parent, b, first, frustum, vis, cam, want["tau_px"], got, focal, near)
    assert np.array_equal(sel["nodes"], np.flatnonzero(br.flags_at(L, H, want["key"])))
    if ref is not None:                                                              # the returned tau on a second context: the same bytes
        other = ref.lod_select(cam, focal, got["tau_px"], near, frustum=to_c(frustum))
        assert other == {k: got[k] for k in other}
        assert ref.num_stored == conv.num_stored and np.array_equal(bits(ref.download()), bits(conv.download()))
        if conv.num_stored:
            assert np.array_equal(ref.download_lod_nodes(), conv.download_lod_nodes())
    return got


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257, 4099))
def test_frustum_cuts_and_budgets_against_the_restatement(conv, ref, n):
    rec = special_records(n, n)
    for levels in CHAINS:
        for max_group in (2, 64):
            for unsigned in (False, True):
                conv.upload_records(rec)
                out = conv.lod_build(levels, max_group, 0.5, unsigned_axis=unsigned)
                ref.upload_records(rec)
                assert ref.lod_build(levels, max_group, 0.5, unsigned_axis=unsigned) == out
                tree, parent, b, first = download_tree(conv)
                for frustum, cam in cameras(b, first):
                    L, H, _, vis = fr.intervals(b, parent, first, cam, FOCAL, NEAR, frustum)
                    ends = br.endpoints(L, H)
                    for key in sorted({0, ends[len(ends) // 2], ends[-1]}):
                        check_select(conv, tree, parent, b, first, frustum, vis, cam, br.tau_of(key))
                    for budget in fr.budgets(L, H, first, vis):
                        check_budget(conv, ref, tree, parent, b, first, frustum, (L, H, vis), cam, budget, 0.0)
                    check_budget(conv, ref, tree, parent, b, first, frustum, (L, H, vis), cam, max(1, first[-1] // 2), 2.0)


def clean_tree(conv, n=600, seed=21, levels=(3, 6, 10), min_scale=0.0):
    """records without a NaN position (a leaf at NaN is inside every frustum); min_scale > 0: no edge of 0 either (a node above the
    leaves whose edge is 0 does not refine even at tau 0)"""
    rec = mr.crafted_records(n, seed, invalid=False)
    rec[:, 8:10] = np.maximum(rec[:, 8:10], F(min_scale))
    conv.upload_records(rec)
    conv.lod_build(levels, 4, 0.5, unsigned_axis=True)
    return download_tree(conv)


def test_nothing_inside_leaves_no_records_and_a_plain_cut_follows(conv):
    tree, parent, b, first = clean_tree(conv)
    frustum, cam = cameras(b, first)[4]
    L, H, _, vis = fr.intervals(b, parent, first, cam, FOCAL, NEAR, frustum)
    assert not vis.any()
    got, _ = check_select(conv, tree, parent, b, first, frustum, vis, cam, 1.0)
    plain = lr.select(b, parent, first, cam, FOCAL, 1.0, NEAR)
    assert got["selected"] == 0 and got["per_level"] == [0] * (len(first) - 1) and got["visible_leaves"] == 0
    assert got["culled"] == plain["counts"]["selected"] and got["refine"] == plain["counts"]["refine"]
    assert conv.num_stored == 0 and conv.device_lod_nodes == 0 and len(conv.download_lod_nodes()) == 0
    for tau_min, key in ((0.0, 0), (2.0, br.key_of(2.0))):
        got = check_budget(conv, None, tree, parent, b, first, frustum, (L, H, vis), cam, 10, tau_min)
        assert (br.key_of(got["tau_px"]), got["selected"], got["met"], got["selected_finer"]) == (key, 0, True, 0) and conv.num_stored == 0
    after = conv.lod_select(cam, FOCAL, 1.0, NEAR)                                   # the tree is whole: the plain cut works
    assert {k: after[k] for k in lod.SELECT_COUNTS} == plain["counts"] and set(after) == set(lod.SELECT_COUNTS) | {"per_level"}
    assert np.array_equal(conv.download_lod_nodes(), plain["nodes"]) and np.array_equal(bits(conv.download()), bits(tree[plain["nodes"]]))


def test_a_tree_of_one_level_and_more_nodes_than_the_sweeps_lanes(conv):
    """one level: the leaves are the last level, nobody has a parent; then 300 003 leaves under a chain 1..10: grid-stride trips in
    every kernel, workgroups beyond the first in the visibility launches"""
    rec = mr.crafted_records(700, 4, invalid=False)
    rec[:, 0:3] = np.random.default_rng(4).normal(0, 1, (700, 3)).astype(F)          # no two in one place: level 0 merges nothing
    conv.upload_records(rec)
    assert conv.lod_build((0,), 4, 0.5)["levels"] == 1
    tree, parent, b, first = download_tree(conv)
    frustum, cam = cameras(b, first)[2]
    L, H, _, vis = fr.intervals(b, parent, first, cam, FOCAL, NEAR, frustum)
    assert 0 < vis.sum() < len(vis)
    check_select(conv, tree, parent, b, first, frustum, vis, cam, 1.0)
    got = check_budget(conv, None, tree, parent, b, first, frustum, (L, H, vis), cam, 1, 0.0)
    assert got["selected"] == int(vis.sum()) and not got["met"]
    n = 300003
    rng = np.random.default_rng(5)
    base = mr.crafted_records(4099, 77)
    rec = base[rng.integers(0, len(base), n)]
    rec[:, 0:3] = rng.normal(0, 1, (n, 3)).astype(F)
    conv.upload_records(rec)
    out = conv.lod_build(tuple(range(1, 11)), 4, -2.0, unsigned_axis=True)
    assert out["levels"] >= 4 and out["nodes"] > 1024 * 256
    tree, parent, b, first = download_tree(conv)
    frustum, cam = (EYE, camera.look_at((0.3, -0.2, 0.1), (2.0, 1.0, -1.0)), PROJ, 1.05), (0.3, -0.2, 0.1)
    L, H, _, vis = fr.intervals(b, parent, first, cam, FOCAL, NEAR, frustum)
    got, sel = check_select(conv, tree, parent, b, first, frustum, vis, cam, 1.5)
    assert sum(1 for v in got["per_level"] if v) >= 2 and got["culled"] > 0
    got = check_budget(conv, None, tree, parent, b, first, frustum, (L, H, vis), cam, 20000, 0.0)
    plain = conv.lod_select_budget(cam, FOCAL, 20000, near=NEAR, dry_run=True)
    assert got["met"] and br.key_of(got["tau_px"]) < br.key_of(plain["tau_px"])       # the budget buys a finer cut of what is on screen


def test_dry_runs_change_nothing(conv):
    tree, parent, b, first = clean_tree(conv, 300, 11)
    rec2 = mr.crafted_records(50, 3)
    conv.upload_records(rec2)                                                        # the tree survives other records
    ptr, n2 = conv.device_records, conv.num_stored
    frustum, cam = cameras(b, first)[2]
    L, H, _, vis = fr.intervals(b, parent, first, cam, FOCAL, NEAR, frustum)
    want = fr.select(b, parent, first, cam, FOCAL, 1.0, NEAR, frustum, vis)
    dry = conv.lod_select(cam, FOCAL, 1.0, NEAR, dry_run=True, frustum=to_c(frustum))
    assert {k: dry[k] for k in lod.SELECT_COUNTS} == want["counts"] and dry["per_level"] == want["per_level"]
    assert (dry["visible_leaves"], dry["culled"]) == (want["visible_leaves"], want["culled"]) and want["culled"] > 0
    budget = max(1, want["counts"]["selected"] // 2)
    bw = fr.search(L, H, first, vis, budget)
    dryb = conv.lod_select_budget(cam, FOCAL, budget, near=NEAR, dry_run=True, frustum=to_c(frustum))
    assert br.key_of(dryb["tau_px"]) == bw["key"] and dryb["selected"] == bw["selected"] and dryb["selected_finer"] == bw["selected_finer"]
    assert conv.device_records == ptr and conv.num_stored == n2 and np.array_equal(bits(conv.download()), bits(rec2)) and conv.device_lod_nodes == 0
    with pytest.raises(M2SError):
        conv.download_lod_nodes()
    real = conv.lod_select_budget(cam, FOCAL, budget, near=NEAR, frustum=to_c(frustum))
    assert real == dryb
    ids, out = conv.download_lod_nodes(), bits(conv.download()).copy()
    assert conv.lod_select_budget(cam, FOCAL, budget, near=NEAR, frustum=to_c(frustum)) == real   # again: the same result and bytes
    assert np.array_equal(conv.download_lod_nodes(), ids) and np.array_equal(bits(conv.download()), out)
    for x, y in zip(download_tree(conv)[:3], (tree, parent, b)):                     # the tree is untouched
        assert np.array_equal(bits(x), bits(y))


def test_the_frame_after_the_frustum_cut_is_the_frame_after_the_plain_cut(conv):
    """prepass_sorted after both cuts at one tau: the nodes drawn after the frustum cut are a subsequence of those drawn after the
    plain cut, and the ones missing are the nodes above the leaves whose own position passes the test while no leaf's does.  At tau 0
    (leaves only) with the prepass's guard the sorted quads are the same bytes."""
    tree, parent, b, first = clean_tree(conv, 3000, 8, (2, 4, 6, 10), min_scale=1e-3)
    assert (b[first[1]:, 3] > 0).all()
    cases = [(c, t) for c in cameras(b, first)[1:4] + cameras(b, first)[5:] for t in (0.0, 3.0, 12.0)]
    # ... and cameras chosen on the restatement so that the plain cut draws a node the frustum cut drops: the eye beside a leaf, the
    # tau at which a node above the leaves is selected whose own position is inside while no leaf below it is
    leaves = np.flatnonzero(np.isfinite(b[:first[1], 0:3]).all(1))
    ctr = b[leaves, 0:3].astype(np.float64).mean(0)
    for j in leaves[::37]:
        eye = b[j, 0:3].astype(np.float64) + 0.02
        frustum, cam = (EYE, camera.look_at(eye, ctr), PROJ, 1.05), tuple(float(F(v)) for v in eye)
        Lp, Hp, _ = br.intervals(b, parent, first, cam, FOCAL, NEAR)
        cand = np.flatnonzero(fr.inside(b, *frustum) & ~fr.visibility(b, parent, first, frustum) & (Lp < Hp))
        if len(cand):
            cases.append(((frustum, cam), float(br.tau_of(int(Lp[cand[0]])))))
        if len(cases) >= 18:
            break
    missing = 0
    for (frustum, cam), tau in cases:
        pp = PrepassParams(view_mat=frustum[1], proj_mat=PROJ, model_mat=frustum[0], renderer_resolution=(1280, 720), resolution_target=1)
        vis = fr.visibility(b, parent, first, frustum)
        got, sel = check_select(conv, tree, parent, b, first, frustum, vis, cam, tau)
        ids = conv.download_lod_nodes() if got["selected"] else np.zeros(0, np.uint32)
        quads_f = conv.prepass_sorted(pp)
        drawn_f = ids[conv.download_sorted_sources(len(quads_f))]
        conv.lod_select(cam, FOCAL, tau, NEAR)
        ids = conv.download_lod_nodes()
        quads_p = conv.prepass_sorted(pp)
        drawn_p = ids[conv.download_sorted_sources(len(quads_p))]
        own = fr.inside(b, frustum[0], frustum[1], frustum[2], 1.05)                 # what the prepass tests: every drawn node's own position
        gone = sel["plain"] & own & ~vis
        keep = ~gone[drawn_p]
        assert np.array_equal(drawn_p[keep], drawn_f) and np.array_equal(bits(quads_p[keep]), bits(quads_f))
        assert set(drawn_p[~keep].tolist()) == set(np.flatnonzero(gone).tolist())
        if frustum[3] >= 1.05:                                                       # (a narrower guard than the prepass's also drops leaves it draws)
            assert not gone[:first[1]].any()
            missing += int(gone.sum())
        if tau == 0.0 and frustum[3] == 1.05:
            assert got["selected_leaves"] == got["selected"] and np.array_equal(bits(quads_p), bits(quads_f))
    print(f"frame test: {len(cases)} frames, {missing} nodes drawn after the plain cut only")
    assert len(cases) > 12 and missing > 0


def test_stage_time_with_profiling(conv):
    tree, parent, b, first = clean_tree(conv, 4099, 2)
    frustum, cam = cameras(b, first)[2]
    conv.set_profiling(True)
    try:
        conv.lod_select(cam, FOCAL, 1.0, NEAR, frustum=to_c(frustum))
        a = conv.last_lod_frustum_ms()
        conv.lod_select_budget(cam, FOCAL, 1000, near=NEAR, frustum=to_c(frustum))
        print(f"lod frustum visibility stage, 4 099 leaves: {a} ms, {conv.last_lod_frustum_ms()} ms in front of the budget search")
        assert a > 0 and conv.last_lod_frustum_ms() > 0
    finally:
        conv.set_profiling(False)


def test_errors(hiplib):
    c = Converter(0)
    try:
        out = (C.c_uint64 * 4)()
        res = lod.LodBudgetResultC()
        nan, inf = float("nan"), float("inf")

        def frustum(**kw):
            f = lod.frustum_to_c(EYE, camera.look_at((0, 0, 5), (0, 0, 0)), PROJ)
            for name, (k, v) in kw.items():
                if name == "guard_band":
                    f.guard_band = v
                else:
                    getattr(f, name)[k] = v
            return f

        def select(f, cam=(0.0, 0.0, 5.0), focal=500.0, tau=1.0, near=0.1, flags=0):
            p = lod.select_to_c(cam, focal, tau, near)
            p.flags = flags
            return hiplib.m2s_lod_select_frustum(c._h, C.byref(p), C.byref(f) if f is not None else None, out)

        def budget(f, cam=(0.0, 0.0, 5.0), focal=500.0, n=10, tau_min=0.0, near=0.1, flags=0):
            p = lod.budget_to_c(cam, focal, n, tau_min, near)
            p.flags = flags
            return hiplib.m2s_lod_select_budget_frustum(c._h, C.byref(p), C.byref(f) if f is not None else None, C.byref(res), out)

        assert select(frustum()) == 7 and budget(frustum()) == 7                     # no tree
        rec = mr.crafted_records(40, 1, invalid=False)
        c.upload_records(rec)
        c.lod_build((3, 10), 4, 0.5)
        before = c.download()
        for call in (select, budget):
            assert call(None) == 1
            for bad in (dict(model_to_world=(3, nan)), dict(world_to_view=(12, inf)), dict(view_to_clip=(0, -inf)), dict(view_to_clip=(15, nan)),
                        dict(guard_band=(0, nan)), dict(guard_band=(0, inf)), dict(guard_band=(0, 0.999)), dict(guard_band=(0, -2.0)),
                        dict(reserved=(0, 1)), dict(reserved=(2, 7))):
                assert call(frustum(**bad)) == 1, bad
            # the errors of the plain functions
            for bad in (dict(cam=(nan, 0, 0)), dict(focal=0.0), dict(focal=inf), dict(near=0.0), dict(near=nan), dict(flags=2)):
                assert call(frustum(), **bad) == 1, bad
        assert select(frustum(), tau=-1.0) == 1 and select(frustum(), tau=nan) == 1
        assert budget(frustum(), n=0) == 1 and budget(frustum(), tau_min=-1.0) == 1
        assert hiplib.m2s_lod_select_frustum(c._h, None, C.byref(frustum()), None) == 1
        assert np.array_equal(bits(c.download()), bits(before))
        assert select(frustum(guard_band=(0, 1.0)), flags=1) == 0 and np.array_equal(bits(c.download()), bits(before))
        two = (C.c_uint64 * 2)()
        assert hiplib.m2s_last_lod_frustum_counts(c._h, two) == 0 and hiplib.m2s_last_lod_frustum_counts(c._h, None) == 1
        p = lod.budget_to_c((0.0, 0.0, 5.0), 500.0, 10, near=0.1)
        f = frustum()
        assert hiplib.m2s_lod_select_budget_frustum(c._h, C.byref(p), C.byref(f), None, None) == 0       # (both outputs may be NULL)
        # an empty tree: the floor, met, nothing selected, nothing inside
        c.upload_records(np.zeros((0, 24), F))
        c.lod_build((1,))
        got = c.lod_select_budget((0, 0, 0), 500.0, 5, tau_min_px=2.0, frustum=frustum())
        assert got == {"nodes": 0, "selected": 0, "selected_leaves": 0, "refine": 0, "per_level": [0], "tau_px": 2.0, "met": True, "selected_finer": 0,
                       "visible_leaves": 0, "culled": 0}
        assert c.lod_select((0, 0, 0), 500.0, frustum=frustum())["selected"] == 0 and c.num_stored == 0
        c.lod_release()
        assert select(frustum()) == 7 and budget(frustum()) == 7
    finally:
        c.close()


def test_zz_the_cases_exercise_every_class():
    """Runs last in this module: over the cuts above some cameras saw every leaf, some none, some a part; selected nodes above the
    leaves were dropped; nodes above the leaves passed the test themselves while none of their leaves did; leaves at NaN were inside."""
    print(f"lod frustum, over the module: {SEEN}")
    assert SEEN["cuts"] > 1000 and all(v > 0 for v in SEEN.values()), SEEN
