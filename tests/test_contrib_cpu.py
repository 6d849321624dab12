"""CPU: the numpy restatement of the contribution pass (tests/contrib_ref.py) against hand-computed stacks and against the albedo alpha
plane of the splat pass's restatement (tests/splat_ref.py)."""
import numpy as np

import contrib_ref
import splat_ref

f32 = np.float32
W, H = 32, 24


def u8(v):
    return f32(np.rint(np.fmin(np.fmax(f32(v), f32(0)), f32(1)) * f32(255.0)) / f32(255.0))


def stack(alphas, px=5, py=7, half_px=3.0):
    return np.stack([splat_ref.quad_at(W, H, px, py, half_px, a=a) for a in alphas])


def test_hand_computed_stack_on_the_centre_pixel():
    """g = exp(0) = 1 on the mean's pixel: w_k = a_k * (1 - A) with A byte-quantised after every fragment."""
    alphas = [0.75, 0.5, 0.25, 0.9]
    q = stack(alphas, half_px=0.6)                           # every quad covers the one pixel its mean sits on
    s = splat_ref.setup(q, W, H)
    fq, fp, rank = contrib_ref.fragments(s)
    centre = 7 * W + 5
    assert np.array_equal(fq[fp == centre], np.arange(4)) and np.array_equal(rank[fp == centre], np.arange(4))
    A = f32(0.0)
    want = []
    for a in alphas:
        w = f32(a) * (f32(1.0) - A)
        want.append(w)
        A = u8(w + A)
    c = contrib_ref.contrib(q, W, H, count_weight=0.0)
    assert np.array_equal(c["wmax"], np.array(want, np.float32).view(np.uint32))
    assert c["alpha"][7, 5] == int(np.rint(A * f32(255)))
    # 0.75 -> 191/255; 0.5 * (64/255) -> A = 223/255; by hand
    assert want[0] == f32(0.75) and want[1] == f32(0.5) * (f32(1.0) - f32(191.0) / f32(255.0))


def test_opaque_first_quad_leaves_nothing_behind():
    q = stack([1.0, 0.8, 0.6], px=16, py=12)
    q[0, 4], q[0, 7] = f32(8.0 / (W * 0.5)), f32(8.0 / (H * 0.5))        # the opaque quad covers the others; flat conic: g = 1 everywhere
    q[0, 12:15] = 0.0
    c = contrib_ref.contrib(q, W, H, count_weight=0.0)
    assert c["wmax"][0] == np.float32(1.0).view(np.uint32)
    assert c["wmax"][1] == 0 and c["wmax"][2] == 0
    assert c["n_lo"][1] == 0 and c["n_hi"][2] == 0 and c["n_lo"][0] == 16 * 16


def test_counts_bracket_the_threshold():
    q = stack([0.3, 0.3])
    c0 = contrib_ref.contrib(q, W, H, count_weight=0.25, bar=0.0)
    c1 = contrib_ref.contrib(q, W, H, count_weight=0.25, bar=0.05)
    assert np.array_equal(c0["n_lo"], c0["n_hi"])
    assert (c1["n_lo"] <= c0["n_lo"]).all() and (c0["n_hi"] <= c1["n_hi"]).all() and (c1["n_lo"] < c1["n_hi"]).any()
    # strict comparison: a weight equal to the threshold does not count
    one = stack([0.5])
    assert contrib_ref.contrib(one, W, H, count_weight=0.5)["n_lo"][0] == 0
    assert contrib_ref.contrib(one, W, H, count_weight=np.nextafter(f32(0.5), f32(0)))["n_lo"][0] == 1


def test_alpha_plane_is_the_splat_restatements():
    for mode in (0, 5):
        q = splat_ref.random_quads(120, W, H, seed=3, max_px=9.0)
        q[7, 0] = np.nan                                     # a skipped quad contributes nothing
        q[9, 4] = 1e9
        s = splat_ref.setup(q, W, H)
        planes, skipped = splat_ref.render(q, W, H, mode=mode, s=s)
        c = contrib_ref.contrib(q, W, H, s=s)
        assert skipped == 2 and c["wmax"][7] == 0 and c["wmax"][9] == 0 and c["n_hi"][7] == 0
        assert np.array_equal(c["alpha"], planes[2][:, :, 3])
        assert (c["wmax"].view(np.float32) <= 1.0).all() and c["wmax"].any()


def test_per_record_folds_quads():
    c = dict(wmax=np.array([3, 9, 4], np.uint32), n=np.array([2, 2, 3]), n_lo=np.array([1, 2, 3]), n_hi=np.array([2, 3, 4]))
    r = contrib_ref.per_record(c, [4, 1, 4], 6)
    assert r["wmax"].tolist() == [0, 9, 0, 0, 4, 0] and r["n_lo"].tolist() == [0, 2, 0, 0, 4, 0] and r["n_hi"].tolist() == [0, 3, 0, 0, 6, 0]
    assert r["n"].tolist() == [0, 2, 0, 0, 5, 0]


def test_a_head_on_view_of_flat_isotropic_gaussians_loses_quads_to_nan_axes(oracle):
    """Why a wall seen exactly head-on shows records of weight 0 that nothing hides.  The conversion gives a texel's Gaussian two equal
    scales and a flat third; seen along the wall's normal its screen-space covariance has c00 == c11 and c01 == 0 up to rounding, so the
    reference's eigenvector formula (gaussianSplattingPrepassCS.glsl:185, dvy = (-c00 + c01 + l1) / (c01 - c11 + l1)) is 0 / 0, or
    x / 0 followed by inf * 0, whenever c11 >= c00 as rounded: the quad's axes are NaN, the pinned rasteriser skips the quad (OpenGL
    discards the triangle), and the record adds nothing to that view — no fragment, hence weight 0.  On the front wall, which nothing
    hides, the zero weights are exactly those quads; a view pitched by 5 degrees (c00 > c11) has none."""
    import prune_cases as pc
    _, rec, _ = oracle.convert(pc.two_walls(), pc.WALL_R, cap=0)
    rec = np.ascontiguousarray(rec, np.float32).reshape(-1, 24)
    front = rec[:, 2] > 0
    assert np.array_equal(np.unique(rec[:, 8:10]), np.unique(rec[:, 8]))        # (one scale for both in-plane axes of every record)
    W, H = pc.WALL_SIZE
    q, src = pc.sorted_with_sources(oracle, pc.wall_params(0.0), rec)
    nan_axes = np.isnan(q[:, 4:8]).any(1)
    assert np.array_equal(splat_ref.setup(q, W, H)["skip"], nan_axes)
    w = contrib_ref.contrib(q, W, H)["wmax"]
    is_front = front[src]
    assert not w[nan_axes].any() and np.array_equal(w[is_front] == 0, nan_axes[is_front])
    assert nan_axes[is_front].sum() > front.sum() // 4                           # (a large share of the FRONT wall)
    q5, _ = pc.sorted_with_sources(oracle, pc.wall_params(), rec)
    assert not np.isnan(q5).any() and not splat_ref.setup(q5, W, H)["skip"].any()
