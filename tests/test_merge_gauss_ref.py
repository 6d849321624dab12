"""CPU: the restatement of the merge pass under M2S_MERGE_MODEL_GAUSSIAN (tests/merge_gauss_ref.py; include/m2s.h pins 2g, 5g, 5sg, 4g)
against values derived by hand from dyadic operands, the condition on its own eigen-solver, the ABI of the switch without a device,
and m2s_read_ply_sh (host code) against m2s_write_ply_sh, a file of the reference's writer and hand-made headers."""
import ctypes as C
import os

import numpy as np
import pytest

import merge_gauss_ref as mg
import merge_ref as mr
from mesh2splat_amd import _lib, gltf_io

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_host")


def records(n, scale, alpha=0.25):
    """n records at the origin: the identity rotation (rows = the coordinate axes), dyadic colours"""
    r = np.zeros((n, 24), F)
    r[:, 3] = 1
    r[:, 4:8] = (0.5, 0.25, 0.75, alpha)
    r[:, 8:11] = scale
    r[:, 11] = 1
    r[:, 14] = 1
    r[:, 16] = 1
    r[:, 20:22] = (0.5, 0.125)
    return r


def test_the_identity_rotation_has_the_coordinate_axes_as_rows():
    rows = mg.rows_f32(records(1, 1.0)[:, 16:20])[0]
    assert np.array_equal(rows, np.eye(3, dtype=F))


def test_two_coincident_identical_records_keep_their_scales_and_add_their_alpha():
    for alpha, want in ((0.25, 0.5), (0.75, 1.0)):
        r = records(2, (0.5, 0.25, 0.125), alpha)
        r[:, 0:3] = (0.5, -0.25, 2.0)
        out, info = mg.parent(r, 1.0)
        assert np.array_equal(out[8:11], r[0, 8:11]) and np.array_equal(out[0:3], r[0, 0:3])
        assert out[7] == F(want)
        assert np.array_equal(out[4:7], r[0, 4:7]) and np.array_equal(out[20:22], r[0, 20:22]) and np.array_equal(out[12:15], r[0, 12:15])
        assert np.array_equal(out[16:20], np.array([1, 0, 0, 0], F))
        assert all(out[k] == r[0, k] for k in mg.COPIED)


@pytest.mark.parametrize("s,sigma,want", ((0.75, 1.0, (1.25, 0.75, 0.75)), (0.375, 2.0, (0.625, 0.375, 0.375))))
def test_two_isotropic_records_one_unit_either_side(s, sigma, want):
    """C = sigma^2 s^2 I = 0.5625 I, the spread adds 1 along x: M = diag(1.5625, 0.5625, 0.5625), already diagonal"""
    r = records(2, s)
    r[0, 0], r[1, 0] = -1.0, 1.0
    out, info = mg.parent(r, sigma)
    assert np.array_equal(out[8:11], np.array(want, F))
    assert np.array_equal(out[0:3], np.zeros(3, F))
    assert np.array_equal(np.abs(info["E"][:, 0]), (1.0, 0.0, 0.0))
    assert np.array_equal(info["M"], np.diag((1.5625, 0.5625, 0.5625)))
    # alpha-weighted area: 2 a alpha / a_p with a = s^2 (two largest of three equal scales)
    assert out[7] == F(2 * s * s * 0.25 / (want[0] * want[1]))


def test_a_two_by_two_block_of_flat_records():
    h, s = 2.0 ** -3, 2.0 ** -4
    r = records(4, (s, s, 0.0))
    r[:, 0] = (0, h, 0, h)
    r[:, 1] = (0, 0, h, h)
    out, info = mg.parent(r, 1.0)
    assert info["l"][0] == info["l"][1] == s * s + h * h / 4 and info["l"][2] == 0.0
    assert out[8] == out[9] == F(np.sqrt(s * s + h * h / 4)) and out[10] == 0.0
    assert np.array_equal(out[0:3], np.array((h / 2, h / 2, 0), F))
    assert np.array_equal(np.abs(info["E"][:, 2]), (0.0, 0.0, 1.0))


def test_the_run_rule_reads_the_row_of_the_smallest_scale():
    """two records whose third rows agree and whose first rows are perpendicular (a quarter turn about z)"""
    r = records(2, 1.0)
    r[1, 16:20] = mr.quat_cast_wxyz((0, 1, 0), (-1, 0, 0), (0, 0, 1)).astype(F)
    rows = mg.rows_f32(r[:, 16:20])
    assert np.allclose(rows[1], ((0, 1, 0), (-1, 0, 0), (0, 0, 1)), atol=1e-6)
    for scale, axis, after in (((0.01, 1, 1), 0, 2), ((1, 0.01, 1), 1, 2), ((1, 1, 0.01), 2, 1), ((1, 1, 0), 2, 1)):
        r[:, 8:11] = scale
        assert list(mg.axis_index(r[:, 8:11])) == [axis, axis]
        assert mg.merge(r, 10, 4, 0.5)[2]["after"] == after, scale
        assert mr.merge(r, 10, 4, 0.5)[2]["after"] == 1                   # (the footprint's rule: r_3 whatever the scales)
    # ties go to the lower index; the rule is sign-free
    assert list(mg.axis_index(np.array([(1, 1, 1), (2, 1, 1), (2, 1, 3), (1, 2, 1), (0, 0, 0)], F))) == [0, 1, 1, 0, 0]
    r[:, 8:11] = (1, 1, 0.01)
    r[1, 16:20] = mr.quat_cast_wxyz((1, 0, 0), (0, -1, 0), (0, 0, -1)).astype(F)  # r_3 = -z
    assert mg.merge(r, 10, 4, 0.5)[2]["after"] == 1 and mr.merge(r, 10, 4, 0.5)[2]["after"] == 2


def test_the_generator_has_what_it_promises():
    rec = mg.gauss_records(4099, 1)
    s = rec[:, 8:11]
    ok = mr.cr.valid_mask(rec)
    assert (~ok).sum() == 3
    flat = (s[:, 2] == 0) & (s[:, 0] > 0)
    iso = (s[:, 0] == s[:, 1]) & (s[:, 1] == s[:, 2]) & (s[:, 0] > 0)
    assert flat.sum() > 300 and iso.sum() > 300 and ((s == 0).all(1)).sum() > 100
    assert all((mg.axis_index(s) == k).sum() > 500 for k in range(3))
    assert len(np.unique(rec[:, 0:3], axis=0)) < len(rec) // 2           # shared positions


@pytest.mark.parametrize("sigma", (1.0, 0.65))
def test_the_eigenpairs_rebuild_the_moment(sigma):
    """the condition on the restatement itself: V diag(l) V^T = M within 1e-12 l1 on every segment of the generator's inputs, the
    eigenvectors orthonormal and the iteration at rest before its sweeps run out"""
    worst, segs = 0.0, 0
    for n, level, group in ((257, 10, 64), (4099, 3, 5), (4099, 10, 2)):
        rec = mg.gauss_records(n, n)
        _, _, _, info = mg.merge(rec, level, group, -2.0, sigma)
        for i in info:
            if i is None:
                continue
            M, E, l = i["M"], i["E"], i["l"]
            assert np.isfinite(M).all() and l[0] >= l[1] >= l[2] >= 0
            _, _, sweeps = mg.jacobi(*(float(M[a, b]) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))))
            assert sweeps < mg.JACOBI_SWEEPS
            if l[0] == 0:
                assert not M.any()
                continue
            worst = max(worst, np.abs(E @ np.diag(l) @ E.T - M).max() / l[0], np.abs(E.T @ E - np.eye(3)).max())
            segs += 1
    print(f"sigma {sigma}: {segs} segments, rebuild / orthonormality within {worst:.2e}")
    assert segs > 500 and worst <= 1e-12


def test_counts_are_monotone_in_level_and_the_parents_are_valid():
    rec = mg.gauss_records(1500, 3)
    prev, finest = None, None
    for level in range(11):
        out, mp, counts, _ = mg.merge(rec, level, 4, 0.5, 0.65)
        assert counts["before"] == 1500 and counts["invalid"] == 3 and len(out) == counts["after"]
        assert prev is None or counts["after"] <= prev
        prev = counts["after"]
        finest = prev if finest is None else finest
        assert mr.cr.valid_mask(out).sum() == len(out) - 3
        assert np.array_equal(np.unique(mp), np.arange(len(out)))
    assert prev < finest < 1500


def test_the_unsigned_flag_has_nothing_to_change_and_bounds_read_three_scales():
    rec = mg.gauss_records(300, 5)
    b = mg.bounds(rec, 0.65)
    ok = mr.cr.valid_mask(rec)
    assert np.array_equal(b[ok, 3], (F(0.65) * rec[ok, 8:11].max(1)).astype(F)) and np.array_equal(b[:, 0:3].view(np.uint32), rec[:, 0:3].view(np.uint32))
    assert (b[ok, 3] != mr.F(0.65) * np.maximum(rec[ok, 8], rec[ok, 9])).any()


def test_abi_symbols_exist_and_null_contexts_are_refused(hiplib):
    assert hiplib.m2s_set_merge_model(None, 1, 1.0) == 1 and hiplib.m2s_set_merge_model(None, 0, 1.0) == 1
    assert hiplib.m2s_merge_model(None) == 0 and hiplib.m2s_merge_sigma(None) == 1.0
    n, pbr, deg = C.c_uint64(), C.c_int(), C.c_uint32()
    rec, sh = C.c_void_p(), C.c_void_p()
    assert hiplib.m2s_read_ply_sh(None, C.byref(rec), C.byref(n), C.byref(pbr), C.byref(sh), C.byref(deg)) == 1
    assert hiplib.m2s_read_ply_sh(b"x.ply", C.byref(rec), C.byref(n), C.byref(pbr), None, C.byref(deg)) == 1
    assert hiplib.m2s_read_ply_sh(b"x.ply", C.byref(rec), C.byref(n), C.byref(pbr), C.byref(sh), None) == 1
    assert hiplib.m2s_read_ply_sh(b"/nonexistent/x.ply", C.byref(rec), C.byref(n), C.byref(pbr), C.byref(sh), C.byref(deg)) == 6
    assert not rec.value and not sh.value
    hiplib.m2s_free_sh(None)
    from mesh2splat_amd import merge
    assert merge.MODELS == ("footprint", "gaussian")
    import mesh2splat_amd
    assert mesh2splat_amd.read_ply_sh is gltf_io.read_ply_sh


# ---- m2s_read_ply_sh ----------------------------------------------------------------------------------------------------------------------
def plane_of_degree(n, degree, seed):
    rng = np.random.default_rng(seed)
    sh = np.zeros((n, 48), F)
    sh[:, 0:3] = rng.normal(0, 1, (n, 3))
    c = (degree + 1) ** 2 - 1
    for ch in range(3):
        sh[:, 3 + 15 * ch:3 + 15 * ch + c] = rng.normal(0, 0.3, (n, c))
    return sh


@pytest.mark.parametrize("degree", (0, 1, 2, 3))
def test_read_ply_sh_round_trips_write_ply_sh(hiplib, tmp_path, degree):
    """m2s_write_ply_sh always writes the 45 f_rest properties (coefficients above the plane's degree are its zeros), so the file says
    degree 3; the rows come back bit for bit, the records as m2s_read_ply reads them"""
    n = 37
    rec = mg.gauss_records(n, 2, invalid=False)
    rec[:, 8:11] = np.maximum(rec[:, 8:11], F(1e-3))
    sh = plane_of_degree(n, degree, degree)
    path = str(tmp_path / "sh.ply")
    assert hiplib.m2s_write_ply_sh(os.fsencode(path), rec.ctypes.data, sh.ctypes.data, n, 1.0) == 0
    plain, pbr0 = gltf_io.read_ply(path)
    got, pbr, plane, deg = gltf_io.read_ply_sh(path)
    assert deg == 3 and pbr == pbr0 and plane.dtype == F and plane.shape == (n, 48)
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))
    assert np.array_equal(plane.view(np.uint32), sh.view(np.uint32))
    assert np.array_equal(got[:, 0:3].view(np.uint32), rec[:, 0:3].view(np.uint32))
    assert np.array_equal(got[:, 4:7], (sh[:, 0:3] * F(0.28209479177387814) + F(0.5)).astype(F))


def test_read_ply_sh_on_a_file_of_the_reference_writer():
    path = os.path.join(GOLD, "pipe_soup_R32.ply")
    header = open(path, "rb").read(4096).split(b"end_header")[0].decode()
    n_rest = header.count("property float f_rest_")
    assert n_rest in (0, 9, 24, 45)
    plain, pbr0 = gltf_io.read_ply(path)
    got, pbr, plane, deg = gltf_io.read_ply_sh(path)
    assert deg == {0: 0, 9: 1, 24: 2, 45: 3}[n_rest] and pbr == pbr0
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)) and plane.shape == (len(got), 48)
    assert np.array_equal(got[:, 4:7], (plane[:, 0:3] * F(0.28209479177387814) + F(0.5)).astype(F))


def handmade(path, n_rest, rows, names=None, ascii_body=False, rest_type="float"):
    names = names if names is not None else [f"f_rest_{k}" for k in range(n_rest)]
    props = ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2"] + names + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    head = "ply\nformat " + ("ascii" if ascii_body else "binary_little_endian") + f" 1.0\nelement vertex {len(rows)}\n"
    head += "".join(f"property {rest_type if p in names else 'float'} {p}\n" for p in props) + "end_header\n"
    rows = np.ascontiguousarray(rows, F)
    assert rows.shape[1] == len(props)
    with open(path, "wb") as f:
        f.write(head.encode())
        if ascii_body:
            f.write("".join(" ".join(repr(float(v)) for v in row) + "\n" for row in rows).encode())
        else:
            f.write(rows.tobytes())


@pytest.mark.parametrize("ascii_body", (False, True))
@pytest.mark.parametrize("n_rest,degree", ((0, 0), (9, 1), (24, 2), (45, 3)))
def test_read_ply_sh_places_the_channels_of_every_degree(tmp_path, n_rest, degree, ascii_body):
    n = 5
    rng = np.random.default_rng(n_rest)
    rows = rng.normal(0, 1, (n, 14 + n_rest)).astype(F)
    path = str(tmp_path / "h.ply")
    handmade(path, n_rest, rows, ascii_body=ascii_body)
    got, pbr, plane, deg = gltf_io.read_ply_sh(path)
    assert deg == degree and not pbr and len(got) == n
    want = np.zeros((n, 48), F)
    want[:, 0:3] = rows[:, 3:6]
    c = n_rest // 3
    for ch in range(3):
        want[:, 3 + 15 * ch:3 + 15 * ch + c] = rows[:, 6 + ch * c:6 + (ch + 1) * c]
    assert np.array_equal(plane.view(np.uint32), want.view(np.uint32))
    assert not np.signbit(plane[:, 3 + c:18]).any()                         # rows above the degree hold +0
    assert np.array_equal(got.view(np.uint32), gltf_io.read_ply(path)[0].view(np.uint32))


def test_read_ply_sh_refuses_other_counts_and_odd_names(tmp_path):
    path = str(tmp_path / "bad.ply")
    rows = np.zeros((2, 24), F)
    handmade(path, 10, rows)
    with pytest.raises(_lib.M2SError, match="0, 9, 24, 45"):
        gltf_io.read_ply_sh(path)
    assert len(gltf_io.read_ply(path)[0]) == 2                               # (m2s_read_ply never looked at them)
    handmade(path, 9, np.zeros((2, 23), F), names=[f"f_rest_{k}" for k in (0, 1, 2, 3, 4, 5, 6, 7, 9)])
    with pytest.raises(_lib.M2SError, match="f_rest"):
        gltf_io.read_ply_sh(path)
    handmade(path, 9, np.zeros((2, 23), F), rest_type="int")
    with pytest.raises(_lib.M2SError, match="f_rest"):
        gltf_io.read_ply_sh(path)
    # zero rows: no plane, the header's degree
    handmade(path, 24, np.zeros((0, 38), F))
    got, pbr, plane, deg = gltf_io.read_ply_sh(path)
    assert len(got) == 0 and plane is None and deg == 2


def test_read_ply_sh_of_a_compact_file_has_no_plane(tmp_path):
    from mesh2splat_amd.converter import write_ply_compact
    rec = mr.crafted_records(100, 3, invalid=False)
    rec[:, 8:11] = np.maximum(rec[:, 8:11], F(1e-3))
    path = str(tmp_path / "c.ply")
    write_ply_compact(path, rec, 1.0)
    got, pbr, plane, deg = gltf_io.read_ply_sh(path)
    assert plane is None and deg == 0 and len(got) == 100
    assert np.array_equal(got.view(np.uint32), gltf_io.read_ply(path)[0].view(np.uint32))
