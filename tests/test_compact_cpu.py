"""CPU: the compact .ply (include/m2s.h "compact export") — m2s_write_ply_compact against the numpy restatement tests/compact_ref.py, byte
for byte, on every edge of the pin; the header text; the round trip through m2s_read_ply within the quantisation bounds; malformed files;
that format-0 files read back as before; the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import compact_ref as cr
from mesh2splat_amd import _lib, gltf_io
from mesh2splat_amd.converter import write_ply, write_ply_compact

F = np.float32
CASES = cr.cases()


def host_file(tmp_path, rec, sm, sh=None, degree=0):
    p = str(tmp_path / "c.ply")
    counts = write_ply_compact(p, rec, sm, sh, degree)
    return open(p, "rb").read(), counts, p


def test_symbols_exported(hiplib):
    for name in ("m2s_write_ply_compact", "m2s_export_ply_compact", "m2s_last_compact_stage_ms"):
        assert hasattr(hiplib, name) and name in _lib.EXPORTS
    assert hiplib.m2s_abi_version() == 1
    import mesh2splat_amd
    assert mesh2splat_amd.write_ply_compact is write_ply_compact


def test_signatures_are_struct_free():
    src = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "m2s.h")).read()
    for name in ("m2s_write_ply_compact", "m2s_export_ply_compact", "m2s_last_compact_stage_ms"):
        decl = re.search(r"m2s_status " + name + r"\(([^;]*)\);", src).group(1)
        assert "struct" not in decl and "params" not in decl


def test_null_arguments(hiplib, tmp_path):
    rec = cr.make_records(3)
    path = os.fsencode(str(tmp_path / "x.ply"))
    counts = (C.c_uint64 * 3)()
    assert hiplib.m2s_write_ply_compact(None, rec.ctypes.data, None, 0, 3, C.c_float(1), counts) == 1
    assert hiplib.m2s_write_ply_compact(path, None, None, 0, 3, C.c_float(1), counts) == 1
    assert hiplib.m2s_write_ply_compact(path, rec.ctypes.data, rec.ctypes.data, 4, 3, C.c_float(1), counts) == 1     # degree above 3
    assert hiplib.m2s_write_ply_compact(path, rec.ctypes.data, None, 0, 3, C.c_float(1), None) == 0                  # counts are optional
    assert hiplib.m2s_write_ply_compact(os.fsencode(str(tmp_path / "no" / "dir.ply")), rec.ctypes.data, None, 0, 3, C.c_float(1), counts) == 6
    assert hiplib.m2s_export_ply_compact(None, path, C.c_float(0.65), 0, counts) == 1                                # null context
    ms = (C.c_float * 4)()
    assert hiplib.m2s_last_compact_stage_ms(None, ms) == 1


@pytest.mark.parametrize("name", list(CASES))
def test_host_writer_equals_restatement(hiplib, tmp_path, name):
    rec, sm = CASES[name]
    got, counts, _ = host_file(tmp_path, rec, sm)
    ref, rc, _ = cr.encode(rec, sm)
    assert counts == rc and counts["rows"] + counts["skipped"] == len(rec) and counts["chunks"] == (counts["rows"] + 255) // 256
    assert got == ref


def test_cases_reach_the_edges_they_claim(hiplib):
    """the restatement's own intermediate values on the named cases: each edge of the pin is really taken"""
    rec, sm = CASES["zero_extent"]
    _, table, rows, _ = cr.parse(cr.encode(rec, sm)[0])
    assert (rows[:, 0] == 0).all() and np.array_equal(table[:, 0:3], table[:, 3:6])
    rec, sm = CASES["duplicates"]
    _, _, perm = cr.encode(rec, sm)
    key = perm % 3                                           # three positions: within one, record order is kept
    for k in range(3):
        assert (np.diff(perm[key == k]) > 0).all()
    rec, sm = CASES["tiny_range"]
    _, table, rows, _ = cr.parse(cr.encode(rec, sm)[0])
    d = table[:, 3:6] - table[:, 0:3]
    assert ((d > 0) & (d < 1e-5)).any() and (rows[:256, 0] == 0).all()
    rec, sm = CASES["scales"]
    _, table, rows, _ = cr.parse(cr.encode(rec, sm)[0])
    assert table[:, 6:9].min() == -20 and table[:, 9:12].max() == 20 and (table[:, 8] == -20).all() and (table[:, 11] == -20).all()
    rec, sm = CASES["quaternions"]
    _, _, perm = cr.encode(rec, sm)
    _, _, rows, _ = cr.parse(cr.encode(rec, sm)[0])
    L = {int(src): int(rows[i, 1] >> 30) for i, src in enumerate(perm)}
    assert [L[k] for k in range(6)] == [0, 0, 1, 1, 3, 3]


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_element(hiplib, tmp_path, degree):
    rec, sm = CASES["hostile"]
    sh = cr.sh_plane(len(rec), degree)
    got, counts, _ = host_file(tmp_path, rec, sm, sh, degree)
    ref, rc, perm = cr.encode(rec, sm, sh, degree)
    assert got == ref and counts == rc
    head, table, rows, shb = cr.parse(got)
    K = (degree + 1) ** 2 - 1
    assert shb.shape == (counts["rows"], 3 * K) and ("element sh" in head) == (degree > 0)
    if degree:
        # the clamp and the trunc edges: +-4 and beyond, the last value below 4, -0
        want = {4.0: 255, 5.0: 255, 100.0: 255, -4.0: 0, -5.0: 0, -100.0: 0, 3.96875: 255, -3.96875: 1, 0.0: 128, 0.03125: 129, -0.03125: 127}
        for v, b in want.items():
            assert cr.sh_bytes(np.full((1, 48), v, F), degree)[0, 0] == b, (v, b)
        assert shb.min() == 0 and shb.max() == 255
    # the colour comes from the plane's DC term
    assert not np.array_equal(rows[:, 3], cr.parse(cr.encode(rec, sm)[0])[2][:, 3])


def test_header_text_is_exact(hiplib, tmp_path):
    rec, sm = CASES["n257"]
    got, _, _ = host_file(tmp_path, rec, sm, cr.sh_plane(257), 1)
    want = ("ply\nformat binary_little_endian 1.0\nelement chunk 2\n" + "".join(f"property float {p}\n" for p in cr.CHUNK_PROPS) +
            "element vertex 257\nproperty uint packed_position\nproperty uint packed_rotation\nproperty uint packed_scale\nproperty uint packed_color\n"
            "element sh 257\n" + "".join(f"property uchar f_rest_{i}\n" for i in range(9)) + "end_header\n").encode()
    assert got.startswith(want) and len(got) == len(want) + 2 * 72 + 257 * 16 + 257 * 9
    empty, counts, _ = host_file(tmp_path, cr.make_records(0), 1.0)
    assert counts == {"rows": 0, "chunks": 0, "skipped": 0} and empty.endswith(b"end_header\n") and b"element chunk 0\n" in empty and b"element vertex 0\n" in empty


def test_round_trip_within_the_quantisation_bounds(hiplib, tmp_path):
    """Bounds: a value v of a chunk with range r = hi - lo is stored as round(v' * t) with t levels, so it comes back within r / (2 t)
    (t = 2047, 1023 for y, 255 for colour and alpha; a chunk with r < 1e-5 stores 0 and comes back as lo: within r); a quaternion
    component a is stored as round((a / sqrt(2) + 0.5) * 1023): within sqrt(2) / 2046; each plus 1e-6 relative for the fp32 arithmetic
    of the encoder and the decoder."""
    rec, sm = CASES["hostile"]
    sm = F(sm)
    data, counts, path = host_file(tmp_path, rec, sm)
    _, _, perm = cr.encode(rec, sm)
    back, pbr = gltf_io.read_ply(path)
    assert not pbr and back.shape == (counts["rows"], 24)
    src = rec[perm].astype(np.float64)
    _, table, _, _ = cr.parse(data)
    t = table[np.arange(len(perm)) // 256].astype(np.float64)
    levels = np.array([2047.0, 1023.0, 2047.0])

    def bound(lo, hi, lv, ref):
        r = hi - lo
        return np.where(r < 1e-5, r, r / (2 * lv)) + 1e-6 * np.maximum(np.abs(ref), np.maximum(np.abs(lo), np.abs(hi)))
    err = np.abs(back[:, 0:3] - src[:, 0:3])
    assert (err <= bound(t[:, 0:3], t[:, 3:6], levels, src[:, 0:3])).all(), err.max()
    ls = np.clip(cr.logf(rec[perm][:, 8:11] * sm).astype(np.float64), -20, 20)
    with np.errstate(divide="ignore"):
        err = np.abs(np.log(back[:, 8:11].astype(np.float64)) - ls)
    assert (err <= bound(t[:, 6:9], t[:, 9:12], levels, ls) + 1e-6 * 20).all(), err.max()
    err = np.abs(back[:, 4:7] - src[:, 4:7])
    assert (err <= bound(t[:, 12:15], t[:, 15:18], 255.0, src[:, 4:7])).all(), err.max()
    assert (np.abs(back[:, 7] - np.clip(src[:, 7], 0, 1)) <= 1 / 510 + 1e-6).all()
    q = src[:, 16:20] / np.linalg.norm(src[:, 16:20], axis=1, keepdims=True)
    L = np.argmax(np.abs(rec[perm][:, 16:20] / np.sqrt((rec[perm][:, 16:20].astype(np.float64) ** 2).sum(1))[:, None].astype(F)), axis=1)
    q = np.where((q[np.arange(len(q)), L] < 0)[:, None], -q, q)
    others = np.ones_like(q, bool)
    others[np.arange(len(q)), L] = False
    err = np.abs(back[:, 16:20] - q)
    assert (err[others] <= np.sqrt(2) / 2046 + 1e-6).all(), err[others].max()
    # the rebuilt component: from three others each within e, |m - q_L| <= (3 e + 3 e^2) / m for m >= 1/2 (the largest of four)
    e = np.sqrt(2) / 2046 + 1e-6
    assert (err[~others] <= 2 * (3 * e + 3 * e * e) + 1e-6).all(), err[~others].max()
    assert (back[:, 3] == 1).all() and (back[:, 11] == 1).all() and (back[:, 12:16] == 0).all() and (back[:, 20:24] == 0).all()
    # the reader's values are the restatement's decoder's
    pos, dls, col, alpha, dq, _ = cr.decode(data)
    assert np.allclose(back[:, 0:3], pos, rtol=1e-6, atol=1e-6) and np.allclose(back[:, 4:7], col, rtol=1e-6, atol=1e-6)
    assert np.allclose(back[:, 16:20], dq, rtol=0, atol=1e-5) and np.allclose(back[:, 7], alpha, atol=1e-7)


def test_sh_element_is_ignored_by_the_reader(hiplib, tmp_path):
    rec, sm = CASES["n785"]
    _, _, p = host_file(tmp_path, rec, sm)
    plain, _ = gltf_io.read_ply(p)
    _, _, p = host_file(tmp_path, rec, sm, cr.sh_plane(785) * 0, 3)
    baked, _ = gltf_io.read_ply(p)
    assert np.array_equal(plain[:, [0, 1, 2, 7, 8, 9, 10, 16, 17, 18, 19]], baked[:, [0, 1, 2, 7, 8, 9, 10, 16, 17, 18, 19]])
    assert np.allclose(baked[:, 4:7], 0.5)


def read_status(hiplib, path):
    rec, n, pbr = C.c_void_p(), C.c_uint64(), C.c_int()
    st = hiplib.m2s_read_ply(os.fsencode(path), C.byref(rec), C.byref(n), C.byref(pbr))
    if st == 0:
        hiplib.m2s_free_records(rec)
    return st, n.value


def test_malformed_files_are_refused(hiplib, tmp_path):
    rec, sm = CASES["n785"]
    data, _, _ = host_file(tmp_path, rec, sm, cr.sh_plane(785), 2)
    p = str(tmp_path / "bad.ply")

    def status(b):
        open(p, "wb").write(b)
        return read_status(hiplib, p)
    assert status(data) == (0, 785)
    assert status(data.replace(b"element chunk 4\n", b"element chunk 3\n"))[0] in (1, 6)            # fewer chunks than ceil(N / 256)
    assert status(data.replace(b"element chunk 4\n", b"element chunk 0\n"))[0] in (1, 6)
    for cut in (1, 785 * 24 - 1, 785 * 24 + 1, 785 * 40, len(data) - data.index(b"end_header\n") - 11):
        assert status(data[:-cut])[0] in (1, 6), cut                                                   # a truncated body (the sh element included)
    for big in (b"9223372036854775808", b"18446744073709551615", b"99999999999999999999999", b"-1", b"x"):
        assert status(data.replace(b"element vertex 785\n", b"element vertex " + big + b"\n"))[0] in (1, 6), big
        assert status(data.replace(b"element chunk 4\n", b"element chunk " + big + b"\n"))[0] in (1, 6), big
        assert status(data.replace(b"element sh 785\n", b"element sh " + big + b"\n"))[0] in (1, 6), big
    assert status(data.replace(b"property float max_b\n", b"property uchar max_b\n"))[0] in (1, 6)
    assert status(data.replace(b"property float max_b\n", b"property list uchar int max_b\n"))[0] in (1, 6)
    assert status(data.replace(b"binary_little_endian", b"binary_big_endian"))[0] in (1, 6)
    assert status(data.replace(b"element vertex 785\n", b"element vertex 0\n"))[0] in (0, 1, 6)


def test_format0_files_read_back_as_before(hiplib, tmp_path):
    rec = cr.make_records(300, 21)
    p = str(tmp_path / "f0.ply")
    write_ply(p, rec, 0, 0.01)
    back, pbr = gltf_io.read_ply(p)
    assert not pbr and back.shape == (300, 24)
    # what parsers::loadPlyFile rebuilds, bit for bit: positions as written, the rotation normalised, scale = exp(log(scale * sm))
    assert np.array_equal(back[:, 0:3].view(np.uint32), rec[:, 0:3].view(np.uint32))
    sc = np.array([np.exp(v) for v in cr.logf(rec[:, 8:11] * F(0.01)).ravel()], F).reshape(-1, 3)
    assert np.allclose(back[:, 8:11], sc, rtol=2e-7, atol=0)
    golden = os.path.join(os.path.dirname(__file__), "golden", "ref_host")
    for name in ("ref_fmt0.ply", "ref_fmt1.ply"):
        assert read_status(hiplib, os.path.join(golden, name)) == (0, 120)


def test_golden_file_is_reproduced(hiplib, tmp_path):
    """a file written when the format was defined: the writer and the restatement still produce its bytes from the stored records"""
    gold = os.path.join(os.path.dirname(__file__), "golden", "compact")
    rec, sh = np.load(os.path.join(gold, "records.npy")), np.load(os.path.join(gold, "sh.npy"))
    want = open(os.path.join(gold, "hostile300_sh1.ply"), "rb").read()
    sm = F(0.65) / F(64)
    got, counts, _ = host_file(tmp_path, rec, sm, sh, 1)
    assert got == want and cr.encode(rec, sm, sh, 1)[0] == want and counts == {"rows": 286, "chunks": 2, "skipped": 14}
