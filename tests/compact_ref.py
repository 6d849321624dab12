"""The compact .ply of include/m2s.h ("compact export") restated in numpy: fp32 operation by operation, logf from the C library through
ctypes, the sort np.argsort(kind="stable").  encode() gives the file's bytes, parse() / decode() take a file apart again, cases() are
the record sets the CPU and the GPU tests share."""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]

CHUNK_PROPS = ("min_x min_y min_z max_x max_y max_z min_scale_x min_scale_y min_scale_z max_scale_x max_scale_y max_scale_z "
               "min_r min_g min_b max_r max_g max_b").split()
POS, COL, SCL, NRM, ROT, PBR = (slice(4 * k, 4 * k + 4) for k in range(6))


def logf(a):
    a = np.asarray(a, F)
    return np.array([_libm.logf(float(v)) for v in a.ravel()], F).reshape(a.shape)


def ordk(v):
    """the order of every min / max: the real line, -0 below +0"""
    u = np.ascontiguousarray(v, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unordk(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F)


def omin(v, axis=0):
    return unordk(ordk(v).min(axis=axis))


def omax(v, axis=0):
    return unordk(ordk(v).max(axis=axis))


def valid_mask(rec):
    with np.errstate(all="ignore"):
        fin = np.isfinite(rec[:, 0:3]).all(1) & np.isfinite(rec[:, COL]).all(1) & np.isfinite(rec[:, 8:11]).all(1) & np.isfinite(rec[:, ROT]).all(1)
        q = rec[:, ROT]
        n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        return fin & (rec[:, 8:11] >= 0).all(1) & np.isfinite(n2) & (n2 > 0)


def part1by2(x):
    x = x.astype(np.uint32) & np.uint32(0x3FF)
    x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
    x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
    x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def keys_of(p, bmin, bmax):
    cells = []
    with np.errstate(all="ignore"):
        for a in range(3):
            ext = F(bmax[a] - bmin[a])
            if not ext > 0:
                cells.append(np.zeros(len(p), np.uint32))
                continue
            f = np.floor(((p[:, a] - bmin[a]) / ext) * F(1024.0))
            cells.append(np.where(f >= 1023, 1023, np.where(f > 0, f, 0)).astype(np.uint32))
    return part1by2(cells[0]) | (part1by2(cells[1]) << np.uint32(1)) | (part1by2(cells[2]) << np.uint32(2))


def unorm(v, bits):
    t = (1 << bits) - 1
    with np.errstate(all="ignore"):
        x = np.floor(np.asarray(v, F) * F(t) + F(0.5))
        return np.where(x > 0, np.minimum(x, F(t)), 0).astype(np.uint32)


def nrm(v, lo, hi):
    with np.errstate(all="ignore"):
        d = (hi - lo).astype(F)
        return np.where(d < F(0.00001), F(0), (v - lo) / d).astype(F)


def pack_11_10_11(v, lo, hi):
    n = nrm(v, lo, hi)
    return (unorm(n[:, 0], 11) << np.uint32(21)) | (unorm(n[:, 1], 10) << np.uint32(11)) | unorm(n[:, 2], 11)


def pack_rotation(q):
    with np.errstate(all="ignore"):
        n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        a = (q / np.sqrt(n2)[:, None]).astype(F)
    L = np.argmax(np.abs(a), axis=1)                     # the first of equal maxima
    aL = a[np.arange(len(a)), L]
    a = np.where((aL < 0)[:, None], -a, a)
    comp = unorm(a * F(0.70710678) + F(0.5), 10)
    word = L.astype(np.uint32)
    for i in range(4):
        word = np.where(L != i, (word << np.uint32(10)) | comp[:, i], word).astype(np.uint32)
    return word


def sh_bytes(plane, degree):
    K = (degree + 1) ** 2 - 1
    cols = [3 + 15 * c + i - 1 for c in range(3) for i in range(1, K + 1)]
    with np.errstate(all="ignore"):
        x = np.trunc((plane[:, cols] / F(8.0) + F(0.5)) * F(256.0))
        return np.where(x > 0, np.minimum(x, F(255)), 0).astype(np.uint8)


def header(C, N, K):
    h = ["ply", "format binary_little_endian 1.0", f"element chunk {C}"] + [f"property float {p}" for p in CHUNK_PROPS]
    h += [f"element vertex {N}"] + [f"property uint packed_{p}" for p in ("position", "rotation", "scale", "color")]
    if K:
        h += [f"element sh {N}"] + [f"property uchar f_rest_{i}" for i in range(3 * K)]
    return ("\n".join(h + ["end_header"]) + "\n").encode()


def encode(records, sm, sh=None, degree=0):
    """-> (the file's bytes, {"rows", "chunks", "skipped"}, the permutation)"""
    rec = np.ascontiguousarray(records, F).reshape(-1, 24)
    sm = F(sm)
    ok = valid_mask(rec)
    src = np.nonzero(ok)[0]
    N = len(src)
    C = (N + 255) // 256
    K = (degree + 1) ** 2 - 1 if sh is not None else 0
    counts = {"rows": N, "chunks": C, "skipped": len(rec) - N}
    if N == 0:
        return header(0, 0, K), counts, src
    p = rec[src][:, 0:3]
    bmin, bmax = omin(p), omax(p)
    perm = src[np.argsort(keys_of(p, bmin, bmax), kind="stable")]
    r = rec[perm]
    with np.errstate(all="ignore"):
        l = logf(r[:, 8:11] * sm)
        ls = np.where(l < F(-20), F(-20), l)
        ls = np.where(ls > F(20), F(20), ls).astype(F)
        col = (sh[perm][:, 0:3].astype(F) * F(0.28209479177387814) + F(0.5)).astype(F) if sh is not None else r[:, 4:7]
    table = np.zeros((C, 18), F)
    rows = np.zeros((N, 4), np.uint32)
    for c in range(C):
        s = slice(256 * c, min(256 * c + 256, N))
        t = table[c]
        for g, v in enumerate((r[s, 0:3], ls[s], col[s])):
            t[6 * g:6 * g + 3], t[6 * g + 3:6 * g + 6] = omin(v), omax(v)
        rows[s, 0] = pack_11_10_11(r[s, 0:3], t[0:3], t[3:6])
        rows[s, 1] = pack_rotation(r[s, ROT])
        rows[s, 2] = pack_11_10_11(ls[s], t[6:9], t[9:12])
        n = nrm(col[s], t[12:15], t[15:18])
        rows[s, 3] = (unorm(n[:, 0], 8) << np.uint32(24)) | (unorm(n[:, 1], 8) << np.uint32(16)) | (unorm(n[:, 2], 8) << np.uint32(8)) | unorm(r[s, 7], 8)
    body = table.tobytes() + rows.tobytes()
    if K:
        body += sh_bytes(np.ascontiguousarray(sh, F)[perm], degree).tobytes()
    return header(C, N, K) + body, counts, perm


def parse(data):
    """a compact file's bytes -> (header text, table (C, 18) f32, rows (N, 4) u32, sh (N, 3K) u8)"""
    head, body = data.split(b"end_header\n", 1)
    head = head.decode() + "end_header\n"
    lines = head.split("\n")
    C = int([ln for ln in lines if ln.startswith("element chunk")][0].split()[2])
    N = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    k3 = sum(ln.startswith("property uchar f_rest_") for ln in lines)
    table = np.frombuffer(body, F, C * 18).reshape(C, 18)
    rows = np.frombuffer(body, np.uint32, N * 4, C * 72).reshape(N, 4)
    sh = np.frombuffer(body, np.uint8, N * k3, C * 72 + N * 16).reshape(N, k3)
    assert len(body) == C * 72 + N * 16 + N * k3
    return head, table, rows, sh


def decode(data):
    """-> position (N, 3), log-scale (N, 3), colour (N, 3), alpha (N,), quaternion (N, 4) as float64, and the table row of every vertex"""
    _, table, rows, _ = parse(data)
    N = len(rows)
    t = table[np.arange(N) // 256].astype(np.float64)

    def un(word, lo, hi):
        x = np.stack([(word >> 21) / 2047.0, ((word >> 11) & 1023) / 1023.0, (word & 2047) / 2047.0], 1)
        return lo + x * (hi - lo)
    pos = un(rows[:, 0], t[:, 0:3], t[:, 3:6])
    ls = un(rows[:, 2], t[:, 6:9], t[:, 9:12])
    cw = rows[:, 3]
    c01 = np.stack([(cw >> 24) & 255, (cw >> 16) & 255, (cw >> 8) & 255], 1) / 255.0
    col = t[:, 12:15] + c01 * (t[:, 15:18] - t[:, 12:15])
    alpha = (cw & 255) / 255.0
    rw = rows[:, 1]
    L = rw >> 30
    v = (np.stack([(rw >> 20) & 1023, (rw >> 10) & 1023, rw & 1023], 1) / 1023.0 - 0.5) / 0.70710678
    m = np.sqrt(np.maximum(0.0, 1.0 - (v * v).sum(1)))
    q = np.zeros((N, 4))
    for i in range(N):
        q[i] = np.insert(v[i], L[i], m[i])
    return pos, ls, col, alpha, q, t


# ---- record sets ----
def make_records(n, seed=0, spread=1.0):
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 24), F)
    rec[:, 0:3] = rng.normal(0, spread, (n, 3))
    rec[:, 3] = 1
    rec[:, 4:8] = rng.random((n, 4))
    rec[:, 8:10] = np.exp(rng.normal(-1, 1, (n, 2)))
    rec[:, 10] = 1e-7
    rec[:, 11] = 1
    rec[:, 12:15] = rng.normal(0, 1, (n, 3))
    q = rng.normal(0, 1, (n, 4))
    rec[:, ROT] = q / np.linalg.norm(q, axis=1, keepdims=True)
    rec[:, 20:22] = rng.random((n, 2))
    return rec


def hostile(rec):
    """rec with 17 hostile records spliced in: NaN / Inf in every field class, a negative scale, a zero quaternion, an overflowing n2"""
    out = [rec[: len(rec) // 2]]
    base = make_records(17, 99)
    bad = [(0, np.nan), (2, np.inf), (1, -np.inf), (4, np.nan), (7, np.inf), (8, np.nan), (10, np.inf), (9, -1e-3), (16, np.nan), (19, -np.inf)]
    for k, (col, val) in enumerate(bad):
        base[k, col] = val
    base[10, ROT] = 0
    base[11, ROT] = (0, -0.0, 0, -0.0)
    base[12, ROT] = (3e19, 3e19, 0, 0)          # n2 overflows
    base[13, 8] = -0.5
    # 14, 15, 16 stay valid: NaN in the fields the format never reads, a -0 scale
    base[14, 12:16] = np.nan
    base[15, 20:24] = np.inf
    base[16, 8] = -0.0
    out += [base, rec[len(rec) // 2:]]
    return np.concatenate(out)


def cases():
    """name -> (records, scale multiplier)"""
    c = {}
    for n in (0, 1, 255, 256, 257, 785):
        c[f"n{n}"] = (make_records(n, n), 0.65 / 64)
    same = make_records(300, 1)
    same[:, 0:3] = (0.25, -1.5, 3.0)
    c["zero_extent"] = (same, 0.01)
    dup = make_records(900, 2)
    dup[:, 0:3] = np.array([(0, 0, 0), (1, 2, 3), (-1, 0.5, 0.25)], F)[np.arange(900) % 3]
    c["duplicates"] = (dup, 0.01)
    tiny = make_records(512, 3)
    tiny[:256, 0:3] = F(5.0) + np.arange(256, dtype=F)[:, None] * F(1e-8)      # sorts into one chunk: range below 1e-5
    tiny[:256, 0] = F(5.0) + (np.arange(256) % 5).astype(F) * F(4.7e-7)
    tiny[256:, 0:3] += 100
    tiny[:256, 4:7] = F(0.5) + (np.arange(256) % 3).astype(F)[:, None] * F(1e-6)
    c["tiny_range"] = (tiny, 0.01)
    sc = make_records(300, 4)
    sc[::7, 8] = 1e12
    sc[::5, 9] = 0.0
    sc[::11, 8] = 1e-30
    c["scales"] = (sc, 0.65 / 1024)
    q = make_records(300, 5)
    q[0, ROT] = (0.5, -0.5, 0.5, 0.5)
    q[1, ROT] = (-0.5, 0.5, 0.5, 0.5)
    q[2, ROT] = (0.1, -0.9, 0.1, 0.1)
    q[3, ROT] = (-0.0, 1.0, -0.0, 0.0)
    q[4, ROT] = (0.0, 0.0, 0.0, -2.0)
    q[5, ROT] = (3.0, 4.0, 0.0, 12.0)
    q[6, ROT] = (1e-20, 1e-20, 0, 0)
    q[7:40, ROT] *= np.linspace(0.1, 30, 33, dtype=F)[:, None]
    c["quaternions"] = (q, 0.01)
    st = make_records(256, 6)
    st[:, 0] = np.arange(256, dtype=F) / F(2047.0) * F(0.5) + (np.arange(256) % 2).astype(F) * F(0.5 / 2047 / 2)      # k + 0.5 steps of an 11-bit grid
    st[0, 0], st[255, 0] = 0.0, 1.0
    st[:, 7] = (np.arange(256, dtype=F) + F(0.5)) / F(255.0)
    st[:, 4] = np.arange(256, dtype=F) / F(255.0)
    st[:, 5] = (np.arange(256, dtype=F) + F(0.5)) / F(255.0) * (np.arange(256) < 255)
    c["unorm_steps"] = (st, 0.01)
    c["hostile"] = (hostile(make_records(600, 7)), 0.65 / 64)
    allbad = make_records(5, 8)
    allbad[:, 0] = np.nan
    c["all_invalid"] = (allbad, 0.01)
    return c


def sh_plane(n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    sh = rng.normal(0, 1.5, (n, 48)).astype(F)
    edge = np.array([4.0, -4.0, 3.96875, -3.96875, 5.0, -5.0, 3.9999998, -4.0000005, 0.0, -0.0, 100.0, -100.0, 0.03125, -0.03125], F)
    m = min(edge.size, sh.size // 3)
    sh.ravel()[: m * 3:3] = edge[:m]
    return sh
