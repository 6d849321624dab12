// m2s_bake.cpp — the point light baked into the spherical harmonics of the standard 3DGS .ply: host side of m2s_bake.hip
// (m2s_bake_light, m2s_sh_shade_records, m2s_export_ply_sh) and the quadrature table both sides of the pin share.
#include "m2s_ctx.h"
#include "m2s_ply.h"
#include "m2s_shbasis.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace m2s;
using namespace m2s_host;

namespace {

constexpr double kPi = 3.141592653589793;

// The n positive-and-negative Gauss-Legendre nodes in z, descending, and their weights: Newton's iteration on P_n from four-digit
// starting values, a FIXED number of steps, nothing but + - * / (IEEE double: the same bits wherever it runs, and in
// mesh2splat_amd/bake.py, which repeats these lines).
void gauss_legendre(int n, double* z, double* w) {
    static const double G4[2] = { 0.8611, 0.3400 };
    static const double G8[4] = { 0.9603, 0.7967, 0.5255, 0.1834 };
    const double* guess = n == 4 ? G4 : G8;
    for (int r = 0; r < n / 2; ++r) {
        double x = guess[r], dp = 0.0;
        for (int it = 0; it < 6; ++it) {
            double p0 = 1.0, p1 = x;
            for (int k = 2; k <= n; ++k) {
                const double pk = (((2.0 * k - 1.0) * x) * p1 - (k - 1.0) * p0) / k;
                p0 = p1;
                p1 = pk;
            }
            dp = (n * (x * p1 - p0)) / (x * x - 1.0);
            if (it == 5) break;                      // (the last pass only evaluates the derivative at the final node)
            x = x - p1 / dp;
        }
        const double wt = 2.0 / ((1.0 - x * x) * (dp * dp));
        z[r] = x; w[r] = wt;
        z[n - 1 - r] = -x; w[n - 1 - r] = wt;
    }
}

// cos / sin of the azimuths 2 pi (j + 0.5) / n_phi from the first quadrant's cosines (decimal literals: no libm in the table)
void azimuths(int n_phi, double* cs, double* sn) {
    static const double Q8[2] = { 0.9238795325112867, 0.3826834323650898 };                                    // cos(pi/8), cos(3 pi/8)
    static const double Q16[4] = { 0.9807852804032304, 0.8314696123025452, 0.5555702330196022, 0.19509032201612825 };   // cos((2k+1) pi/16)
    const double* Q = n_phi == 8 ? Q8 : Q16;
    const int h = n_phi / 4;
    for (int j = 0; j < n_phi; ++j) {
        const int q = j / h, k = j % h;
        const double c = Q[k], s = Q[h - 1 - k];
        cs[j] = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
        sn[j] = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
    }
}

bool table_sizes_ok(uint32_t nt, uint32_t np) { return (nt == 4 || nt == 8) && (np == 8 || np == 16); }

// rows of kBakeTableRow floats, row t * n_phi + j: d.xyz, w, w * B_0..15(d) — double, rounded once
void build_table(uint32_t nt, uint32_t np, float* out) {
    double z[8], wz[8], cs[16], sn[16];
    gauss_legendre((int)nt, z, wz);
    azimuths((int)np, cs, sn);
    const double wphi = (2.0 * kPi) / (double)np;
    for (uint32_t t = 0; t < nt; ++t) {
        const double st = std::sqrt(1.0 - z[t] * z[t]);
        const double w = wz[t] * wphi;
        for (uint32_t j = 0; j < np; ++j) {
            const double x = st * cs[j], y = st * sn[j];
            double B[16];
            sh_basis<double>(x, y, z[t], B);
            float* row = out + (size_t)(t * np + j) * kBakeTableRow;
            row[0] = (float)x; row[1] = (float)y; row[2] = (float)z[t]; row[3] = (float)w;
            for (int i = 0; i < 16; ++i) row[4 + i] = (float)(w * B[i]);
        }
    }
}

void model_matrices(const float model_to_world[16], float M[16], float MinvT[16]) {
    m2s_prepass_params pp;
    std::memset(&pp, 0, sizeof(pp));
    std::memcpy(pp.model_to_world, model_to_world, sizeof(pp.model_to_world));
    pp.resolution[0] = pp.resolution[1] = 1;
    pp.resolution_target = 1;
    PrepassK k;
    prepass_prepare(pp, 0, &k);                      // the viewer prepass's own transpose(inverse(M)): the normal is ITS normalWs
    std::memcpy(M, k.M, sizeof(k.M));
    if (MinvT) std::memcpy(MinvT, k.MinvT, sizeof(k.MinvT));
}

}  // namespace

extern "C" {

m2s_status m2s_bake_directions(uint32_t n_theta, uint32_t n_phi, float* out, uint64_t capacity_floats) {
    if (!n_theta) n_theta = 8;
    if (!n_phi) n_phi = 16;
    if (!out || !table_sizes_ok(n_theta, n_phi) || capacity_floats < (uint64_t)n_theta * n_phi * kBakeTableRow) return M2S_ERR_INVALID;
    build_table(n_theta, n_phi, out);
    return M2S_OK;
}

m2s_status m2s_bake_light(m2s_ctx* c, const m2s_bake_params* bp, const m2s_light_params* lp, const void* d_records, uint64_t n) {
    if (!c || !bp || !lp) return M2S_ERR_INVALID;
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    const uint32_t nt = bp->n_theta ? bp->n_theta : 8, np = bp->n_phi ? bp->n_phi : 16;
    if (bp->degree > 3) return fail(c, M2S_ERR_INVALID, "degree above 3");
    if (!table_sizes_ok(nt, np)) return fail(c, M2S_ERR_INVALID, "n_theta must be 4 or 8 and n_phi 8 or 16 (0: the default, 8 x 16)");
    if (bp->reserved != 0) return fail(c, M2S_ERR_INVALID, "reserved != 0");
    if (m2s_status s = pick_records(c, d_records, n)) return s;
    if (bp->use_shadows && !c->shadow_S) return fail(c, M2S_ERR_STATE, "no shadow cube exists (run m2s_shadow or m2s_upload_shadow_cubemap)");
    HIPCHK(c, hipSetDevice(c->device));
    M2S_TRY(c->bake_clock.begin(c->err, c->profiling));
    c->sh_tag.clear();
    c->bake_has_counts = false;
    M2S_TRY(c->d_sh.reserve(c->err, n, 48 * sizeof(float)));
    const bool counts = bp->want_shadow_counts != 0;
    if (counts) M2S_TRY(c->d_bake_counts.reserve(c->err, n, 1));
    if (c->bake_table_nt != nt || c->bake_table_np != np) {
        c->bake_table_nt = c->bake_table_np = 0;
        M2S_TRY(c->d_bake_table.reserve(c->err, 128 * kBakeTableRow, sizeof(float)));
        float h_table[128 * kBakeTableRow];
        build_table(nt, np, h_table);
        HIPCHK(c, hipMemcpy(c->d_bake_table, h_table, (size_t)nt * np * kBakeTableRow * sizeof(float), hipMemcpyHostToDevice));
        c->bake_table_nt = nt; c->bake_table_np = np;
    }
    BakeK k;
    model_matrices(bp->model_to_world, k.M, k.MinvT);
    for (int i = 0; i < 3; ++i) { k.light[i] = lp->light_position[i]; k.color[i] = lp->light_color[i]; }
    k.intensity = lp->light_intensity;
    k.far_plane = lp->near_far[1];
    k.S = bp->use_shadows ? c->shadow_S : 0;
    k.n_dirs = nt * np;
    k.n_coef = (bp->degree + 1) * (bp->degree + 1);
    k.use_shadows = bp->use_shadows ? 1u : 0u;
    k.viewer_metallic = bp->viewer_metallic ? 1u : 0u;
    HIPCHK(c, c->bake_clock.mark(SpanMark::Begin, c->stream));
    HIPCHK(c, launch_bake_sh(k, (const float4*)d_records, (uint32_t)n, c->d_bake_table, k.use_shadows ? c->d_shadow_cube.get() : nullptr, c->d_sh,
                             counts ? c->d_bake_counts.get() : nullptr, c->stream));
    HIPCHK(c, c->bake_clock.mark(SpanMark::End, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->bake_clock.on()) HIPCHK(c, c->bake_clock.span(SpanMark::Begin, SpanMark::End, &c->last_bake_ms));
    if (d_records == c->last_records) c->sh_tag.set(*c, n);
    else c->sh_tag.set_foreign(d_records, n);
    c->bake_has_counts = counts;
    c->sh_degree = bp->degree;
    return M2S_OK;
}

const void* m2s_device_sh(const m2s_ctx* c) { return c && c->sh_tag.is_set() ? c->d_sh.get() : nullptr; }

m2s_status m2s_download_sh(m2s_ctx* c, float* dst, uint64_t capacity_records) {
    if (!c) return M2S_ERR_INVALID;
    if (!c->sh_tag.is_set()) return fail(c, M2S_ERR_STATE, "no m2s_bake_light has run");
    if (!c->sh_tag.n) return M2S_OK;
    if (!dst) return fail(c, M2S_ERR_INVALID, "dst is NULL");
    if (capacity_records < c->sh_tag.n) return fail(c, M2S_ERR_CAPACITY, "destination smaller than the plane");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_sh, c->sh_tag.n * 48 * sizeof(float), hipMemcpyDeviceToHost));
    return M2S_OK;
}

m2s_status m2s_upload_sh(m2s_ctx* c, const float* host, uint64_t n, uint32_t degree) {
    if (!c) return M2S_ERR_INVALID;
    if (degree > 3) return fail(c, M2S_ERR_INVALID, "degree above 3");
    M2S_TRY(have_records(c));
    if (n != c->last_stored) return fail(c, M2S_ERR_INVALID, "the number of rows is not the number of stored records");
    if (n && !host) return fail(c, M2S_ERR_INVALID, "host is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    c->sh_tag.clear();
    c->bake_has_counts = false;
    M2S_TRY(c->d_sh.reserve(c->err, std::max<uint64_t>(n, 1), 48 * sizeof(float)));
    if (n) HIPCHK(c, hipMemcpy(c->d_sh, host, n * 48 * sizeof(float), hipMemcpyHostToDevice));
    c->sh_tag.set(*c, n);
    c->sh_degree = degree;
    return M2S_OK;
}

m2s_status m2s_sh_plane_info(const m2s_ctx* c, uint64_t* rows, uint32_t* degree) {
    if (rows) *rows = 0;
    if (degree) *degree = 0;
    if (!c) return M2S_ERR_INVALID;
    if (!c->sh_tag.is_set()) return M2S_ERR_STATE;
    if (rows) *rows = c->sh_tag.n;
    if (degree) *degree = c->sh_degree;
    return M2S_OK;
}

m2s_status m2s_download_bake_shadow_counts(m2s_ctx* c, uint8_t* dst, uint64_t capacity_bytes) {
    if (!c) return M2S_ERR_INVALID;
    if (!c->sh_tag.is_set() || !c->bake_has_counts) return fail(c, M2S_ERR_STATE, "the last m2s_bake_light kept no shadow counts (want_shadow_counts)");
    if (!c->sh_tag.n) return M2S_OK;
    if (!dst) return fail(c, M2S_ERR_INVALID, "dst is NULL");
    if (capacity_bytes < c->sh_tag.n) return fail(c, M2S_ERR_CAPACITY, "destination smaller than the plane");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_bake_counts, c->sh_tag.n, hipMemcpyDeviceToHost));
    return M2S_OK;
}

float m2s_last_bake_ms(const m2s_ctx* c) { return c ? c->last_bake_ms : 0.0f; }

m2s_status m2s_sh_shade_records(m2s_ctx* c, const float model_to_world[16], const float camera_position[3], const void* d_records, uint64_t n,
                                void* d_dst) {
    if (!c || !model_to_world || !camera_position) return M2S_ERR_INVALID;
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    if (m2s_status s = pick_records(c, d_records, n)) return s;
    if (!c->sh_tag.is_set() || c->sh_tag.n != n) return fail(c, M2S_ERR_STATE, "no baked coefficients for this many records (run m2s_bake_light on them)");
    if (n && !d_dst) return fail(c, M2S_ERR_INVALID, "d_dst is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    ShadeK k;
    model_matrices(model_to_world, k.M, nullptr);
    for (int i = 0; i < 3; ++i) k.cam[i] = camera_position[i];
    HIPCHK(c, launch_sh_shade(k, (const float4*)d_records, c->d_sh, (uint32_t)n, (float4*)d_dst, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return M2S_OK;
}

m2s_status m2s_write_ply_sh(const char* path, const m2s_gaussian* records, const float* sh, uint64_t n, float scale_multiplier) {
    if (!path || (n && (!records || !sh))) return M2S_ERR_INVALID;
    m2s_ply::Writer w;
    m2s_status s = w.open(path, n, 0, scale_multiplier);
    if (s == M2S_OK) s = w.append(records, (size_t)n, sh);
    const m2s_status cs = w.close();
    return s != M2S_OK ? s : cs;
}

// The context's records and its baked plane, chunk by chunk through two host buffers into the format-0 writer (append returns once it
// has read them).
m2s_status m2s_export_ply_sh(m2s_ctx* c, const char* path, float gaussian_std) {
    if (!c || !path) return M2S_ERR_INVALID;
    if (!c->last_R) return fail(c, M2S_ERR_STATE, "no conversion has run (uploaded records carry no resolutionTarget: use m2s_write_ply_sh)");
    if (c->records_stale) return fail(c, M2S_ERR_STATE, kStaleMsg);
    if (!c->sh_tag.is_set()) return fail(c, M2S_ERR_STATE, "no m2s_bake_light has run");
    if (c->sh_tag.n != c->last_stored) return fail(c, M2S_ERR_STATE, "the baked plane holds another number of records than the conversion stored");
    HIPCHK(c, hipSetDevice(c->device));
    const float scale_multiplier = gaussian_std / static_cast<float>(c->last_R);      // SceneManager.cpp:668, as m2s_export_ply
    const uint64_t n = c->last_stored;
    const size_t chunk = m2s_ply::kChunkRows;
    std::vector<m2s_gaussian> rec;
    std::vector<float> sh;
    try { rec.resize((size_t)std::min<uint64_t>(n, chunk)); sh.resize(rec.size() * 48); } catch (...) { return fail(c, M2S_ERR_OOM, "host memory"); }
    m2s_ply::Writer w;
    m2s_status s = w.open(path, n, 0, scale_multiplier);
    if (s != M2S_OK) { c->err = std::string("could not write ") + path; return s; }
    for (uint64_t r0 = 0; r0 < n && s == M2S_OK; r0 += chunk) {
        const size_t rows = (size_t)std::min<uint64_t>(chunk, n - r0);
        HIPCHK(c, hipMemcpy(rec.data(), static_cast<const char*>(c->last_records) + r0 * sizeof(m2s_gaussian), rows * sizeof(m2s_gaussian),
                            hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(sh.data(), c->d_sh + r0 * 48, rows * 48 * sizeof(float), hipMemcpyDeviceToHost));
        s = w.append(rec.data(), rows, sh.data());
    }
    const m2s_status cs = w.close();
    if (s == M2S_OK) s = cs;
    if (s != M2S_OK) c->err = std::string("could not write ") + path;
    return s;
}

}  // extern "C"
