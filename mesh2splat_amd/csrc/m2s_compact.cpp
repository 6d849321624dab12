// m2s_compact.cpp — the compact .ply export of the context's records (include/m2s.h "compact export"): host side of m2s_compact.hip.
// Everything up to the file's bytes is computed on the device; the host reads {N, skipped} back once, copies the chunk table, the
// rows and the SH bytes through the pinned chunks of m2s_export_ply and writes them behind the header.  The host writer of the same
// format (m2s_write_ply_compact, the yardstick) and the decoder are m2s_compact_host.cpp.
#include "m2s_compactmath.h"
#include "m2s_ctx.h"
#include "m2s_host.h"
#include "m2s_ply.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <string>

using namespace m2s;
using namespace m2s_host;

namespace {

// `bytes` of device memory into the file through the two pinned chunks: chunk k + 1 is on the bus while chunk k is written
m2s_status stream_to_file(m2s_ctx* c, const uint8_t* src, uint64_t bytes, FILE* f, bool* io_ok) {
    const uint64_t chunk = m2s_ply::kChunkRows * sizeof(m2s_gaussian);
    const uint64_t n_chunks = (bytes + chunk - 1) / chunk;
    auto size_of = [&](uint64_t k) { return (size_t)std::min<uint64_t>(chunk, bytes - k * chunk); };
    if (n_chunks) HIPCHK(c, hipMemcpyAsync(c->h_export[0], src, size_of(0), hipMemcpyDeviceToHost, c->stream));
    for (uint64_t k = 0; k < n_chunks; ++k) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (k + 1 < n_chunks) HIPCHK(c, hipMemcpyAsync(c->h_export[(k + 1) & 1], src + (k + 1) * chunk, size_of(k + 1), hipMemcpyDeviceToHost, c->stream));
        *io_ok = *io_ok && std::fwrite(static_cast<m2s_gaussian*>(c->h_export[k & 1]), 1, size_of(k), f) == size_of(k);
    }
    return M2S_OK;
}

}  // namespace

extern "C" {

m2s_status m2s_export_ply_compact(m2s_ctx* c, const char* path, float gaussian_std, int use_baked_sh, uint64_t out_counts[3]) {
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = 0;
    if (!c || !path) return M2S_ERR_INVALID;
    if (!std::isfinite(gaussian_std) || !(gaussian_std > 0.0f)) return fail(c, M2S_ERR_INVALID, "gaussian_std must be finite and > 0");
    uint64_t n64 = 0;
    M2S_TRY(need_records(c, &n64));
    if (use_baked_sh && (!c->sh_tag.is_set() || c->sh_tag.n != n64)) return fail(c, M2S_ERR_STATE, "no baked coefficients for this many records (run m2s_bake_light on them)");
    const uint32_t n = (uint32_t)n64;
    const uint32_t K = use_baked_sh ? m2s_compact::sh_coefficients(c->sh_degree) : 0u;
    // SceneManager.cpp:668, as m2s_export_ply; records without a resolutionTarget (uploaded ones) are taken as converted at R = 1
    const float sm = c->last_R ? gaussian_std / static_cast<float>(c->last_R) : gaussian_std;
    HIPCHK(c, hipSetDevice(c->device));
    ClockOf<CompactMark>& clock = c->compact_clock;
    M2S_TRY(clock.begin(c->err, true));            // (measured whatever m2s_set_profiling says)
    M2S_TRY(c->h_compact.ensure(c->err, 2 * sizeof(uint32_t)));
    for (int k = 0; k < 2; ++k) M2S_TRY(c->h_export[k].ensure(c->err, m2s_ply::kChunkRows * sizeof(m2s_gaussian)));
    for (float& v : c->last_compact_stage_ms) v = 0.0f;
    uint32_t N = 0, skipped = 0;
    const uint32_t* perm = nullptr;
    if (n) {
        const uint32_t n_waves = compact_waves(n);
        M2S_TRY(c->d_compact_u32.reserve(c->err, n, 4 * sizeof(uint32_t)));
        M2S_TRY(c->d_compact_waves.reserve(c->err, (uint64_t)n_waves + 1, 8 * sizeof(uint32_t)));
        const size_t temp_bytes = compact_sort_temp_bytes(n);
        M2S_TRY(c->d_compact_temp.reserve(c->err, temp_bytes, 1));
        const uint64_t cap = c->d_compact_u32.cap();
        uint32_t* const u = c->d_compact_u32.get();
        uint32_t* const head = c->d_compact_waves.get() + (size_t)n_waves * 8;
        const float4* plane = m2s_positions_ready(c) ? c->d_pos_plane.get() : nullptr;
        HIPCHK(c, compact_keys_and_sort((const float4*)c->last_records, plane, n, c->d_compact_waves, head, u, u + cap, u + 2 * cap, u + 3 * cap, c->d_compact_temp,
                                        temp_bytes, clock.marks(), c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_compact, head + 6, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        N = static_cast<uint32_t*>(c->h_compact)[0];
        skipped = static_cast<uint32_t*>(c->h_compact)[1];
        if (N > n || skipped != n - N) return fail(c, M2S_ERR_HIP, "the compact export's record count came back inconsistent");
        perm = u + 3 * cap;
    }
    const uint64_t C = ((uint64_t)N + m2s_compact::kChunkRows - 1) / m2s_compact::kChunkRows;
    const uint64_t table_bytes = C * 18 * sizeof(float), row_bytes = (uint64_t)N * 16, sh_bytes = (uint64_t)N * 3 * K;
    const uint64_t rows_at = align_up((size_t)table_bytes, 256), sh_at = rows_at + align_up((size_t)row_bytes, 256);
    const uint64_t sh_room = C * m2s_compact::kChunkRows * 3 * K;                 // whole chunks (m2s_compact.hip)
    if (N) {
        M2S_TRY(c->d_compact_out.reserve(c->err, sh_at + sh_room, 1));
        uint8_t* const o = c->d_compact_out.get();
        HIPCHK(c, clock.mark(CompactMark::Pack, c->stream));
        HIPCHK(c, compact_pack((const float4*)c->last_records, use_baked_sh ? c->d_sh.get() : nullptr, perm, N, sm, K, reinterpret_cast<float*>(o), o + rows_at,
                               K ? o + sh_at : nullptr, c->stream));
        HIPCHK(c, clock.mark(CompactMark::Packed, c->stream));
    }
    const auto t0 = std::chrono::steady_clock::now();
    FILE* f = std::fopen(path, "wb");
    if (!f) { (void)hipStreamSynchronize(c->stream); return fail(c, M2S_ERR_IO, std::string("could not write ") + path); }
    const std::string header = compact_ply_header(C, N, K);
    bool ok = std::fwrite(header.data(), 1, header.size(), f) == header.size();
    m2s_status s = M2S_OK;
    if (N) {
        const uint8_t* const o = c->d_compact_out.get();
        s = stream_to_file(c, o, table_bytes, f, &ok);
        if (s == M2S_OK) s = stream_to_file(c, o + rows_at, row_bytes, f, &ok);
        if (s == M2S_OK && K) s = stream_to_file(c, o + sh_at, sh_bytes, f, &ok);
    }
    ok = (std::fclose(f) == 0) && ok;
    if (s != M2S_OK) { (void)hipStreamSynchronize(c->stream); return s; }
    if (!ok) return fail(c, M2S_ERR_IO, std::string("could not write ") + path);
    c->last_compact_stage_ms[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // (no records: no marks, [0..2] are 0; none of them valid: nothing was packed, [2] is)
    HIPCHK(c, clock.span(CompactMark::Start, CompactMark::Keyed, &c->last_compact_stage_ms[0]));
    HIPCHK(c, clock.span(CompactMark::Keyed, CompactMark::Sorted, &c->last_compact_stage_ms[1]));
    HIPCHK(c, clock.span(CompactMark::Pack, CompactMark::Packed, &c->last_compact_stage_ms[2]));
    if (out_counts) { out_counts[0] = N; out_counts[1] = C; out_counts[2] = skipped; }
    return M2S_OK;
}

m2s_status m2s_last_compact_stage_ms(const m2s_ctx* c, float out_ms[4]) { return get_array(c, &m2s_ctx::last_compact_stage_ms, out_ms); }

}  // extern "C"
