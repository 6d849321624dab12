// m2s_compact_host.cpp — the compact .ply (include/m2s.h "compact export") on the host: the writer m2s_write_ply_compact, which is the
// pin in plain C++ and the yardstick of the device path (m2s_compact.cpp / m2s_compact.hip), and the decoder behind m2s_read_ply.
// No HIP: a plain host compiler builds this file for tools/fuzz_host.sh.
#include "m2s_compactmath.h"
#include "m2s_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace mc = m2s_compact;

namespace m2s_host {

static const char* const kChunkProps[18] = { "min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z",
                                             "max_scale_x", "max_scale_y", "max_scale_z", "min_r", "min_g", "min_b", "max_r", "max_g", "max_b" };
static const char* const kVertexProps[4] = { "packed_position", "packed_rotation", "packed_scale", "packed_color" };

std::string compact_ply_header(uint64_t n_chunks, uint64_t n_rows, uint32_t sh_k) {
    std::string h = "ply\nformat binary_little_endian 1.0\nelement chunk " + std::to_string(n_chunks) + "\n";
    for (const char* p : kChunkProps) h += std::string("property float ") + p + "\n";
    h += "element vertex " + std::to_string(n_rows) + "\n";
    for (const char* p : kVertexProps) h += std::string("property uint ") + p + "\n";
    if (sh_k) {
        h += "element sh " + std::to_string(n_rows) + "\n";
        for (uint32_t i = 0; i < 3 * sh_k; ++i) h += "property uchar f_rest_" + std::to_string(i) + "\n";
    }
    return h + "end_header\n";
}

namespace {

struct Element {
    std::string name;
    uint64_t count = 0;
    uint64_t row = 0;                                           // bytes
    std::vector<std::pair<std::string, std::pair<uint64_t, int>>> props;   // name -> (offset, type: 'f' float, 'u' uint, 'b' uchar, 'o' other)
    long find(const char* n, int type) const {
        for (const auto& p : props) if (p.first == n) return p.second.second == type ? (long)p.second.first : -1;
        return -1;
    }
};

inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

}  // namespace

int read_compact_ply(const char* path, m2s_gaussian** out, uint64_t* out_n, std::string& err, m2s_status* st) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 0;                                            // (the caller reports what it cannot open)
    m2s_gaussian* rec = nullptr;
    auto refuse = [&](m2s_status s, const std::string& m) { std::fclose(f); std::free(rec); err = m; *st = s; return -1; };
    auto other = [&]() { std::fclose(f); return 0; };
    try {
        char line[512];
        if (!std::fgets(line, sizeof line, f) || std::strncmp(line, "ply", 3) != 0) return other();
        std::vector<Element> els;
        bool little = false, got_end = false;
        for (int lines = 0; lines < 4096 && std::fgets(line, sizeof line, f); ++lines) {
            char a[64] = "", b[64] = "", c[64] = "";
            const int k = std::sscanf(line, "%63s %63s %63s", a, b, c);
            if (k >= 1 && !std::strcmp(a, "end_header")) { got_end = true; break; }
            if (k >= 2 && !std::strcmp(a, "format")) little = !std::strcmp(b, "binary_little_endian");
            else if (k >= 3 && !std::strcmp(a, "element")) {
                if (els.size() >= 16) return other();
                Element e;
                e.name = b;
                char* end = nullptr;
                e.count = std::strtoull(c, &end, 10);
                if (end == c || c[0] == '-') e.count = UINT64_MAX;   // not a count: refused below if the file turns out to be compact
                els.push_back(e);
            } else if (k >= 3 && !std::strcmp(a, "property") && !els.empty()) {
                Element& e = els.back();
                int sz = 0, type = 'o';
                auto is = [&](const char* x, const char* y) { return !std::strcmp(b, x) || !std::strcmp(b, y); };
                if (is("float", "float32")) { sz = 4; type = 'f'; }
                else if (is("uint", "uint32")) { sz = 4; type = 'u'; }
                else if (is("uchar", "uint8")) { sz = 1; type = 'b'; }
                else if (is("int", "int32")) sz = 4;
                else if (is("double", "float64")) sz = 8;
                else if (is("short", "int16") || is("ushort", "uint16")) sz = 2;
                else if (is("char", "int8")) sz = 1;
                else sz = -1;                                    // a list or an unknown type: the row size is unknown
                if (e.props.size() >= 4096) return other();
                e.props.push_back({ c, { e.row, sz < 0 ? 'l' : type } });
                if (sz > 0) e.row += (uint64_t)sz;
            }
        }
        const Element *chunk = nullptr, *vertex = nullptr;
        for (const Element& e : els) { if (e.name == "chunk" && !chunk) chunk = &e; if (e.name == "vertex" && !vertex) vertex = &e; }
        if (!got_end || !chunk || !vertex) return other();
        long vo[4];
        for (int i = 0; i < 4; ++i) if ((vo[i] = vertex->find(kVertexProps[i], 'u')) < 0) return other();
        // from here on the file claims to be compact: what does not fit is refused, not handed to the other parser
        if (!little) return refuse(M2S_ERR_INVALID, "compact PLY: only binary_little_endian bodies are supported");
        long co[18];
        for (int i = 0; i < 18; ++i)
            if ((co[i] = chunk->find(kChunkProps[i], 'f')) < 0) return refuse(M2S_ERR_INVALID, std::string("compact PLY: missing float property ") + kChunkProps[i]);
        const long body0 = std::ftell(f);
        if (body0 < 0 || std::fseek(f, 0, SEEK_END) != 0) return refuse(M2S_ERR_IO, "cannot seek in PLY file");
        const long fsize = std::ftell(f);
        if (fsize < body0) return refuse(M2S_ERR_IO, "cannot seek in PLY file");
        uint64_t left = (uint64_t)(fsize - body0), chunk_at = 0, vertex_at = 0, at = 0;
        for (const Element& e : els) {                           // every element's bytes must be in the file, the ignored ones included
            for (const auto& p : e.props) if (p.second.second == 'l') return refuse(M2S_ERR_INVALID, "compact PLY: list or unknown property type in element " + e.name);
            if (e.count == UINT64_MAX) return refuse(M2S_ERR_INVALID, "compact PLY: element " + e.name + " has no valid count");
            if (e.count && (e.row == 0 || e.count > left / e.row)) return refuse(M2S_ERR_IO, "truncated PLY body (element " + e.name + ")");
            if (&e == chunk) chunk_at = at;
            if (&e == vertex) vertex_at = at;
            at += e.count * e.row;
            left -= e.count * e.row;
        }
        const uint64_t n = vertex->count, nc = chunk->count;
        if (nc < n / mc::kChunkRows + (n % mc::kChunkRows ? 1 : 0)) return refuse(M2S_ERR_INVALID, "compact PLY: fewer chunks than ceil(vertices / 256)");
        if (n > SIZE_MAX / sizeof(m2s_gaussian)) return refuse(M2S_ERR_INVALID, "PLY vertex count too large");
        rec = n ? (m2s_gaussian*)std::malloc((size_t)n * sizeof(m2s_gaussian)) : nullptr;
        if (n && !rec) return refuse(M2S_ERR_OOM, "host allocation failed");
        const size_t crow = (size_t)chunk->row, vrow = (size_t)vertex->row;
        std::vector<uint8_t> cbuf(crow), vbuf(vrow * mc::kChunkRows);
        for (uint64_t c0 = 0; c0 * mc::kChunkRows < n; ++c0) {
            if (fseeko(f, (off_t)((uint64_t)body0 + chunk_at + c0 * crow), SEEK_SET) != 0 || std::fread(cbuf.data(), 1, crow, f) != crow)
                return refuse(M2S_ERR_IO, "truncated PLY body");
            float t[18];
            for (int i = 0; i < 18; ++i) t[i] = mc::u2f(rd32(cbuf.data() + co[i]));
            const size_t rows = (size_t)std::min<uint64_t>(mc::kChunkRows, n - c0 * mc::kChunkRows);
            if (fseeko(f, (off_t)((uint64_t)body0 + vertex_at + c0 * mc::kChunkRows * vrow), SEEK_SET) != 0 || std::fread(vbuf.data(), vrow, rows, f) != rows)
                return refuse(M2S_ERR_IO, "truncated PLY body");
            for (size_t r = 0; r < rows; ++r) {
                const uint8_t* v = vbuf.data() + r * vrow;
                const uint32_t pp = rd32(v + vo[0]), pr = rd32(v + vo[1]), ps = rd32(v + vo[2]), pc = rd32(v + vo[3]);
                m2s_gaussian& g = rec[c0 * mc::kChunkRows + r];
                g.position[0] = mc::lerp_unorm(pp >> 21, 2047u, t[0], t[3]);
                g.position[1] = mc::lerp_unorm((pp >> 11) & 1023u, 1023u, t[1], t[4]);
                g.position[2] = mc::lerp_unorm(pp & 2047u, 2047u, t[2], t[5]);
                g.position[3] = 1.0f;
                g.scale[0] = std::exp(mc::lerp_unorm(ps >> 21, 2047u, t[6], t[9]));
                g.scale[1] = std::exp(mc::lerp_unorm((ps >> 11) & 1023u, 1023u, t[7], t[10]));
                g.scale[2] = std::exp(mc::lerp_unorm(ps & 2047u, 2047u, t[8], t[11]));
                g.scale[3] = 1.0f;
                g.color[0] = mc::lerp_unorm(pc >> 24, 255u, t[12], t[15]);
                g.color[1] = mc::lerp_unorm((pc >> 16) & 255u, 255u, t[13], t[16]);
                g.color[2] = mc::lerp_unorm((pc >> 8) & 255u, 255u, t[14], t[17]);
                g.color[3] = (float)(pc & 255u) / 255.0f;
                mc::unpack_rotation(pr, g.rotation);
                g.normal[0] = g.normal[1] = g.normal[2] = g.normal[3] = 0.0f;
                g.pbr[0] = g.pbr[1] = g.pbr[2] = g.pbr[3] = 0.0f;
            }
        }
        std::fclose(f);
        *out = rec;
        *out_n = n;
        *st = M2S_OK;
        return 1;
    } catch (const std::bad_alloc&) {
        return refuse(M2S_ERR_OOM, "host allocation failed");
    } catch (...) {
        return refuse(M2S_ERR_IO, "unexpected failure while reading the PLY file");
    }
}

}  // namespace m2s_host

extern "C" m2s_status m2s_write_ply_compact(const char* path, const m2s_gaussian* records, const float* sh, uint32_t sh_degree, uint64_t n,
                                            float scale_multiplier, uint64_t out_counts[3]) {
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = 0;
    if (!path || (n && !records) || (sh && sh_degree > 3)) return M2S_ERR_INVALID;
    if (n > 0xFFFFFFFFull) return M2S_ERR_CAPACITY;
    const uint32_t K = sh ? mc::sh_coefficients(sh_degree) : 0u;
    try {
        // 1, 2: the valid records and their box
        std::vector<uint32_t> idx;
        idx.reserve((size_t)n);
        uint32_t lo[3] = { mc::kOrdMinNeutral, mc::kOrdMinNeutral, mc::kOrdMinNeutral }, hi[3] = { mc::kOrdMaxNeutral, mc::kOrdMaxNeutral, mc::kOrdMaxNeutral };
        for (uint64_t i = 0; i < n; ++i) {
            const m2s_gaussian& g = records[i];
            if (!mc::valid(g.position, g.color, g.scale, g.rotation)) continue;
            idx.push_back((uint32_t)i);
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], mc::ord(g.position[a])); hi[a] = std::max(hi[a], mc::ord(g.position[a])); }
        }
        const uint64_t N = idx.size(), C = (N + mc::kChunkRows - 1) / mc::kChunkRows;
        float bmin[3], bmax[3];
        for (int a = 0; a < 3; ++a) { bmin[a] = mc::unord(lo[a]); bmax[a] = mc::unord(hi[a]); }
        // 3, 4: keys, stable sort
        std::vector<uint32_t> key((size_t)n);
        for (uint32_t i : idx) key[i] = mc::morton_key(records[i].position, bmin, bmax);
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
        std::vector<uint32_t>().swap(key);
        // 5 - 8: chunk by chunk
        std::vector<float> table((size_t)C * 18);
        std::vector<uint32_t> rows((size_t)N * 4);
        std::vector<uint8_t> shb((size_t)N * 3 * K);
        float val[mc::kChunkRows][9];                           // p, ls, col of the chunk's rows
        for (uint64_t c = 0; c < C; ++c) {
            const uint64_t r0 = c * mc::kChunkRows;
            const uint32_t m = (uint32_t)std::min<uint64_t>(mc::kChunkRows, N - r0);
            uint32_t mn[9], mx[9];
            for (int k = 0; k < 9; ++k) { mn[k] = mc::kOrdMinNeutral; mx[k] = mc::kOrdMaxNeutral; }
            for (uint32_t r = 0; r < m; ++r) {
                const uint32_t src = idx[r0 + r];
                const m2s_gaussian& g = records[src];
                float* v = val[r];
                for (int a = 0; a < 3; ++a) {
                    v[a] = g.position[a];
                    v[3 + a] = mc::clamp_log_scale(std::log(g.scale[a] * scale_multiplier));
                    v[6 + a] = sh ? mc::sh_dc_colour(sh[(size_t)src * 48 + a]) : g.color[a];
                }
                for (int k = 0; k < 9; ++k) { mn[k] = std::min(mn[k], mc::ord(v[k])); mx[k] = std::max(mx[k], mc::ord(v[k])); }
            }
            float* t = &table[(size_t)c * 18];
            for (int g3 = 0; g3 < 3; ++g3)
                for (int a = 0; a < 3; ++a) { t[6 * g3 + a] = mc::unord(mn[3 * g3 + a]); t[6 * g3 + 3 + a] = mc::unord(mx[3 * g3 + a]); }
            for (uint32_t r = 0; r < m; ++r) {
                const uint32_t src = idx[r0 + r];
                const m2s_gaussian& g = records[src];
                const float* v = val[r];
                uint32_t* w = &rows[(size_t)(r0 + r) * 4];
                w[0] = mc::pack_11_10_11(v, t, t + 3);
                w[1] = mc::pack_rotation(g.rotation);
                w[2] = mc::pack_11_10_11(v + 3, t + 6, t + 9);
                w[3] = mc::pack_colour(v + 6, t + 12, t + 15, g.color[3]);
                uint8_t* b = K ? &shb[(size_t)(r0 + r) * 3 * K] : nullptr;
                for (uint32_t ch = 0; ch < 3 && K; ++ch)
                    for (uint32_t i = 1; i <= K; ++i) b[ch * K + i - 1] = (uint8_t)mc::sh_byte(sh[(size_t)src * 48 + mc::sh_plane_word(ch, i)]);
            }
        }
        const std::string header = m2s_host::compact_ply_header(C, N, K);
        FILE* f = std::fopen(path, "wb");
        if (!f) return M2S_ERR_IO;
        bool ok = std::fwrite(header.data(), 1, header.size(), f) == header.size();
        ok = ok && (table.empty() || std::fwrite(table.data(), 4, table.size(), f) == table.size());     // (an empty vector's data() may be NULL)
        ok = ok && (rows.empty() || std::fwrite(rows.data(), 4, rows.size(), f) == rows.size());
        ok = ok && (shb.empty() || std::fwrite(shb.data(), 1, shb.size(), f) == shb.size());
        ok = (std::fclose(f) == 0) && ok;
        if (!ok) return M2S_ERR_IO;
        if (out_counts) { out_counts[0] = N; out_counts[1] = C; out_counts[2] = n - N; }
        return M2S_OK;
    } catch (const std::bad_alloc&) {
        return M2S_ERR_OOM;
    } catch (...) {
        return M2S_ERR_IO;
    }
}
