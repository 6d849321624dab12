// m2s_lodtree.h — the level-of-detail tree as the context keeps it: LodTree owns the node planes, the levels and the generation, and is
// the only code that grows the planes, ends a tree or commits one; LodWork is what the cuts, the budget search, the visibility stage and
// the blend work in.  The passes over them: m2s_lod.cpp.
// Self-contained like m2s_devbuf.h (the runtime's API header, the standard library, m2s.h, m2s_recstate.h for the blend's tag): a plain
// host compiler builds tests/lodtree against it, so the planes are typed by their row size and not by the kernels' vector types.
#pragma once
#include "m2s_devbuf.h"
#include "m2s_recstate.h"

#include <algorithm>
#include <type_traits>

namespace m2s_host {

// The planes of the tree, one row per node: the node pool (leaves, then every level a merging step added), a parent word, a bound
// (x, y, z, longer edge) and, only for a tree built with m2s_set_carry_sh on over records with a plane, the SH rows (48 floats).
enum LodPlane : uint32_t { kLodRecords = 0, kLodParent = 1, kLodBounds = 2, kLodSh = 3, kLodPlanes = 4 };

struct LodTree {
    uint32_t levels = 0;                                 // 0: no tree
    uint64_t first[M2S_LOD_MAX_STEPS + 2] = {};          // first node of every level; [levels] = the nodes
    uint32_t R = 0;                                      // resolutionTarget of the leaves
    bool has_sh = false;                                 // the tree has an SH plane ...
    uint32_t sh_degree = 0;                              // ... of this degree
    uint32_t model = M2S_MERGE_MODEL_FOOTPRINT;          // the merge model the tree was built under, and its sigma (m2s_lod_blend refuses
    float sigma = 1.0f;                                  // a Gaussian tree)
    uint64_t gen = 0;                                    // counts the trees this context has had: end() advances it

    static constexpr size_t row_bytes(uint32_t which) { return which == kLodRecords ? sizeof(m2s_gaussian) : which == kLodParent ? 4 : which == kLodBounds ? 16 : 192; }
    uint64_t nodes() const { return first[levels]; }
    uint64_t cap(uint32_t which) const { return plane_[which].cap(); }
    // Plane `which` as the ABI hands it out: NULL without a tree, for a tree of no nodes and for the SH plane of a tree that has none.
    const void* plane(uint32_t which) const { return levels && nodes() && (which != kLodSh || has_sh) ? plane_[which].get() : nullptr; }
    // Row i of plane `which` as the kernels type it (T: float4, uint32_t, float), whatever tree there is: what a build fills.
    template <typename T> T* rows(uint32_t which, uint64_t i = 0) const { return reinterpret_cast<T*>(static_cast<char*>(plane_[which].get()) + i * row_bytes(which)); }
    // What the per-level launchers take (K: LodLevelsK of m2s_device.h, whose `bounds` names the kernels' type of a bound).
    template <typename K> K levels_k() const {
        return K{ rows<std::remove_pointer_t<decltype(K::bounds)>>(kLodBounds), rows<const uint32_t>(kLodParent), first, levels };
    }

    // Room for `want` nodes in the three node planes — and in the SH plane, for a tree that has one (sh) —, the first `keep` nodes of
    // every plane kept where it has to move (keep <= the old capacity).  The node planes grow together, to max(want, 2 * cap, 1); the SH
    // plane, short or absent, to max(want, their capacity, 1).  Every new block first, the kept rows copied on `stream`, one synchronise,
    // then the swap: a failed allocation leaves the old planes and their rows as they were.
    m2s_status reserve(std::string& err, hipStream_t stream, uint64_t want, uint64_t keep, bool sh) {
        const bool grow = cap(kLodRecords) < want || !plane_[kLodRecords].get();
        const uint64_t node_cap = grow ? std::max<uint64_t>(std::max<uint64_t>(want, 2 * cap(kLodRecords)), 1) : cap(kLodRecords);
        const bool grow_sh = sh && (cap(kLodSh) < want || !plane_[kLodSh].get());
        DevBuf<void> fresh[kLodPlanes];
        for (uint32_t w = 0; w < kLodPlanes; ++w)
            if (w == kLodSh ? grow_sh : grow)
                if (m2s_status s = fresh[w].reserve(err, w == kLodSh ? std::max<uint64_t>(std::max<uint64_t>(want, node_cap), 1) : node_cap, row_bytes(w))) return s;
        bool copied = false;
        for (uint32_t w = 0; w < kLodPlanes; ++w)
            if (fresh[w].get() && keep && plane_[w].get()) {
                if (m2s_status s = hip_status(err, "hipMemcpyAsync (the tree's kept rows)",
                                              hipMemcpyAsync(fresh[w].get(), plane_[w].get(), keep * row_bytes(w), hipMemcpyDeviceToDevice, stream))) return s;
                copied = true;
            }
        if (copied)
            if (m2s_status s = hip_status(err, "hipStreamSynchronize (the tree's kept rows)", hipStreamSynchronize(stream))) return s;
        for (uint32_t w = 0; w < kLodPlanes; ++w)
            if (fresh[w].get()) plane_[w].swap(fresh[w]);
        return M2S_OK;
    }
    void drop_sh() { plane_[kLodSh].release(); }         // (192 bytes per node: not kept for a tree that has no use for it)
    // The tree ends here, whatever follows: no levels, the next generation (what m2s_lod_blend tells one tree's cut from another's by).
    void end() { levels = 0; ++gen; has_sh = false; }
    void release() {
        end();
        for (DevBuf<void>& p : plane_) p.release();
    }
    // A finished build: n_levels levels whose first nodes are first_in[0 .. n_levels] (first_in[n_levels]: the nodes).
    void commit(uint32_t n_levels, const uint64_t* first_in, uint32_t leaves_R, bool sh, uint32_t degree, uint32_t merge_model, float merge_sigma) {
        for (uint32_t l = 0; l < M2S_LOD_MAX_STEPS + 2; ++l) first[l] = first_in[std::min(l, n_levels)];
        levels = n_levels; R = leaves_R; has_sh = sh; sh_degree = degree; model = merge_model; sigma = merge_sigma;
    }

private:
    DevBuf<void> plane_[kLodPlanes];                     // one capacity of nodes each (the SH plane: its own)
};

// What the passes over the tree work in.  Sized by the tree (released with it): a byte per node (every ancestor-or-self refines), the
// budget search's keys (L, H: a uint2 per node), the visibility byte per node, a host depth image's copy on the device (no other pass
// reads it), the blend's weight per record of the last cut (valid while blend_tag holds).  Kept: the cut's count words (kLodCountWords),
// the node index of every record of the last cut (valid while RecordState::lod_ids_tag holds; ids_gen: the tree — LodTree::gen — they
// index), the search's words (kLodBudgetStateWords), the blend's count words (kLodBlendCountWords).
struct LodWork {
    DevBuf<uint8_t> open, vis;
    DevBuf<void> lh;
    DevBuf<float> occ_depth, blend_t;                    // occ_depth: capacity in texels
    DevBuf<uint32_t> counts, ids, budget_state, blend_counts;
    uint64_t ids_gen = 0;
    RecordsTag blend_tag;
    void release_tree_sized() {
        open.release(); lh.release(); vis.release(); occ_depth.release(); blend_t.release();
        blend_tag.clear();
    }
};

}  // namespace m2s_host
