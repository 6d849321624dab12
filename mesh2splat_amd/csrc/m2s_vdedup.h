// m2s_vdedup.h — host interface of m2s_vdedup.hip: the deduplicated vertex table of an uploaded scene (layout and rules: m2s_vtable.h).
#pragma once
#include "m2s_devbuf.h"
#include "m2s_device.h"
#include "m2s_vtable.h"

namespace m2s {

// Temporaries of one deduplication (device memory; released by vt_dedup_finish or release()): the hash table of owner corners
// (vt_hash_words words), per corner its slot / owner, the first-occurrence flags and their scan (corners + 1 words each).
struct VtWork {
    void* mem = nullptr;                    // one allocation; the pointers below lie inside it
    uint32_t *table = nullptr, *owner = nullptr, *flags = nullptr, *rank = nullptr;
    void* temp = nullptr;
    size_t temp_bytes = 0;
    uint32_t corners = 0;
    VtWork() = default;
    VtWork(const VtWork&) = delete;
    VtWork& operator=(const VtWork&) = delete;
    ~VtWork() { release(); }
    void release();
};
uint32_t vt_hash_words(uint32_t corners);   // a power of two, at least twice the corners
// Enqueues hash insertion, flags and scan over the n_tri triangles of `tp` on `st`; does not wait.  1 <= n_tri <= kVtMaxTriangles.
hipError_t vt_dedup_begin(const TriPlanes& tp, uint32_t n_tri, VtWork& w, hipStream_t st);
// Waits for `st`, reads the number of distinct vertices (*n_rows) and, if vt_rows_ok(*n_rows, corners, id_limit, min_sharing), allocates
// rows (3 float4 each) and ids (one VtIds per triangle) at their exact sizes and fills them (*eligible = true; waits again).  Otherwise
// rows / ids are left as they were.  The temporaries are released either way.
hipError_t vt_dedup_finish(const TriPlanes& tp, uint32_t n_tri, VtWork& w, uint32_t id_limit, uint32_t min_sharing, m2s_host::DevBuf<float4>& rows,
                           m2s_host::DevBuf<VtIds>& ids, uint32_t* n_rows, bool* eligible, hipStream_t st);

}  // namespace m2s
