// One per-row record table of a generation: a [max_batch] device array, which the captured step graphs point at, and the pinned host
// array its rows are staged in before a call's first step.  RowTable owns neither: the handle's groups (devmem.h) free them and null the
// fields.  Host code only, as devmem.h and hipres.h: the one runtime call is a seam, and tests/native/rowtable_test.cpp runs on the CPU.
#pragma once
#include <string.h>

#include "devmem.h"

typedef struct ihipStream_t* hipStream_t;   // as hip_runtime_api.h declares it (so that this header compiles without it)

namespace mgea {
#pragma GCC visibility push(hidden)

// hipMemcpyAsync host -> device on `st` (capi.hip): MGEA_OK, or MGEA_EHIP with the error string set
int upload_async(void* dst, const void* src, size_t bytes, hipStream_t st);

// The untyped table: what staging code that walks a list of tables of several record types needs.
struct RowTableBase {
    void* dev = nullptr;     // [max_batch] records on the device
    void* stage = nullptr;   // [max_batch] pinned records; whoever rewrites them waits for the previous upload first (stage_free)
    size_t elt = 0;          // bytes of one record
    // a row that runs on another row's inputs (a guidance shadow, a blend member) takes that row's record, unless the table is the row's OWN
    enum Kind { MIRRORED, OWN };
    bool mirrored = true;
    void copy_row(int u, int b) { memcpy(static_cast<char*>(stage) + (size_t)u * elt, static_cast<const char*>(stage) + (size_t)b * elt, elt); }   // staged row u <- staged row b
    int upload(int B, hipStream_t st) const { return upload_async(dev, stage, (size_t)B * elt, st); }   // staged rows [0, B) -> device, in stream order
};

template <typename T>
struct RowTable : RowTableBase {
    explicit RowTable(Kind k = MIRRORED) { elt = sizeof(T), mirrored = k == MIRRORED; }
    T* d() const { return static_cast<T*>(dev); }
    T* s() const { return static_cast<T*>(stage); }
    void set(int b, const T& v) { s()[b] = v; }
    // Both arrays at the END of their groups, the device array first (as arrays of T: the groups' alloc<T>).  MGEA_ENOMEM (no error
    // string, as BufGroup::alloc): both fields null again and neither group holds anything of the table.
    int allocate(DevGroup& dg, PinnedGroup& pg, int max_batch) {
        T **pd = reinterpret_cast<T**>(&dev), **ps = reinterpret_cast<T**>(&stage);
        if (dg.alloc(pd, (size_t)max_batch * elt)) return MGEA_ENOMEM;
        if (pg.alloc(ps, (size_t)max_batch * elt) == MGEA_OK) return MGEA_OK;
        dg.drop(pd);
        return MGEA_ENOMEM;
    }
};

#pragma GCC visibility pop
}  // namespace mgea
