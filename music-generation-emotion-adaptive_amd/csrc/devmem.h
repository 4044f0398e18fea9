// Who frees a buffer.  A handle's fields stay raw pointers (kernels, launchers and accessors read them as before); every buffer is
// allocated through the group of its lifetime, which frees it and nulls the field again: DevGroup for device memory, PinnedGroup for
// pinned host memory.  Host code only.
#pragma once
#include <stddef.h>

#include <utility>
#include <vector>

#include "../../include/mgea.h"

namespace mgea {

// hipMalloc / hipFree and hipHostMalloc (flags 0) / hipHostFree (capi.hip).  The only seams: tests/native/devmem_test.cpp puts
// malloc / free behind them and runs both groups on the CPU.
bool dev_malloc(void** p, size_t bytes);   // false: out of memory
void dev_free(void* p);
bool pinned_malloc(void** p, size_t bytes);
void pinned_free(void* p);

template <bool (*Malloc)(void**, size_t), void (*Free)(void*)>
struct BufGroup {
    BufGroup() = default;
    BufGroup(BufGroup&& o) noexcept : fields(std::move(o.fields)) { o.fields.clear(); }   // (move-only: no copy, no assignment)
    ~BufGroup() { release(); }

    // MGEA_OK (0: calls chain with ||), or MGEA_ENOMEM with *field null and no error string: the caller knows what the buffer was for.
    // *field must live until the group's next release(): a local group is declared after the pointers it fills.
    template <typename T>
    int alloc(T** field, size_t bytes) {
        void* p = nullptr;
        const bool ok = Malloc(&p, bytes);
        *field = ok ? static_cast<T*>(p) : nullptr;
        if (ok) fields.push_back(reinterpret_cast<void**>(field));   // (as hipMalloc itself takes it)
        return ok ? MGEA_OK : MGEA_ENOMEM;
    }

    // Frees the group's buffers in the order they were allocated in and nulls the fields.  Idempotent.
    void release() {
        for (void** f : fields) {
            if (*f) Free(*f);
            *f = nullptr;
        }
        fields.clear();
    }

    // Frees the buffer of one field, nulls it and forgets it: for an owner of two buffers whose second allocation failed.
    template <typename T>
    void drop(T** field) {
        void** f = reinterpret_cast<void**>(field);
        for (size_t i = fields.size(); i-- > 0;) {
            if (fields[i] != f) continue;
            if (*f) Free(*f);
            *f = nullptr;
            fields.erase(fields.begin() + (long)i);
            return;
        }
    }

private:
    std::vector<void**> fields;
};
using DevGroup = BufGroup<dev_malloc, dev_free>;
using PinnedGroup = BufGroup<pinned_malloc, pinned_free>;

}  // namespace mgea
