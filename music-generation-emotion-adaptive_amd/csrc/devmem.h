// Who frees a device buffer.  A handle's fields stay raw pointers (kernels, launchers and accessors read them as before); every buffer
// is allocated through the DevGroup of its lifetime, which frees it and nulls the field again.  Host code only.
#pragma once
#include <stddef.h>

#include <utility>
#include <vector>

#include "../../include/mgea.h"

namespace mgea {

// hipMalloc / hipFree (capi.hip).  The only seam: tests/native/devmem_test.cpp puts malloc / free behind it and runs DevGroup on the CPU.
bool dev_malloc(void** p, size_t bytes);   // false: out of memory
void dev_free(void* p);

struct DevGroup {
    DevGroup() = default;
    DevGroup(DevGroup&& o) noexcept : fields(std::move(o.fields)) { o.fields.clear(); }   // (move-only: no copy, no assignment)
    ~DevGroup() { release(); }

    // MGEA_OK (0: calls chain with ||), or MGEA_ENOMEM with *field null and no error string: the caller knows what the buffer was for.
    // *field must live until the group's next release(): a local group is declared after the pointers it fills.
    template <typename T>
    int alloc(T** field, size_t bytes) {
        void* p = nullptr;
        const bool ok = dev_malloc(&p, bytes);
        *field = ok ? static_cast<T*>(p) : nullptr;
        if (ok) fields.push_back(reinterpret_cast<void**>(field));   // (as hipMalloc itself takes it)
        return ok ? MGEA_OK : MGEA_ENOMEM;
    }

    // Frees the group's buffers in the order they were allocated in and nulls the fields.  Idempotent.
    void release() {
        for (void** f : fields) {
            if (*f) dev_free(*f);
            *f = nullptr;
        }
        fields.clear();
    }

private:
    std::vector<void**> fields;
};

}  // namespace mgea
