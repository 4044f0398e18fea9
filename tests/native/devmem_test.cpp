// DevGroup and PinnedGroup (csrc/devmem.h) on the CPU: each group's malloc / free pair over malloc / free with a "fail the k-th call"
// counter and a count of live allocations of its own (a buffer freed through the other group's seam shows in both counts).  Built with
// -fsanitize=address,undefined and run by tests/test_devmem_host.py; exit status 0 = every check held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../music-generation-emotion-adaptive_amd/csrc/devmem.h"

namespace {
int g_failures = 0;
struct Fake {
    int calls = 0, fail_at = -1, live = 0;
    bool get(void** p, size_t bytes) {
        if (calls++ == fail_at) return false;
        *p = malloc(bytes ? bytes : 1);
        if (!*p) return false;
        ++live;
        return true;
    }
    void put(void* p) {
        --live;
        free(p);
    }
} g_dev, g_pinned;
}  // namespace

namespace mgea {
bool dev_malloc(void** p, size_t bytes) { return g_dev.get(p, bytes); }
void dev_free(void* p) { g_dev.put(p); }
bool pinned_malloc(void** p, size_t bytes) { return g_pinned.get(p, bytes); }
void pinned_free(void* p) { g_pinned.put(p); }
}  // namespace mgea

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++g_failures;                                               \
        }                                                               \
    } while (0)

// a handle in the engines' style: raw fields of several types, one group
template <class Group>
struct Handle {
    Group dev;
    float* a = nullptr;
    void* b = nullptr;
    int32_t* c = nullptr;
    struct Inner { uint32_t* d = nullptr; } in;
    float* e = nullptr;
    static constexpr int N = 5;
    int grow(size_t scale) {   // the engines' chain: stops at the first failure
        return dev.alloc(&a, 16 * scale) || dev.alloc(&b, 3 * scale) || dev.alloc(&c, 64 * scale) || dev.alloc(&in.d, 8 * scale) ||
                       dev.alloc(&e, scale)
                   ? MGEA_ENOMEM
                   : MGEA_OK;
    }
    bool all_null() const { return !a && !b && !c && !in.d && !e; }
    bool all_set() const { return a && b && c && in.d && e; }
};

// every check on one group type, whose seam is the fake `f`
template <class Group>
void group_checks(Fake& f) {
    using Handle = ::Handle<Group>;
    int& g_calls = f.calls;
    int& g_live = f.live;
    auto arm = [&f](int fail_at) {
        f.calls = 0;
        f.fail_at = fail_at;
    };
    // every k-th allocation of a group of n failing: after the caller's release() nothing is live and every field reads null
    for (int k = 0; k < Handle::N; ++k) {
        Handle h;
        arm(k);
        CHECK(h.grow(1) == MGEA_ENOMEM);
        CHECK(g_calls == k + 1);   // the chain stopped at the failure
        CHECK(g_live == k);
        h.dev.release();
        CHECK(h.all_null());
        CHECK(g_live == 0);
    }
    // a failed alloc() answers MGEA_ENOMEM with the field null and the group as it was
    {
        float *x = nullptr, *y = reinterpret_cast<float*>(&g_live);
        Group g;
        arm(1);
        CHECK(g.alloc(&x, 32) == MGEA_OK && x);
        CHECK(g.alloc(&y, 32) == MGEA_ENOMEM && !y);
        CHECK(g_live == 1);
        x[7] = 1.f;   // the buffer is usable memory of the size asked for
        g.release();
        CHECK(!x && g_live == 0);
    }
    // release() twice is harmless; release then regrow works (ensure_ws: bigger buffers through the same fields)
    {
        Handle h;
        arm(-1);
        CHECK(h.grow(1) == MGEA_OK && h.all_set() && g_live == Handle::N);
        h.dev.release();
        h.dev.release();
        CHECK(h.all_null() && g_live == 0);
        CHECK(h.grow(4) == MGEA_OK && h.all_set() && g_live == Handle::N);
        h.c[64 * 4 / sizeof(int32_t) - 1] = 7;
        // a regrowth that fails halfway, released, leaves nothing behind
        h.dev.release();
        arm(2);
        CHECK(h.grow(8) == MGEA_ENOMEM);
        h.dev.release();
        CHECK(h.all_null() && g_live == 0);
        arm(-1);
        CHECK(h.grow(2) == MGEA_OK && g_live == Handle::N);
    }   // destruction releases
    CHECK(g_live == 0);
    // a zero-byte allocation is a success (hipMalloc answers NULL for it) and costs nothing to release
    {
        float* z = nullptr;
        Group g;   // (after the field: the group writes to it when it goes)
        arm(-1);
        CHECK(g.alloc(&z, 0) == MGEA_OK);
    }
    CHECK(g_live == 0);
    // a moved-from group owns nothing (and is a working empty group); the buffers live until the new owner goes
    {
        float *x = nullptr, *y = nullptr;
        arm(-1);
        Group a;
        CHECK(a.alloc(&x, 8) == MGEA_OK);
        {
            Group b(std::move(a));
            a.release();
            CHECK(x && g_live == 1);
            CHECK(a.alloc(&y, 8) == MGEA_OK && g_live == 2);
        }
        CHECK(!x && y && g_live == 1);
        a.release();
        CHECK(!y && g_live == 0);
    }
}

int main() {
    group_checks<mgea::DevGroup>(g_dev);
    CHECK(g_pinned.calls == 0);   // (each group reaches its own pair)
    group_checks<mgea::PinnedGroup>(g_pinned);
    CHECK(g_dev.live == 0 && g_pinned.live == 0);
    if (g_failures) return 1;
    puts("devmem ok");
    return 0;
}
