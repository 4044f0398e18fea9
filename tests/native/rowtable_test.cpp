// RowTable (csrc/rowtable.h) on the CPU, over the malloc seams of devmem_test.cpp and an upload seam that is a memcpy which records
// its range: an allocation that fails at either position, set / copy_row / upload at B = 1 and B = max_batch with guard rows around
// what they may touch, and release through the groups.  Built with -fsanitize=address,undefined and run by tests/test_devmem_host.py;
// exit status 0 and "rowtable ok" = every check held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../music-generation-emotion-adaptive_amd/csrc/rowtable.h"

namespace {
int g_failures = 0;
struct Fake {
    int calls = 0, fail_at = -1, live = 0;
    bool get(void** p, size_t bytes) {
        if (calls++ == fail_at) return false;
        *p = malloc(bytes ? bytes : 1);   // exactly the bytes asked for: AddressSanitizer sees a write past a table's last row
        if (!*p) return false;
        ++live;
        return true;
    }
    void put(void* p) {
        --live;
        free(p);
    }
} g_dev, g_pinned;
struct Upload { void* dst; const void* src; size_t bytes; hipStream_t st; int calls; } g_up{};
}  // namespace

namespace mgea {
bool dev_malloc(void** p, size_t bytes) { return g_dev.get(p, bytes); }
void dev_free(void* p) { g_dev.put(p); }
bool pinned_malloc(void** p, size_t bytes) { return g_pinned.get(p, bytes); }
void pinned_free(void* p) { g_pinned.put(p); }
int upload_async(void* dst, const void* src, size_t bytes, hipStream_t st) {
    g_up = Upload{dst, src, bytes, st, g_up.calls + 1};
    memcpy(dst, src, bytes);
    return MGEA_OK;
}
}  // namespace mgea

using namespace mgea;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++g_failures;                                               \
        }                                                               \
    } while (0)

struct Rec { float a; int32_t b; uint64_t c; };   // a record of several words, as the sampler's
bool same(const Rec& x, const Rec& y) { return x.a == y.a && x.b == y.b && x.c == y.c; }
Rec rec(int i) { return Rec{0.5f * (float)i, i, 1000u + (uint64_t)i}; }

// set, copy_row and upload on a table of max_batch rows with B rows in use
template <int MAX_BATCH>
void range_checks(int B) {
    float* before = nullptr;   // the handle's style: fields first, then the groups that null them
    RowTable<Rec> t;
    RowTable<int32_t> ints;
    float* after = nullptr;
    DevGroup dev;
    PinnedGroup pinned;
    g_dev.fail_at = g_pinned.fail_at = -1;
    CHECK(dev.alloc(&before, 8) == MGEA_OK);
    CHECK(t.allocate(dev, pinned, MAX_BATCH) == MGEA_OK && t.dev && t.stage && t.elt == sizeof(Rec));
    CHECK(ints.allocate(dev, pinned, MAX_BATCH) == MGEA_OK && ints.elt == 4);
    CHECK(dev.alloc(&after, 8) == MGEA_OK);
    CHECK(g_dev.live == 4 && g_pinned.live == 2);
    const Rec guard{-1.f, -1, ~0ull};
    for (int b = 0; b < MAX_BATCH; ++b) {
        t.set(b, guard);
        t.d()[b] = guard;
        ints.set(b, -7);
        ints.d()[b] = -7;
    }
    for (int b = 0; b < B; ++b) {   // the fill of gen_stage
        t.set(b, rec(b));
        ints.set(b, 10 + b);
    }
    for (int b = 0; b < MAX_BATCH; ++b) CHECK(same(t.s()[b], b < B ? rec(b) : guard) && ints.s()[b] == (b < B ? 10 + b : -7));
    if (B > 1) {   // the mirror: row B - 1 takes row 0's record, through the untyped table, and no other row changes
        RowTable<int32_t> own(RowTableBase::OWN);   // (what a mirror skips: never allocated here, so a copy would fault)
        RowTableBase* list[3] = {&t, &own, &ints};
        CHECK(t.mirrored && ints.mirrored && !own.mirrored && own.elt == 4);
        for (RowTableBase* x : list)
            if (x->mirrored) x->copy_row(B - 1, 0);
        for (int b = 0; b < MAX_BATCH; ++b) {
            const int src = b == B - 1 ? 0 : b;
            CHECK(same(t.s()[b], b < B ? rec(src) : guard) && ints.s()[b] == (b < B ? 10 + src : -7));
        }
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(&g_up);   // never dereferenced
    const int calls = g_up.calls;
    CHECK(t.upload(B, st) == MGEA_OK);
    CHECK(g_up.calls == calls + 1 && g_up.dst == t.dev && g_up.src == t.stage && g_up.bytes == (size_t)B * sizeof(Rec) && g_up.st == st);
    CHECK(ints.upload(B, st) == MGEA_OK);
    CHECK(g_up.calls == calls + 2 && g_up.dst == ints.dev && g_up.src == ints.stage && g_up.bytes == (size_t)B * 4);
    for (int b = 0; b < MAX_BATCH; ++b)   // rows [0, B) arrived, the rows behind them kept what they held
        CHECK(same(t.d()[b], b < B ? t.s()[b] : guard) && ints.d()[b] == (b < B ? ints.s()[b] : -7));
    // release through the groups nulls the table, whichever group goes first
    pinned.release();
    CHECK(!t.stage && !ints.stage && t.dev && ints.dev && g_pinned.live == 0);
    dev.release();
    CHECK(!t.dev && !ints.dev && !before && !after && g_dev.live == 0);
}

int main() {
    // an allocation that fails at either position: both pointers null, the groups hold nothing of the table and stay usable
    for (int pos = 0; pos < 2; ++pos) {
        float *x = nullptr, *y = nullptr;
        RowTable<Rec> t;
        DevGroup dev;
        PinnedGroup pinned;
        g_dev = Fake();
        g_pinned = Fake();
        CHECK(dev.alloc(&x, 16) == MGEA_OK && pinned.alloc(&y, 16) == MGEA_OK);   // the groups have other buffers
        (pos == 0 ? g_dev : g_pinned).fail_at = 1;                                // (each group's second call)
        CHECK(t.allocate(dev, pinned, 8) == MGEA_ENOMEM);
        CHECK(!t.dev && !t.stage);
        CHECK(g_dev.live == 1 && g_pinned.live == 1 && x && y);                   // the device array of pos == 1 was given back
        CHECK(g_pinned.calls == (pos == 0 ? 1 : 2));                              // the device array goes first; its failure ends the attempt
        CHECK(t.allocate(dev, pinned, 8) == MGEA_OK && t.dev && t.stage && g_dev.live == 2 && g_pinned.live == 2);
        t.set(7, rec(7));
        dev.release();
        CHECK(!t.dev && !x && t.stage && g_dev.live == 0);
        dev.release();   // idempotent: the dropped field is not freed twice
        pinned.release();
        CHECK(!t.stage && !y && g_pinned.live == 0);
    }
    // drop(): the field that is not in the group is left alone; the last and a middle field go
    {
        float *a = nullptr, *b = nullptr, *c = nullptr, *other = reinterpret_cast<float*>(&g_up);
        DevGroup g;
        g_dev = Fake();
        CHECK(g.alloc(&a, 4) == MGEA_OK && g.alloc(&b, 4) == MGEA_OK && g.alloc(&c, 4) == MGEA_OK);
        g.drop(&other);
        CHECK(other && g_dev.live == 3);
        g.drop(&b);
        CHECK(!b && a && c && g_dev.live == 2);
        g.drop(&c);
        g.drop(&c);
        CHECK(!c && a && g_dev.live == 1);
    }
    CHECK(g_dev.live == 0);
    range_checks<8>(1);
    range_checks<8>(8);
    range_checks<1>(1);
    CHECK(g_dev.live == 0 && g_pinned.live == 0);
    if (g_failures) return 1;
    puts("rowtable ok");
    return 0;
}
