// Who destroys an event and a captured graph.  Event owns one hipEvent_t; StepGraphs owns the decoder's captured decode steps and is
// the only code that destroys one.  Creation, capture, instantiation and every synchronisation stay with the caller.  Host code only,
// in the style of devmem.h: the destroy calls sit behind two seams, and tests/native/stepgraphs_test.cpp runs both owners on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "gen_plan.h"   // StepKind

// the three handle types, as hip_runtime_api.h declares them (so that this header compiles without it)
typedef struct ihipEvent_t* hipEvent_t;
typedef struct ihipGraph* hipGraph_t;
typedef struct hipGraphExec* hipGraphExec_t;

namespace mgea {

// hipEventDestroy; hipGraphExecDestroy, then hipGraphDestroy (capi.hip)
void event_destroy(hipEvent_t ev);
void graph_destroy(hipGraph_t graph, hipGraphExec_t exec);

// One event, null until the caller creates it (hipEventCreate(&e.ev)), destroyed with its owner.
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }   // (move-only: no copy, no assignment)
    ~Event() {
        if (ev) event_destroy(ev);
    }
};

// The captured decode steps of a handle, one (graph, exec) pair per key, at most CAP of them.
struct StepGraphs {
    // two per (batch, form, scored): the single step and the 8-step graph -- (5 forms + 4 scored) x 2 = 18 for one batch size, two batch sizes whole
    // (the graphs of a windowed engine and of guided and scheduled generations share the cache and its LRU)
    static constexpr size_t CAP = 36;
    // one captured launch sequence: that many steps of that StepKind (gen_plan.h) over that many rows
    struct Key {
        int batch; int steps; StepKind kind;
        bool operator==(const Key& o) const { return batch == o.batch && steps == o.steps && kind == o.kind; }
    };
    struct Entry { Key key; hipGraph_t graph; hipGraphExec_t exec; int64_t nodes; uint64_t last_use; };

    StepGraphs() = default;
    StepGraphs(const StepGraphs&) = delete;
    StepGraphs& operator=(const StepGraphs&) = delete;
    ~StepGraphs() { drop_all(); }

    // the entry of `k`, now the most recently used one, or NULL
    const Entry* find(const Key& k) {
        for (Entry& e : entries)
            if (e.key == k) {
                e.last_use = ++clock;
                return &e;
            }
        return nullptr;
    }
    // true: the next insert() destroys the least recently used pair -- which may still be replaying: the caller synchronises first
    bool full() const { return entries.size() >= CAP; }
    // takes a finished pair under a key that is not in the cache
    void insert(const Key& k, hipGraph_t graph, hipGraphExec_t exec, int64_t nodes) {
        if (full()) {
            size_t lru = 0;
            for (size_t i = 1; i < entries.size(); ++i)
                if (entries[i].last_use < entries[lru].last_use) lru = i;
            graph_destroy(entries[lru].graph, entries[lru].exec);
            entries.erase(entries.begin() + (long)lru);
        }
        entries.push_back({k, graph, exec, nodes, ++clock});
        ++n_inserted;
    }
    void drop_all() {
        for (Entry& e : entries) graph_destroy(e.graph, e.exec);
        entries.clear();
    }
    // destroys the entries whose key `pred` accepts; the others keep their stamps
    template <class Pred>
    void drop_if(Pred pred) {
        for (size_t i = entries.size(); i-- > 0;)
            if (pred(entries[i].key)) {
                graph_destroy(entries[i].graph, entries[i].exec);
                entries.erase(entries.begin() + (long)i);
            }
    }
    size_t size() const { return entries.size(); }
    int64_t inserted() const { return n_inserted; }   // over the cache's lifetime: drops and evictions do not lower it

private:
    std::vector<Entry> entries;
    uint64_t clock = 0;
    int64_t n_inserted = 0;
};

}  // namespace mgea
