// bp_workspace.h -- how large the block-parallel inflate's decode workspace
// is for a stream, and how that capacity moves.  Pure host code without HIP
// (tests/test_bp_workspace.py compiles it with g++); pmd_inflate_bp.hip keeps
// one Capacity per (device, stream) under its mutex, asks the device for its
// free memory, allocates, and calls these.
//
// The capacity is what bp_fit_kernel admits: tasks (regions) and symbol words.
//   * It grows to the totals an earlier call needed plus a quarter, within
//     half the device's free memory (grow_to).
//   * A workspace that cannot be allocated falls back to the last capacity
//     that could -- halving, and below 2^16 words to none: every long payload
//     then takes the wave kernel (alloc_failed, alloc_retry).
//   * The capacity that could be had is then a ceiling for the next `hold`
//     calls (8, doubling with every failure up to 1024), so under memory
//     pressure a call does not sync, free and fail to allocate again every
//     time (alloc_settled).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bp.h"

namespace bpmd {
namespace bp {

// tasks and symbol words: a capacity, or what a batch needs
struct Need {
    unsigned long long tasks, words;
};

struct Capacity {
    unsigned long long tasks = 0, words = 0;
    unsigned long long ceil_tasks = 0, ceil_words = 0;   // in force while hold > 0
    uint32_t hold = 0, backoff = 8;
    bool sized = false;   // set by the stream's first call or by a reserve
};

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// decode workspace layout for a capacity (n: the batch's message count):
// tasks, results, fallback list, region map, marks, symbols
struct DwLayout {
    size_t tasks, res, fb, map, mark, sym, bytes;
    DwLayout(Need cap, uint32_t n)
    {
        tasks = 0;
        res = al256(tasks + sizeof(SegTask) * cap.tasks);
        fb = al256(res + sizeof(SegRes) * cap.tasks);
        map = al256(fb + 4ull * n);
        mark = al256(map + 4ull * cap.tasks);
        sym = al256(mark + 4ull * n);
        bytes = al256(sym + 2ull * (cap.words + SYM_GUARD + 64));
    }
};
inline size_t dw_bytes(Need cap, uint32_t n) { return DwLayout(cap, n).bytes; }

// bpmd_inflate_reserve: a capacity for batches whose long payloads total at
// most in_bytes of input, out_bytes of output capacity and msgs payloads --
// bp_stats_kernel's bounds: regions of >= R_MIN bytes, at most one more per
// payload; slots of 3 (len + regions) x F16 symbols, F16 = 1.25 x
// min(cap / len, 4), + SLACK per region + the guard per payload.
inline Need reserve_need(unsigned long long in_bytes, unsigned long long out_bytes, unsigned long long msgs)
{
    const unsigned long long t = in_bytes / R_MIN + msgs;
    return {t, (15 * out_bytes) / 4 + (15ull + SLACK) * t + (SYM_GUARD + 64ull) * msgs};
}

// the capacity `want` asks for before any bound: itself plus a quarter where
// it exceeds the present one, at most 2^32 - 1 tasks (task indices are 32 bits)
inline Need headroom(const Capacity& c, Need want)
{
    Need g = {c.tasks, c.words};
    if (want.tasks > g.tasks) g.tasks = want.tasks + want.tasks / 4;
    if (want.words > g.words) g.words = want.words + want.words / 4;
    if (g.tasks > 0xffffffffull) g.tasks = 0xffffffffull;
    return g;
}
// whether grow_to(c, want, ...) depends on the free memory at all
inline bool grows(const Capacity& c, Need want)
{
    const Need g = headroom(c, want);
    return g.tasks != c.tasks || g.words != c.words;
}

constexpr unsigned long long FREE_UNKNOWN = ~0ull;

// grows the capacity to `want` plus a quarter, within half of free_bytes
// (FREE_UNKNOWN: unbounded) and the ceiling while it holds; never shrinks
inline void grow_to(Capacity& c, Need want, unsigned long long free_bytes)
{
    Need g = headroom(c, want);
    if (grows(c, want) && free_bytes != FREE_UNKNOWN) {
        // per task: the task, its result and the region map word
        const unsigned long long budget = free_bytes / 2, per_task = sizeof(SegTask) + sizeof(SegRes) + 4;
        if (g.tasks * per_task > budget) g.tasks = budget / per_task;
        if (2 * g.words + g.tasks * per_task > budget) g.words = (budget - g.tasks * per_task) / 2;
    }
    if (c.hold) {
        g.tasks = g.tasks < c.ceil_tasks ? g.tasks : c.ceil_tasks;
        g.words = g.words < c.ceil_words ? g.words : c.ceil_words;
    }
    c.tasks = g.tasks > c.tasks ? g.tasks : c.tasks;
    c.words = g.words > c.words ? g.words : c.words;
}

// a call begins: the ceiling lifts after `hold` calls
inline void begin_call(Capacity& c)
{
    if (c.hold) --c.hold;
}

// below 2^16 words a workspace is not worth its scan: none at all
inline Need floored(Need x) { return x.words < (1ull << 16) ? Need{0, 0} : x; }

// The workspace for `failed` could not be allocated.  Halves the stream's
// capacity where it is still the one that failed (another thread may have
// moved it since) and returns the size to try next.
inline Need alloc_failed(Capacity& c, Need failed)
{
    if (c.tasks == failed.tasks) c.tasks /= 2;
    if (c.words == failed.words) c.words /= 2;
    return floored({c.tasks, c.words});
}
// `tried` could not be allocated either: the next size to try, or false when
// `tried` was none already (not even the lists fit)
inline bool alloc_retry(Need& tried)
{
    if (tried.words == 0) return false;
    tried = floored({tried.tasks / 2, tried.words / 2});
    return true;
}
// `got` could be allocated after a failure: the capacity, and its ceiling for
// the next `backoff` calls
inline void alloc_settled(Capacity& c, Need got)
{
    c.tasks = c.ceil_tasks = got.tasks;
    c.words = c.ceil_words = got.words;
    c.hold = c.backoff;
    c.backoff = c.backoff < 1024 ? 2 * c.backoff : 1024u;
}

}  // namespace bp
}  // namespace bpmd
