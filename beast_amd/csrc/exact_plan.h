// exact_plan.h -- the rules of exact-mode deflate (pmd_deflate_exact.hip:
// deflate_exact_kernel and its driver) as pure functions and
// constants: the configuration, the tiers by message length, where each
// tier's arrays lie in LDS and in the per-wave workspace, the grid, and when
// the workspace tier's queue is done.  The kernel takes every pointer from
// here and the driver every size.  Host-compilable without HIP:
// tests/test_exact_plan.py checks the rules, tests/cpp/exact_host_backend.cpp
// runs the deflater (deflate_exact_core.h) in heap blocks of exactly these
// sizes, tests/cpp/exact_plan_main.cpp under the address sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "send_plan.h"   // BPMD_SP_HD

namespace bpmd {
namespace dx {

// zlib's match lengths; LOOK is MIN_LOOKAHEAD, WINIT the bytes kept zeroed
// behind the data (deflate_stream.hpp: minMatch, maxMatch, kWinInit)
enum : int { MINM = 3, MAXM = 258, LOOK = MAXM + MINM + 1, WINIT = MAXM };

struct Cfg {
    int level, strategy;
    uint32_t wbits, hbits, lit_bufsize;
};
// from the public configuration, already validated (deflate_stream.ipp:227-265)
BPMD_SP_HD constexpr Cfg make_cfg(int level, int window_bits, int mem_level, int strategy)
{
    return {level, strategy, (uint32_t)window_bits, (uint32_t)mem_level + 7, 1u << (mem_level + 6)};
}

// ---- tiers.  0 and 1 keep window, prev_, head and the symbol buffer in LDS
// (memLevel <= 5, by message length); 2 is the per-wave global workspace.
struct Tier {
    uint32_t MAX, WIN, PRV;   // longest message; window bytes; prev_ entries
};
BPMD_SP_HD constexpr Tier tier(int t) { return t == 0 ? Tier{4096, 4096 + 512, 4096} : Tier{8192 - LOOK, 8192 + 512, 8192}; }
constexpr uint32_t LDS_HBITS = 12;   // the LDS tiers' largest head[] (memLevel 5)
BPMD_SP_HD constexpr int tier_of(uint32_t len, uint32_t hbits)
{
    return hbits > LDS_HBITS ? 2 : len <= tier(0).MAX ? 0 : len <= tier(1).MAX ? 1 : 2;
}

// The deflater touches window bytes below strstart + lookahead + WINIT (the
// zeroed bytes; a comparison reads up to strstart + MAXM - 1) and the
// workspace tier gives it 2 * w_size + MAXM + 64.  A tier's LDS window holds
// either that much of the physical window (then slides run as in tier 2, over
// w_size <= PRV entries of prev_), or, when the physical window is larger,
// the longest message and the WINIT bytes behind it: the message ends before
// a slide can begin (strstart >= 2 * w_size - LOOK), so no position reaches
// past MAX, in the window or in prev_.
constexpr uint32_t WIN_SLACK = MAXM + 64;
BPMD_SP_HD constexpr bool tier_holds(Tier t, uint32_t wbits)
{
    const uint32_t w2 = 2u << wbits;
    return w2 + WIN_SLACK <= t.WIN ? w2 / 2 <= t.PRV : (t.MAX + LOOK < w2 && t.MAX + WINIT <= t.WIN && t.MAX <= t.PRV);
}
BPMD_SP_HD constexpr bool tier_sound(Tier t)
{
    for (uint32_t wbits = 9; wbits <= 15; ++wbits)
        if (!tier_holds(t, wbits)) return false;
    return t.WIN % 16 == 0 && (2 * t.PRV) % 16 == 0;
}
static_assert(tier_sound(tier(0)) && tier_sound(tier(1)), "every windowBits fits each LDS tier; 16-byte regions");
static_assert(tier(0).MAX < tier(1).MAX && tier(0).PRV >= tier(0).MAX && tier(1).PRV >= tier(1).MAX, "tiers by length");

BPMD_SP_HD constexpr size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }
BPMD_SP_HD constexpr uint32_t prv_entries(int t, uint32_t wbits)   // prev_ entries cleared per message
{
    const uint32_t wsize = 1u << wbits;
    return t < 2 && wsize > tier(t).PRV ? tier(t).PRV : wsize;
}

// ---- LDS of one wave (one workgroup), from the 16-byte-aligned tree
// workspace of trees_bytes:  trees | win | prv | hd | syms  in tiers 0 and 1;
// trees | hd  in tier 2 when head[] has at most T2_LDS_HEAD entries (one
// global round trip fewer per inserted position), else trees alone.
constexpr uint32_t T2_LDS_HEAD = 2048;
BPMD_SP_HD constexpr bool t2_head_in_lds(uint32_t hbits) { return (1u << hbits) <= T2_LDS_HEAD; }
constexpr uint32_t NOT_IN_LDS = ~0u;
struct Lds {
    uint32_t win, prv, hd, syms, bytes;   // offsets, or NOT_IN_LDS; the dynamic LDS request
};
BPMD_SP_HD constexpr Lds lds_layout(size_t trees_bytes, int t, uint32_t hbits, uint32_t lit_bufsize)
{
    const uint32_t trees = (uint32_t)al16(trees_bytes), hash_size = 1u << hbits;
    if (t == 2) {
        const bool in = t2_head_in_lds(hbits);
        return {NOT_IN_LDS, NOT_IN_LDS, in ? trees : NOT_IN_LDS, NOT_IN_LDS, trees + (in ? 2 * hash_size : 0u)};
    }
    const uint32_t prv = trees + tier(t).WIN, hd = prv + 2 * tier(t).PRV, syms = hd + 2 * hash_size;
    return {trees, prv, hd, syms, syms + 3 * lit_bufsize};
}

// ---- tier 2's workspace of one wave, from the address `base` (16-byte
// aligned; 0 gives offsets):  win | prv | hd | syms, and WS_PAD bytes
constexpr uint32_t WS_PAD = 64;
struct Ws {
    size_t win, prv, hd, syms, end;
};
BPMD_SP_HD constexpr Ws ws_layout(size_t base, uint32_t wbits, uint32_t hbits, uint32_t lit_bufsize)
{
    const uint32_t wsize = 1u << wbits, hash_size = 1u << hbits;
    const size_t prv = al16(base + (2 * wsize + WIN_SLACK)), hd = prv + 2 * wsize, syms = hd + 2 * hash_size;
    return {base, prv, hd, syms, syms + 3 * lit_bufsize};
}
BPMD_SP_HD constexpr size_t ws_per_wave(uint32_t wbits, uint32_t hbits, uint32_t lit_bufsize)
{
    return ws_layout(0, wbits, hbits, lit_bufsize).end + WS_PAD;
}

// ---- tier 2's grid.  Its waves wait on global memory most of the time, so
// the kernel is held to T2_OCC waves per SIMD (<= 128 VGPRs) and as many run
// on every CU; the workspace has room for all of them.
constexpr uint32_t T2_OCC = 4, T2_WAVES_PER_CU = 4 * T2_OCC;
BPMD_SP_HD constexpr uint32_t t2_waves(uint32_t cus) { return cus * T2_WAVES_PER_CU; }
BPMD_SP_HD constexpr uint32_t t2_grid(uint32_t cus, uint32_t n) { return t2_waves(cus) < n ? t2_waves(cus) : n; }

// ---- tier 2's queue hands the messages out longest first, in the order of
// the keys len >> QUEUE_KEY_SHIFT (lane_order's).  A wave that draws `len`
// stops when no message of a key up to len's can be tier 2: every later one
// is shorter than (len | 63) + 1 <= len + 64.
constexpr uint32_t QUEUE_KEY_SHIFT = 6;
BPMD_SP_HD constexpr bool queue_done(uint32_t len, uint32_t hbits)
{
    return hbits <= LDS_HBITS && len + (1u << QUEUE_KEY_SHIFT) <= tier(1).MAX;
}

}  // namespace dx
}  // namespace bpmd
