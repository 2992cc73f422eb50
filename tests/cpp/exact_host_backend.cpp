// exact_host_backend.cpp -- TEST INFRASTRUCTURE.  The exact-mode deflater
// (beast_amd/csrc/deflate_exact_core.h) on the CPU, compiled through
// exact_shim.h, in arrays sized by beast_amd/csrc/exact_plan.h; and the plan's
// rules for tests/test_exact_plan.py.  Built with clang++ by
// tests/model/exact_host.py and by tests/cpp/exact_plan_main.cpp (which
// includes this file); nothing under beast_amd/ loads it.
#include "exact_shim.h"

#include "../../beast_amd/csrc/deflate_exact_core.h"
#include "../../beast_amd/csrc/exact_plan.h"

#include <memory>

using namespace bpmd::dx;

// One message.  tier -1: arrays of the workspace tier's generous sizes, whatever
// the length.  tier 0, 1, 2: as that tier's kernel runs it, every array a heap
// block of its own of exactly the plan's bytes; -2 when the message is not an
// LDS tier's own (the workspace tier's arrays hold any).  Else the payload's
// length, or -1 for need_buffers.
extern "C" int32_t dx_host(int level, int wbits, int mem, int strategy, const uint8_t* msg, uint32_t len, uint8_t* out,
                           uint32_t cap, int tier)
{
    if (level == -1) level = 6;
    if (wbits == 8) wbits = 9;
    const Cfg c = make_cfg(level, wbits, mem, strategy);
    const Ws W = ws_layout(0, c.wbits, c.hbits, c.lit_bufsize);
    size_t win_b = W.prv - W.win, prv_b = W.hd - W.prv;
    uint32_t prv_n = 1u << c.wbits;
    if (tier >= 0) {
        if (tier > 2 || (tier < 2 && tier_of(len, c.hbits) != tier)) return -2;
        prv_n = prv_entries(tier, c.wbits);
        if (tier < 2) {
            const Lds L = lds_layout(sizeof(Trees), tier, c.hbits, c.lit_bufsize);
            win_b = L.prv - L.win;
            prv_b = L.hd - L.prv;
            if (L.syms - L.hd != W.syms - W.hd || L.bytes - L.syms != W.end - W.syms) return -3;
        }
    }
    static thread_local Trees T;
    const std::unique_ptr<uint8_t[]> win(new uint8_t[win_b]()), syms(new uint8_t[W.end - W.syms]());
    const std::unique_ptr<uint16_t[]> prv(new uint16_t[prv_b / 2]()), hd(new uint16_t[(W.syms - W.hd) / 2]());
    return exact_msg(&T, win.get(), prv.get(), hd.get(), syms.get(), prv_n, msg, len, out, cap, c);
}

// ---- the plan, for the Python tests
extern "C" int xp_tier_of(uint32_t len, uint32_t hbits) { return tier_of(len, hbits); }
extern "C" void xp_tables(uint32_t hbits, uint32_t n, uint8_t* tier_out, uint8_t* done_out)
{
    for (uint32_t len = 0; len < n; ++len) {
        tier_out[len] = (uint8_t)tier_of(len, hbits);
        done_out[len] = queue_done(len, hbits);
    }
}
// o: MAX WIN PRV of tiers 0 and 1, then QUEUE_KEY_SHIFT, T2_LDS_HEAD, T2_OCC, T2_WAVES_PER_CU, LDS_HBITS, sizeof(Trees)
extern "C" void xp_constants(uint32_t* o)
{
    for (int t = 0; t < 2; ++t) {
        o[3 * t] = tier(t).MAX;
        o[3 * t + 1] = tier(t).WIN;
        o[3 * t + 2] = tier(t).PRV;
    }
    o[6] = QUEUE_KEY_SHIFT;
    o[7] = T2_LDS_HEAD;
    o[8] = T2_OCC;
    o[9] = T2_WAVES_PER_CU;
    o[10] = LDS_HBITS;
    o[11] = (uint32_t)sizeof(Trees);
}
// o: hbits, lit_bufsize, wbits, level, strategy
extern "C" void xp_cfg(int level, int wbits, int mem, int strategy, uint32_t* o)
{
    const Cfg c = make_cfg(level, wbits, mem, strategy);
    o[0] = c.hbits;
    o[1] = c.lit_bufsize;
    o[2] = c.wbits;
    o[3] = (uint32_t)c.level;
    o[4] = (uint32_t)c.strategy;
}
// o: win prv hd syms bytes (NOT_IN_LDS = 0xFFFFFFFF), prv_entries
extern "C" void xp_lds(uint32_t trees_bytes, int t, uint32_t wbits, uint32_t hbits, uint32_t lit_bufsize, uint32_t* o)
{
    const Lds L = lds_layout(trees_bytes, t, hbits, lit_bufsize);
    o[0] = L.win;
    o[1] = L.prv;
    o[2] = L.hd;
    o[3] = L.syms;
    o[4] = L.bytes;
    o[5] = prv_entries(t, wbits);
}
// o: win prv hd syms end per
extern "C" void xp_ws(uint64_t base, uint32_t wbits, uint32_t hbits, uint32_t lit_bufsize, uint64_t* o)
{
    const Ws W = ws_layout(base, wbits, hbits, lit_bufsize);
    o[0] = W.win;
    o[1] = W.prv;
    o[2] = W.hd;
    o[3] = W.syms;
    o[4] = W.end;
    o[5] = ws_per_wave(wbits, hbits, lit_bufsize);
}
extern "C" uint32_t xp_t2_grid(uint32_t cus, uint32_t n) { return t2_grid(cus, n); }
extern "C" uint32_t xp_t2_waves(uint32_t cus) { return t2_waves(cus); }
