// pmd_deflate_exact.hip -- exact mode of the batch deflater (BPMD_F_EXACT,
// SURVEY.md §8(f) N4): payloads bit-identical to Beast's deflate_stream
// (include/boost/beast/zlib/detail/deflate_stream.ipp) under the
// permessage-deflate call sequence of impl_base<true>::deflate
// (websocket/detail/impl_base.hpp:85-154: Flush::none over the message,
// Flush::block, Flush::sync, 00 00 FF FF dropped) with a reset per message.
//
// Exactness needs Beast's serial decisions: the lazy parse (each match
// decision depends on the previous one), hash chains in insertion order,
// blocks cut when the symbol buffer fills (lit_bufsize - 1 symbols),
// Huffman trees from zlib's heap with its depth tie-break, the
// stored/fixed/dynamic choice, and even the bytes a match comparison sees
// past the end of the data after a window slide.  So one WAVE runs one
// message's state machine as wave-uniform code, and the lanes share the
// bulk work inside it: the 256-byte match comparisons of longest_match
// (64 bytes per step, first mismatch by ballot), window fills and slides,
// table clears.  The window / prev / head arrays live in LDS for messages
// of up to 4 096 and up to 7 930 bytes at memLevel <= 5 (tiers 0 and 1) and
// in a per-wave global workspace otherwise (tier 2); the code is the same
// through generic pointers.  Tree construction uses per-wave LDS in all.
//
// The deflater itself is deflate_exact_core.h (exact_msg); the tiers, where
// their arrays lie, the grid and the queue's rule are exact_plan.h.  Here:
// the kernel, which hands each message to exact_msg, and its driver.
#include "pmd_common.h"
#include "pmd_internal.h"

#include "deflate_exact_core.h"
#include "exact_plan.h"

namespace bpmd {
namespace dx {

// Where a tier's arrays begin, as steps from p: behind the trees in LDS (tiers
// 0 and 1), the wave's workspace (tier 2).  exact_plan.h has the layouts as
// offsets; the kernel takes these steps on a pointer instead, in this order
// and from its own wsize, which is what keeps its instructions those it was
// measured with (a pointer built from an offset, or wsize shifted after the
// workspace's address, schedules differently).  Taken on an offset, as below,
// the steps land on the plan's layouts at every configuration.
template <class P> struct Arrays {
    P win, prv, hd, syms;
    uint32_t prv_n;
};
template <int TIER, class P> __host__ __device__ constexpr Arrays<P> carve(P p, uint32_t wsize, uint32_t hbits)
{
    const uint32_t hash_size = 1u << hbits;
    Arrays<P> a{};
    a.win = p;
    if constexpr (TIER < 2) {
        constexpr Tier D = tier(TIER);
        p += D.WIN;
        a.prv = p;
        a.prv_n = wsize < D.PRV ? wsize : D.PRV;
        p += 2 * D.PRV;
    } else {
        p += 2 * wsize + WIN_SLACK;
        p = (P)(((uintptr_t)p + 15) & ~(uintptr_t)15);
        a.prv = p;
        a.prv_n = wsize;
        p += 2 * wsize;
    }
    a.hd = p;
    p += 2 * hash_size;
    a.syms = p;
    return a;
}
template <int TIER> constexpr bool plan_holds()
{
    for (uint32_t wbits = 9; wbits <= 15; ++wbits)
        for (int mem = 1; mem <= 9; ++mem) {
            const Cfg c = make_cfg(6, (int)wbits, mem, 0);
            const Lds L = lds_layout(sizeof(Trees), TIER, c.hbits, c.lit_bufsize);
            const Ws W = ws_layout(0, c.wbits, c.hbits, c.lit_bufsize);
            // no launch raises the dynamic-LDS limit (the LDS tiers run at memLevel <= 5 only)
            if ((TIER == 2 || c.hbits <= LDS_HBITS) && L.bytes > 65536) return false;
            const Arrays<size_t> a = carve<TIER, size_t>(TIER < 2 ? al16(sizeof(Trees)) : 0, 1u << c.wbits, c.hbits);
            if (a.prv_n != prv_entries(TIER, c.wbits)) return false;
            if (TIER < 2 ? a.win != L.win || a.prv != L.prv || a.hd != L.hd || a.syms != L.syms
                         : a.win != W.win || a.prv != W.prv || a.hd != W.hd || a.syms != W.syms)
                return false;
            if (TIER == 2 && L.hd != (t2_head_in_lds(c.hbits) ? (uint32_t)al16(sizeof(Trees)) : NOT_IN_LDS)) return false;
        }
    return true;
}
static_assert(plan_holds<0>() && plan_holds<1>() && plan_holds<2>(), "the kernel's carve is the plan's; LDS <= 64 KiB");
static_assert(QUEUE_KEY_SHIFT == LANE_ORDER_KEY_SHIFT, "queue_done relies on the keys lane_order sorts by");

template <int TIER>
__global__ void __launch_bounds__(64, TIER == 2 ? T2_OCC : 1)
deflate_exact_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                     const uint32_t* __restrict__ in_len, uint32_t n, uint8_t* __restrict__ out,
                     const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ out_cap,
                     uint32_t* __restrict__ out_len, int32_t* __restrict__ status, const uint32_t* __restrict__ mask_key,
                     Cfg c, uint8_t* __restrict__ ws, size_t ws_per_wave, const uint32_t* __restrict__ order,
                     uint32_t* __restrict__ qctr)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Trees* T = (Trees*)smem;
    constexpr size_t TREES = al16(sizeof(Trees));
    const uint32_t wsize = 1u << c.wbits;
    const Arrays<uint8_t*> A = carve<TIER>(TIER < 2 ? smem + TREES : ws + (size_t)blockIdx.x * ws_per_wave, wsize, c.hbits);
    uint8_t *win = A.win, *syms = A.syms;
    uint16_t *prv = (uint16_t*)A.prv, *hd = (uint16_t*)A.hd;
    if (TIER == 2 && t2_head_in_lds(c.hbits)) hd = (uint16_t*)(smem + TREES);   // head[] beside the trees
    const uint32_t prv_n = A.prv_n;
    // the workspace tier takes the messages longest first from a queue, so
    // the longest start at once and the waves end together; the LDS tiers
    // stride over the batch.  Each kernel leaves the other tiers' messages.
    // (One call site of the message body: two would inline it twice and
    // double the registers.)
    uint32_t next = blockIdx.x;
    for (;;) {
        uint32_t i, len;
        if constexpr (TIER == 2) {
            uint32_t k = 0;
            if (lane_id() == 0) k = atomicAdd(qctr, 1u);
            k = U(k);
            if (k >= n) break;
            i = U(order[k]);
            len = U(in_len[i]);
            if (queue_done(len, c.hbits)) break;   // every later one is shorter
        } else {
            if (next >= n) break;
            i = next;
            next += gridDim.x;
            len = in_len[i];
        }
        if (tier_of(len, c.hbits) != TIER) continue;
        uint8_t* o = out + out_off[i];
        const uint32_t cap = out_cap[i];
        const int32_t r = exact_msg(T, win, prv, hd, syms, prv_n, in + in_off[i], len, o, cap, c);
        mem_fence();
        if (r >= 0 && mask_key) {
            // client role: the payload masked on the way out (write.hpp:679-685)
            const uint32_t key = mask_key[i];
            for (uint32_t j = lane_id(); j < (uint32_t)r; j += WAVE) o[j] ^= (uint8_t)(key >> (8 * (j & 3)));
        }
        if (lane_id() == 0) {
            out_len[i] = r >= 0 ? (uint32_t)r : 0u;
            status[i] = r >= 0 ? ST_OK : ST_NEED_BUFFERS;
        }
        mem_fence();
    }
}

template <int TIER>
static hipError_t launch(const Batch& b, unsigned grid, const Cfg& c, const uint32_t* mask_key, uint8_t* ws, size_t per,
                         const uint32_t* order, uint32_t* qctr, hipStream_t stream)
{
    const size_t lds = lds_layout(sizeof(Trees), TIER, c.hbits, c.lit_bufsize).bytes;
    hipLaunchKernelGGL(deflate_exact_kernel<TIER>, dim3(grid), dim3(64), lds, stream, b.in, b.in_off, b.in_len, b.n, b.out,
                       b.out_off, b.out_cap, b.out_len, b.status, mask_key, c, ws, per, order, qctr);
    return hipGetLastError();
}

}  // namespace dx
}  // namespace bpmd

// cfg already validated (pmd_capi.hip deflate_impl)
int bpmd::deflate_exact(const Batch& b, int level, int window_bits, int mem_level, int strategy,
                        const uint32_t* mask_key, hipStream_t stream)
{
    using namespace bpmd::dx;
    const uint32_t n = b.n;
    if (n == 0) return 0;
    const Cfg c = make_cfg(level, window_bits, mem_level, strategy);
    const uint32_t cus = (uint32_t)cu_count();
    hipError_t e;
    // the LDS tiers: one workgroup per message
    if (c.hbits <= LDS_HBITS) {
        if ((e = launch<0>(b, n, c, mask_key, nullptr, 0, nullptr, nullptr, stream)) != hipSuccess) return (int)e;
        if ((e = launch<1>(b, n, c, mask_key, nullptr, 0, nullptr, nullptr, stream)) != hipSuccess) return (int)e;
    }
    // the rest: window / prev / head / symbols in a per-wave workspace,
    // taking the messages longest first from a queue
    const size_t per = ws_per_wave(c.wbits, c.hbits, c.lit_bufsize);
    uint8_t* ws = scratch_block(stream, per * t2_waves(cus), SCR_EXACT_WS);
    uint32_t* qctr = (uint32_t*)scratch_block(stream, 256, SCR_EXACT_QUEUE);
    const uint32_t* order = lane_order(b.in_len, n, stream, nullptr);
    if (!ws || !qctr) return (int)hipErrorOutOfMemory;
    if (!order || hipMemsetAsync(qctr, 0, sizeof(uint32_t), stream) != hipSuccess) return (int)hipErrorUnknown;
    return (int)launch<2>(b, t2_grid(cus, n), c, mask_key, ws, per, order, qctr, stream);
}
