// receive_common.h -- what the two chained receive calls share
// (bpmd_receive_batch, pmd_receive.hip; bpmd_receive_takeover_batch,
// pmd_receive_takeover.hip): the wave geometry of their per-entry kernels, the
// UTF-8 walk over one message, the grid of a one-wave-per-entry kernel and the
// layout of the caller's workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pmd_internal.h"
#include "utf8_unit.h"

namespace bpmd {
namespace recv {

constexpr unsigned WAVE = 64;
constexpr unsigned WPB = 4;   // waves (entries in flight) per block

// utf8_kernel's walk over one message (pmd_frame.hip), the verdict reduced to
// valid or not: true when the nb bytes at p are not well-formed UTF-8 or stop
// inside a code point.  Wave-uniform result.
__device__ __forceinline__ bool utf8_fails(const uint8_t* __restrict__ p, uint32_t nb, unsigned lane)
{
    using frame::H;
    if (nb == 0) return false;
    const uint32_t s = (uint32_t)((uintptr_t)p & 15u);
    const uint8_t* base = p - s;
    const uint32_t units = (s + nb + 15u) >> 4, end = s + nb;
    bool err = false, inc = false;
    for (uint32_t u0 = 0; u0 < units; u0 += WAVE) {
        const uint32_t u = u0 + lane, b0 = u * 16;
        uint4 w = make_uint4(0, 0, 0, 0);
        if (u < units) w = *(const uint4*)(base + b0);
        uint32_t nxt = __shfl_down(w.x, 1);
        if (lane == WAVE - 1) nxt = (b0 + 16 < end) ? *(const uint32_t*)(base + b0 + 16) : 0u;
        if (u >= units) continue;
        if (((w.x | w.y | w.z | w.w | nxt) & H) == 0) continue;   // all ASCII: nothing to reject
        const uint32_t x[5] = {w.x, w.y, w.z, w.w, nxt};
        if (b0 >= s && b0 + 20 <= end) {   // unit and look-ahead inside the message
            const uint32_t v[5] = {H, H, H, H, H};
            frame::utf8_unit(x, v, err, inc);
        } else {
            uint32_t v[5];
#pragma unroll
            for (int d = 0; d < 5; ++d)
                v[d] = frame::span_flags((int32_t)s - (int32_t)(b0 + 4 * d), (int32_t)end - (int32_t)(b0 + 4 * d));
            frame::utf8_unit(x, v, err, inc);
        }
        if (u == 0) {   // the first byte must start a code point
            const uint32_t f = x[s >> 2] >> (8 * (s & 3));
            err = err || (f & 0xC0u) == 0x80u;
        }
    }
    return __any(err || inc) != 0;
}

// one wave per entry, grid-strided beyond 8 blocks per compute unit
inline unsigned wave_grid(uint32_t n)
{
    const unsigned want = (n + WPB - 1) / WPB, cap = (unsigned)cu_count() * 8u;
    return want < cap ? want : cap;
}
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the workspace: three 32-bit arrays and a byte array, each from a 256-byte boundary
struct Work {
    uint32_t *z_in_len, *z_cap;
    int32_t* zst;
    uint8_t* z_text;
};
inline Work carve(void* d_work, uint32_t n)
{
    uint8_t* p = (uint8_t*)d_work;
    const size_t a = align256((size_t)n * sizeof(uint32_t));
    return Work{(uint32_t*)p, (uint32_t*)(p + a), (int32_t*)(p + 2 * a), p + 3 * a};
}

}  // namespace recv
}  // namespace bpmd
