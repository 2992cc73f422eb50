// utf8_unit.h -- the unit step of the UTF-8 check (websocket/detail/
// utf8_checker.ipp:39-315 restated over 16-byte units): what utf8_kernel
// (pmd_frame.hip) and utf8_fails (receive_common.h, for the finish kernels of
// pmd_receive.hip and pmd_receive_takeover.hip) run per lane on 16 bytes and
// the 4 bytes after them.  The callers load the bytes and say which of them
// lie inside the message.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bpmd {
namespace frame {

constexpr uint32_t H = 0x80808080u;

// byte flags (0x80 per byte) of the bytes [lo, hi) of a dword, lo/hi in bytes
// relative to the dword and clamped to 0..4
__device__ __forceinline__ uint32_t span_flags(int32_t lo, int32_t hi)
{
    lo = lo < 0 ? 0 : lo > 4 ? 4 : lo;
    hi = hi < 0 ? 0 : hi > 4 ? 4 : hi;
    if (hi <= lo) return 0u;
    const uint64_t m = (1ull << (8 * hi)) - (1ull << (8 * lo));
    return (uint32_t)m & H;
}

// the dword starting k bytes later (k = 1..3) in the byte stream lo, hi
__device__ __forceinline__ uint32_t sh(uint32_t lo, uint32_t hi, uint32_t k) { return __builtin_amdgcn_alignbit(hi, lo, 8u * k); }

// Verdict bits of one 16-byte unit: x[0..3] the unit, x[4] the next unit's
// first dword; v[0..4] the same bytes' in-message flags.  Each byte inside
// the message that starts a code point is checked against the bytes after it
// (at most 4 further on, hence x[4]):
//   invalid lead (C0, C1, F5..FF), a missing continuation, a continuation too
//   many (the byte after a complete code point), the second-byte ranges of
//   E0 / ED / F0 / F4 (overlong, surrogate, > U+10FFFF).
// A continuation byte that no lead claims is always the byte right after a
// complete code point (caught there) or the message's first byte (checked by
// the caller).  Bytes past the message count as "continuation still to come"
// for the missing-continuation test, which reports them as incomplete.
__device__ __forceinline__ void utf8_unit(const uint32_t (&x)[5], const uint32_t (&v)[5], bool& err, bool& inc)
{
    uint32_t Cx[5], Cy[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        const uint32_t c = x[d] & ~(x[d] << 1) & H;   // 10xxxxxx
        Cx[d] = c | (~v[d] & H);
        Cy[d] = c & v[d];
    }
    uint32_t e = 0, ic = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t b = x[d];
        const uint32_t g0 = b & (b << 1) & H;   // 11xxxxxx
        const uint32_t g1 = g0 & (b << 2);      // 111xxxxx
        const uint32_t g2 = g1 & (b << 3);      // 1111xxxx
        const uint32_t g3 = g2 & (b << 4);      // 11111xxx
        const uint32_t a1 = ~b & H;             // 0xxxxxxx
        const uint32_t l2 = g0 & ~g1, l3 = g1 & ~g2, l4 = g2 & ~g3;
        const uint32_t lo4 = b & 0x0F0F0F0Fu, lo3 = b & 0x07070707u;
        const uint32_t z1e = ~((b & 0x1E1E1E1Eu) + 0x7F7F7F7Fu) & H;   // C0 / C1
        const uint32_t ge5 = (lo3 + 0x7B7B7B7Bu) & H;                   // F5..F7
        const uint32_t bad = g3 | (l2 & z1e) | (l4 & ge5);
        const uint32_t e0 = l3 & ~(lo4 + 0x7F7F7F7Fu);
        const uint32_t ed = l3 & ~((lo4 ^ 0x0D0D0D0Du) + 0x7F7F7F7Fu);
        const uint32_t f0 = l4 & ~(lo3 + 0x7F7F7F7Fu);
        const uint32_t f4 = l4 & ~((lo3 ^ 0x04040404u) + 0x7F7F7F7Fu);
        const uint32_t y = sh(x[d], x[d + 1], 1);                              // second bytes
        const uint32_t y20 = (y << 2) & H, y30 = ((y << 2) | (y << 3)) & H;   // >= A0, >= 90 for 10xxxxxx
        const uint32_t range = ((e0 & ~y20) | (ed & y20) | (f0 & ~y30) | (f4 & y30)) & sh(Cy[d], Cy[d + 1], 1);
        const uint32_t n2 = l2 | l3 | l4, n3 = l3 | l4;
        const uint32_t c1 = sh(Cx[d], Cx[d + 1], 1), c2 = sh(Cx[d], Cx[d + 1], 2), c3 = sh(Cx[d], Cx[d + 1], 3);
        const uint32_t t1 = sh(Cy[d], Cy[d + 1], 1), t2 = sh(Cy[d], Cy[d + 1], 2), t3 = sh(Cy[d], Cy[d + 1], 3);
        const uint32_t t4 = Cy[d + 1];
        const uint32_t ed_ =
            bad | (n2 & ~c1) | (n3 & ~c2) | (l4 & ~c3) | (a1 & t1) | (l2 & t2) | (l3 & t3) | (l4 & t4) | range;
        e |= ed_ & v[d];
        const uint32_t v1 = sh(v[d], v[d + 1], 1), v2 = sh(v[d], v[d + 1], 2), v3 = sh(v[d], v[d + 1], 3);
        ic |= ((n2 & ~v1) | (n3 & ~v2) | (l4 & ~v3)) & v[d];
    }
    err = err || e != 0;
    inc = inc || ic != 0;
}

}  // namespace frame
}  // namespace bpmd
