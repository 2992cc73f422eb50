// pmd_frame.hip -- the byte passes either side of the codec on Beast's frame
// path:
//
//   * masking: payload byte j ^= prepared[(j + phase) % 4], prepared[i] =
//     key >> 8i (websocket/detail/mask.ipp:20-59); the key is the frame
//     header's, read little-endian (impl/stream_impl.hpp:866-870).  Masking
//     is an involution: one pass masks (write.hpp:679-685) or unmasks
//     (read.hpp:1324-1327).
//   * UTF-8 validation of text payloads (websocket/detail/utf8_checker.ipp:
//     39-315, called at read.hpp:1372-1384).  For one message fed as a
//     single write() the checker accepts exactly the well-formed UTF-8 of
//     RFC 3629 (valid(), utf8_checker.ipp:43-85: no overlongs, no
//     surrogates, nothing above U+10FFFF); a message that stops inside a
//     code point whose bytes so far are a valid prefix passes write() (the
//     fail-fast rule, :86-157) and fails finish() (:31-37).
//
// Both passes stream HBM: one wave per message, 16 bytes per lane per step,
// aligned 16-byte accesses (an aligned block holding a payload byte never
// leaves that byte's page).  The mask pass stores bytes one at a time only at
// a message's two ragged edges, so neighbouring messages are never
// read-modify-written.
//
// The fused forms -- unmasking inside inflate's input loads, masking inside
// deflate's output stores -- live in the codec kernels; bpmd_read_batch runs
// the UTF-8 pass right after inflate on the same stream (pmd_capi.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/beast_pmd.h"
#include "frame_parse.h"
#include "pmd_internal.h"
#include "utf8_unit.h"

namespace bpmd {
namespace frame {

constexpr unsigned WAVE = 64;
constexpr unsigned WPB = 4;   // waves (messages in flight) per block

// rotate right by 8*r bits: byte t of the result is byte (t + r) % 4 of k
__device__ __forceinline__ uint32_t rotr8(uint32_t k, uint32_t r) { return __builtin_amdgcn_alignbit(k, k, 8u * (r & 3u)); }

__global__ void __launch_bounds__(WAVE * WPB)
mask_kernel(uint8_t* __restrict__ data, const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
            const uint32_t* __restrict__ key, const uint8_t* __restrict__ phase, uint32_t n)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const uint32_t nb = len[m];
        if (nb == 0) continue;
        uint8_t* p = data + off[m];
        const uint32_t s = (uint32_t)((uintptr_t)p & 15u);
        uint8_t* base = p - s;
        // byte base + a is payload byte a - s: prepared[(a - s + phase) % 4],
        // so every dword of an aligned block takes the same rotation of key
        const uint32_t kw = rotr8(key[m], (phase ? phase[m] : 0u) - s);
        const uint32_t units = (s + nb + 15u) >> 4;
        for (uint32_t u = lane; u < units; u += WAVE) {
            const uint32_t b0 = u * 16;
            if (b0 >= s && b0 + 16 <= s + nb) {
                uint4 w = *(uint4*)(base + b0);
                w.x ^= kw;
                w.y ^= kw;
                w.z ^= kw;
                w.w ^= kw;
                *(uint4*)(base + b0) = w;
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 16; ++j) {
                    const uint32_t a = b0 + j;
                    if (a >= s && a < s + nb) base[a] ^= (uint8_t)(kw >> (8 * (j & 3)));
                }
            }
        }
    }
}

// text == nullptr: result[m] = verdict (0 valid, 1 incomplete, 2 invalid)
// for every message.  text != nullptr: only messages with text[m] != 0 and
// result[m] == 0 are checked, and one that is not valid gets result[m] =
// fail_status (bpmd_read_batch: result holds the inflate status, data / off /
// len describe the inflated output).
__global__ void __launch_bounds__(WAVE * WPB)
utf8_kernel(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
            uint32_t n, int32_t* __restrict__ result, const uint8_t* __restrict__ text, int32_t fail_status)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        if (text && (text[m] == 0 || result[m] != 0)) continue;
        const uint32_t nb = len[m];
        const uint8_t* p = data + off[m];
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
                utf8_unit(x, v, err, inc);
            } else {
                uint32_t v[5];
#pragma unroll
                for (int d = 0; d < 5; ++d)
                    v[d] = span_flags((int32_t)s - (int32_t)(b0 + 4 * d), (int32_t)end - (int32_t)(b0 + 4 * d));
                utf8_unit(x, v, err, inc);
            }
            if (u == 0 && nb) {   // the first byte must start a code point
                const uint32_t f = x[s >> 2] >> (8 * (s & 3));
                err = err || (f & 0xC0u) == 0x80u;
            }
        }
        const bool any_err = __any(err), any_inc = __any(inc);
        if (lane == 0) {
            const int32_t verdict = any_err ? 2 : any_inc ? 1 : 0;
            if (!text) result[m] = verdict;
            else if (verdict) result[m] = fail_status;
        }
    }
}

// Context takeover (§8(f) N3) window maintenance: move the last keep[i]
// bytes before pos[i] of connection buffer i to its front.  The caller slides
// only when pos >= 2 * keep, so source and destination never overlap.
typedef uint4 uint4_u __attribute__((aligned(1)));

__global__ void __launch_bounds__(WAVE * WPB)
slide_kernel(uint8_t* __restrict__ buf, const uint64_t* __restrict__ base, const uint32_t* __restrict__ pos,
             const uint32_t* __restrict__ keep, uint32_t n)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const uint32_t k = keep[m];
        uint8_t* dst = buf + base[m];
        const uint8_t* src = dst + pos[m] - k;
        for (uint32_t j = 16 * lane; j < k; j += 16 * WAVE) {
            if (j + 16 <= k) *(uint4_u*)(dst + j) = *(const uint4_u*)(src + j);
            else
                for (uint32_t t = j; t < k; ++t) dst[t] = src[t];
        }
    }
}


// ---------------------------------------------------------------- frames
// Send side of a message (write.hpp:463-545): the payload goes out in frames
// of at most frame_max bytes, each with its header (frame.hpp:134-175): FIN
// on the last, RSV1 and the opcode on the first (cont = 0 after), MASK and
// the frame's own key (little-endian on the wire) for a client, whose frame
// payload is then masked from the key's first byte.  One wave per message:
// lanes 0..13 write the header bytes, then 16 payload bytes per lane per step
// (a frame's 16-byte units start at frame offsets that are multiples of 4,
// so every dword of a unit takes the key as it is).
__device__ __forceinline__ uint32_t hdr_len(uint64_t len, bool masked)
{
    return (len <= 125 ? 2u : len <= 65535 ? 4u : 10u) + (masked ? 4u : 0u);
}

typedef uint4 uint4_fu __attribute__((aligned(1)));

// One frame's payload, XORed with the frame's key on the way (masking is an
// involution): 16 bytes per lane per step at frame offsets that are multiples
// of 16, so every dword takes the key as it is, then a byte tail.
__device__ __forceinline__ void copy_xor(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t key, unsigned lane)
{
    const uint32_t full = len >> 4;
    for (uint32_t u = lane; u < full; u += WAVE) {
        uint4 v = *(const uint4_fu*)(src + 16 * u);
        v.x ^= key;
        v.y ^= key;
        v.z ^= key;
        v.w ^= key;
        *(uint4_fu*)(dst + 16 * u) = v;
    }
    const uint32_t t = 16 * full + lane;
    if (t < len) dst[t] = src[t] ^ (uint8_t)(key >> (8 * (t & 3u)));
}

__global__ void __launch_bounds__(WAVE * WPB)
frame_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ in_len,
             const uint8_t* __restrict__ op, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ keys,
             const uint32_t* __restrict__ key_base, uint32_t frame_max, uint32_t n, uint8_t* __restrict__ wire,
             const uint64_t* __restrict__ wire_off)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const uint32_t nb = in_len[m];
        const uint8_t* p = in + in_off[m];
        uint8_t* w = wire + wire_off[m];
        const uint32_t frames = nb == 0 ? 1u : (nb + frame_max - 1) / frame_max;
        const bool masked = keys != nullptr;
        const uint32_t kb = masked ? key_base[m] : 0u;
        const uint32_t opc = op ? op[m] & 15u : 2u;
        const bool rsv1 = flags ? (flags[m] & 1u) != 0 : true;
        uint64_t wp = 0;
        for (uint32_t f = 0; f < frames; ++f) {
            const uint32_t a = f * frame_max, len = f + 1 < frames ? frame_max : nb - a;
            const uint32_t key = masked ? keys[kb + f] : 0u;
            // header bytes 0-7 in h0, 8-13 in h1 (frame.hpp:134-175)
            const uint32_t b0 = (f + 1 == frames ? 0x80u : 0u) | (f == 0 && rsv1 ? 0x40u : 0u) | (f == 0 ? opc : 0u);
            uint64_t h0, h1 = 0;
            uint32_t hl;
            if (len <= 125) {
                h0 = b0 | (uint64_t)((masked ? 0x80u : 0u) | len) << 8;
                hl = 2;
            } else if (len <= 65535) {
                h0 = b0 | (uint64_t)((masked ? 0x80u : 0u) | 126u) << 8 | (uint64_t)(len >> 8) << 16 |
                     (uint64_t)(len & 0xffu) << 24;
                hl = 4;
            } else {
                // 64-bit big-endian length: bytes 2..9 = 0, 0, 0, 0, len >> 24 .. len
                h0 = b0 | (uint64_t)((masked ? 0x80u : 0u) | 127u) << 8 | (uint64_t)(len >> 24) << 48 |
                     (uint64_t)((len >> 16) & 0xffu) << 56;
                h1 = (uint64_t)((len >> 8) & 0xffu) | (uint64_t)(len & 0xffu) << 8;
                hl = 10;
            }
            if (masked) {
                if (hl == 10) h1 |= (uint64_t)key << 16;
                else h0 |= (uint64_t)key << (8 * hl);
                hl += 4;
            }
            if (lane < hl) w[wp + lane] = (uint8_t)((lane < 8 ? h0 >> (8 * lane) : h1 >> (8 * (lane - 8))) & 0xffu);
            copy_xor(w + wp + hl, p + a, len, key, lane);
            wp += hl + len;
        }
    }
}

// Receive side, frame_kernel's mirror (read.hpp:1063-1283 read_some's frame
// loop over parse_fh, stream_impl.hpp:701-913): one wave per entry walks the
// frames in the entry's wire bytes.  The walk is wave-uniform: every lane
// runs the header step (frame_parse.h) on the same bytes, which are loaded
// only below the entry's wire_len.  A data frame's payload is unmasked with
// the frame's own key and appended to the entry's out slot, 16 bytes per lane
// per step at frame offsets that are multiples of 16 (so every dword takes
// the key as it is), then a byte tail; a control frame's payload goes to the
// entry's 128-byte control slot.  The walk stops at the first complete
// message, control frame, refused header or end of the buffer.
//
// Whole frames only: a frame whose header or payload the buffer cuts is left
// unconsumed, where Beast consumes the part of a data frame's payload that
// has arrived (rd_remain, read.hpp:1201-1280); the caller keeps those bytes and
// calls again once more have come.  The wire is only read; stores stay inside
// [out_off, out_off + out_cap), which the header step's buffer_overflow check
// guarantees before any byte of a frame is copied.
__global__ void __launch_bounds__(WAVE * WPB)
unframe_kernel(uint32_t role, uint32_t pmd_on, uint64_t msg_max, const uint8_t* __restrict__ wire,
               const uint64_t* __restrict__ wire_off, const uint32_t* __restrict__ wire_len, uint32_t n,
               fp::RdState* __restrict__ state, uint8_t* __restrict__ out, const uint64_t* __restrict__ out_off,
               const uint32_t* __restrict__ out_cap, uint32_t* __restrict__ out_len, uint8_t* __restrict__ op,
               uint8_t* __restrict__ compressed, uint8_t* __restrict__ event, int32_t* __restrict__ status,
               uint32_t* __restrict__ consumed, uint8_t* __restrict__ ctl, uint8_t* __restrict__ ctl_len,
               uint16_t* __restrict__ close_code)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const uint8_t* p = wire + wire_off[m];
        const uint32_t wl = wire_len[m], cap = out_cap[m];
        uint8_t* dst = out + out_off[m];
        fp::RdState st;
        if (state) st = state[m];
        else fp::reset(st);
        uint8_t* c = ctl + 128u * (uint64_t)m;
        fp::Stop s;
        fp::walk(
            p, wl, role, pmd_on != 0, msg_max, cap, st,
            [&](uint64_t at, const uint8_t* src, uint32_t len, uint32_t key) {
                copy_xor(dst + at, src, len, key, lane);
            },
            [&](const uint8_t* src, uint32_t len, uint32_t key) {
                for (uint32_t t = lane; t < len; t += WAVE) c[t] = src[t] ^ (uint8_t)(key >> (8 * (t & 3u)));
            },
            s);
        if (lane == 0) {
            out_len[m] = (uint32_t)s.msg_len;
            op[m] = (uint8_t)s.msg_op;
            compressed[m] = (uint8_t)s.msg_deflated;
            event[m] = (uint8_t)s.event;
            status[m] = s.status;
            consumed[m] = s.consumed;
            ctl_len[m] = (uint8_t)s.ctl_len;
            close_code[m] = s.close_code;
            if (state) state[m] = st;
        }
    }
}

// frame_parse.h names its outcomes without the public header
static_assert(fp::E_BAD_FRAME_PAYLOAD == BPMD_BAD_FRAME_PAYLOAD && fp::E_BUFFER_OVERFLOW == BPMD_WS_BUFFER_OVERFLOW &&
                  fp::E_MESSAGE_TOO_BIG == BPMD_WS_MESSAGE_TOO_BIG && fp::E_BAD_OPCODE == BPMD_WS_BAD_OPCODE &&
                  fp::E_BAD_DATA_FRAME == BPMD_WS_BAD_DATA_FRAME && fp::E_BAD_CONTINUATION == BPMD_WS_BAD_CONTINUATION &&
                  fp::E_BAD_RESERVED_BITS == BPMD_WS_BAD_RESERVED_BITS &&
                  fp::E_BAD_CONTROL_FRAGMENT == BPMD_WS_BAD_CONTROL_FRAGMENT &&
                  fp::E_BAD_CONTROL_SIZE == BPMD_WS_BAD_CONTROL_SIZE &&
                  fp::E_BAD_UNMASKED_FRAME == BPMD_WS_BAD_UNMASKED_FRAME &&
                  fp::E_BAD_MASKED_FRAME == BPMD_WS_BAD_MASKED_FRAME && fp::E_BAD_SIZE == BPMD_WS_BAD_SIZE &&
                  fp::E_BAD_CLOSE_CODE == BPMD_WS_BAD_CLOSE_CODE && fp::E_BAD_CLOSE_SIZE == BPMD_WS_BAD_CLOSE_SIZE &&
                  fp::E_BAD_CLOSE_PAYLOAD == BPMD_WS_BAD_CLOSE_PAYLOAD,
              "frame_parse.h and beast_pmd.h name the same websocket::error values");
static_assert(sizeof(fp::RdState) == sizeof(bpmd_rd_state), "bpmd_rd_state is RdState");
static_assert(fp::EV_NEED_MORE == BPMD_EV_NEED_MORE && fp::EV_MESSAGE == BPMD_EV_MESSAGE && fp::EV_PING == BPMD_EV_PING &&
                  fp::EV_PONG == BPMD_EV_PONG && fp::EV_CLOSE == BPMD_EV_CLOSE &&
                  fp::ROLE_SERVER == BPMD_ROLE_SERVER && fp::ROLE_CLIENT == BPMD_ROLE_CLIENT,
              "frame_parse.h and beast_pmd.h name the same events and roles");

}  // namespace frame
}  // namespace bpmd

namespace {
unsigned frame_grid(uint32_t n)
{
    const unsigned want = (n + bpmd::frame::WPB - 1) / bpmd::frame::WPB, cap = (unsigned)bpmd::cu_count() * 8u;
    return want < cap ? want : cap;
}
}  // namespace

int bpmd::launch_mask(uint8_t* data, const uint64_t* off, const uint32_t* len, uint32_t n, const uint32_t* key,
                      const uint8_t* phase, hipStream_t stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(bpmd::frame::mask_kernel, dim3(frame_grid(n)), dim3(bpmd::frame::WAVE * bpmd::frame::WPB), 0,
                       stream, data, off, len, key, phase, n);
    return (int)hipGetLastError();
}

int bpmd::launch_utf8(const uint8_t* data, const uint64_t* off, const uint32_t* len, uint32_t n, int32_t* result,
                      const uint8_t* text, int32_t fail_status, hipStream_t stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(bpmd::frame::utf8_kernel, dim3(frame_grid(n)), dim3(bpmd::frame::WAVE * bpmd::frame::WPB), 0,
                       stream, data, off, len, n, result, text, fail_status);
    return (int)hipGetLastError();
}

int bpmd::launch_slide(uint8_t* buf, const uint64_t* base, const uint32_t* pos, const uint32_t* keep, uint32_t n,
                       hipStream_t stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(bpmd::frame::slide_kernel, dim3(frame_grid(n)), dim3(bpmd::frame::WAVE * bpmd::frame::WPB), 0,
                       stream, buf, base, pos, keep, n);
    return (int)hipGetLastError();
}

int bpmd::launch_frame(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint8_t* op,
                       const uint8_t* flags, const uint32_t* keys, const uint32_t* key_base, uint32_t frame_max,
                       uint32_t n, uint8_t* wire, const uint64_t* wire_off, hipStream_t stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(bpmd::frame::frame_kernel, dim3(frame_grid(n)), dim3(bpmd::frame::WAVE * bpmd::frame::WPB), 0,
                       stream, in, in_off, in_len, op, flags, keys, key_base, frame_max, n, wire, wire_off);
    return (int)hipGetLastError();
}

int bpmd::launch_unframe(uint32_t role, uint32_t pmd_on, uint64_t msg_max, const uint8_t* wire, const uint64_t* wire_off,
                         const uint32_t* wire_len, uint32_t n, void* state, uint8_t* out, const uint64_t* out_off,
                         const uint32_t* out_cap, uint32_t* out_len, uint8_t* op, uint8_t* compressed, uint8_t* event,
                         int32_t* status, uint32_t* consumed, uint8_t* ctl, uint8_t* ctl_len, uint16_t* close_code,
                         hipStream_t stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(bpmd::frame::unframe_kernel, dim3(frame_grid(n)), dim3(bpmd::frame::WAVE * bpmd::frame::WPB), 0,
                       stream, role, pmd_on, msg_max, wire, wire_off, wire_len, n, (bpmd::fp::RdState*)state, out,
                       out_off, out_cap, out_len, op, compressed, event, status, consumed, ctl, ctl_len, close_code);
    return (int)hipGetLastError();
}
