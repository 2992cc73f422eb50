// pmd_send.hip -- the batch send side: from messages to packed wire bytes in
// one chained call, as write_some sends a message (websocket/impl/write.hpp:
// 625-831) after begin_msg decided whether to compress it (websocket/impl/
// stream_impl.hpp:225-252), and the control frames of write_ping / write_close
// (stream_impl.hpp:915-996).  The plan -- decision, frame split, header bytes,
// wire offsets and sizes -- is send_plan.h, shared with the CPU tests.
//
// bpmd_send_batch enqueues, all on the caller's stream and with nothing read
// back by any step of its own:
//   1. send_select_kernel   the decision, and the deflater's length array
//                           (len when compressing, 0 otherwise);
//   2. the deflater         bpmd_deflate_batch over all n messages;
//   3. send_size_kernel     each message's wire size and status;
//   4. a 64-bit exclusive sum (hipCUB) of the sizes: the packed offsets;
//   5. send_frame_kernel    headers and payloads, masked in client role.
// Steps 4 and 5 behind a caller's own size kernel are send_scan_frames, which
// bpmd_send_takeover_batch (pmd_send_takeover.hip) shares.
// The deflater's length array lives in the caller's d_wire_len until step 3
// overwrites it, so nothing of a call lives in the stream's shared scratch
// while the stream's launch lock is released around step 2 (bpmd_deflate_batch
// takes that lock itself).
//
// The frame kernel follows frame_kernel's data path (pmd_frame.hip): 16 bytes
// per lane per step in unaligned 16-byte accesses, the key applied per dword
// (frame units start at multiples of 4, so every dword takes the key as it
// is), then a byte tail; the source is picked per message, so an uncompressed
// message is framed straight from the caller's input.  One wave per message:
// with send_plan.h's closed-form frame offsets the four waves of a block could
// take alternate frames of one long message, and that was measured (wave w
// taking frame f of the block's message j when (f + j) % 4 == w): on 16 Ki
// messages of 64 KiB in 4 KiB frames it changed nothing (0.594 ms either way;
// the batch already fills every CU), and on 64 Ki one-frame messages it cost
// 0.070 -> 0.090 ms, every wave reading four messages' plans
// (profiles/send_vs_frame.log).  No wave waits for another.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <limits.h>
#include <stdint.h>

#include <mutex>

#include "../../include/beast_pmd.h"
#include "pmd_internal.h"
#include "send_plan.h"

namespace bpmd {
namespace send {

constexpr unsigned WAVE = 64;
constexpr unsigned WPB = 4;   // waves (messages in flight) per block

typedef uint4 uint4_u __attribute__((aligned(1)));

// One frame's payload XORed with its key: two 16-byte units per lane in
// flight, then single units, then a byte tail.
__device__ __forceinline__ void copy_xor(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t len,
                                         uint32_t key, unsigned lane)
{
    const uint32_t full = len >> 4;
    uint32_t u = lane;
    for (; u + WAVE < full; u += 2 * WAVE) {
        uint4 a = *(const uint4_u*)(src + 16ull * u);
        uint4 b = *(const uint4_u*)(src + 16ull * (u + WAVE));
        a.x ^= key, a.y ^= key, a.z ^= key, a.w ^= key;
        b.x ^= key, b.y ^= key, b.z ^= key, b.w ^= key;
        *(uint4_u*)(dst + 16ull * u) = a;
        *(uint4_u*)(dst + 16ull * (u + WAVE)) = b;
    }
    if (u < full) {
        uint4 a = *(const uint4_u*)(src + 16ull * u);
        a.x ^= key, a.y ^= key, a.z ^= key, a.w ^= key;
        *(uint4_u*)(dst + 16ull * u) = a;
    }
    const uint32_t t = 16 * full + lane;
    if (t < len) dst[t] = src[t] ^ (uint8_t)(key >> (8 * (t & 3u)));
}

// step 1: begin_msg's rule per message
__global__ void __launch_bounds__(256)
send_select_kernel(const uint32_t* __restrict__ in_len, const uint8_t* __restrict__ opt, uint64_t threshold, uint32_t n,
                   uint8_t* __restrict__ compressed, uint32_t* __restrict__ z_in_len)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t len = in_len[i];
    const bool c = sp::compress(true, opt ? opt[i] != 0 : true, len, threshold);
    compressed[i] = c ? 1 : 0;
    z_in_len[i] = c ? len : 0u;
}

// step 3: wire size (0 for a message that is not sent) and the status so far.
// have_z == 0: permessage-deflate is off, nothing was deflated and the
// decision is written here.
__global__ void __launch_bounds__(256)
send_size_kernel(const uint32_t* __restrict__ in_len, const uint32_t* __restrict__ z_len, const uint8_t* __restrict__ op,
                 uint8_t* __restrict__ compressed, uint32_t have_z, uint32_t masked, uint32_t frag, uint32_t frame_max,
                 uint32_t n, int32_t* __restrict__ status, uint64_t* __restrict__ sizes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool c = false;
    if (have_z) c = compressed[i] != 0;
    else compressed[i] = 0;
    const uint32_t o = op ? op[i] : (uint32_t)sp::OP_BINARY;
    int32_t st = 0;
    if (o != sp::OP_TEXT && o != sp::OP_BINARY) st = sp::E_BAD_OPCODE;
    else if (c) st = status[i];   // the deflater's
    const uint32_t len = c ? z_len[i] : in_len[i];
    sizes[i] = st ? 0 : sp::wire_size(sp::split(len, frame_max, c, frag != 0), masked != 0);
    status[i] = st;
}

// step 5: one wave per message, as frame_kernel; each frame is placed by the
// closed form.  A size of 0 marks a message that is not sent (every frame has
// at least 2 bytes); a message that does not fit [0, wire_cap) at its packed
// offset, or whose size does not fit d_wire_len's 32 bits, is refused and none
// of its bytes are written.  first / fin (NULL = all 1): an entry that is one
// piece of a message opens it only with first[m] and ends it only with fin[m].
__global__ void __launch_bounds__(WAVE * WPB)
send_frame_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                  const uint32_t* __restrict__ in_len, const uint8_t* __restrict__ z,
                  const uint64_t* __restrict__ z_off, const uint32_t* __restrict__ z_len,
                  const uint8_t* __restrict__ op, const uint8_t* __restrict__ compressed,
                  const uint32_t* __restrict__ keys, const uint32_t* __restrict__ key_base, uint32_t frag,
                  uint32_t frame_max, uint32_t n, const uint64_t* __restrict__ sizes, uint8_t* __restrict__ wire,
                  uint64_t wire_cap, const uint64_t* __restrict__ wire_off, uint32_t* __restrict__ wire_len,
                  int32_t* __restrict__ status, uint64_t* __restrict__ total, const uint8_t* __restrict__ first,
                  const uint8_t* __restrict__ fin)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    const bool masked = keys != nullptr;
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const uint64_t size = sizes[m], off = wire_off[m];
        const bool fits = size != 0 && size <= 0xffffffffull && off <= wire_cap && size <= wire_cap - off;
        if (lane == 0) {
            wire_len[m] = fits ? (uint32_t)size : 0u;
            if (size != 0 && !fits) status[m] = sp::E_BUFFER_OVERFLOW;
            if (m == n - 1) *total = off + size;
        }
        if (!fits) continue;
        const bool c = compressed[m] != 0;
        const uint8_t* src = c ? z + z_off[m] : in + in_off[m];
        const sp::Split s = sp::split(c ? z_len[m] : in_len[m], frame_max, c, frag != 0);
        const uint32_t o = op ? op[m] : (uint32_t)sp::OP_BINARY;
        const uint32_t kb = masked ? key_base[m] : 0u;
        const bool opens = first ? first[m] != 0 : true, ends = fin ? fin[m] != 0 : true;
        uint8_t* dst = wire + off;
        for (uint64_t f = 0; f < s.frames; ++f) {
            const uint32_t len = (uint32_t)sp::frame_len(s, f);
            const uint32_t key = masked ? keys[kb + f] : 0u;
            uint64_t h0, h1;
            const uint32_t hl = sp::header(len, f == 0 && opens, f + 1 == s.frames && ends, c, o, masked, key, h0, h1);
            uint8_t* p = dst + sp::frame_off(s, masked, f);
            if (lane < hl) p[lane] = sp::header_byte(h0, h1, lane);
            copy_xor(p + hl, src + sp::frame_src(s, f), len, key, lane);
        }
    }
}

// write_ping / write_close: one wave per entry, a byte per lane per step (a
// control frame has at most 131 bytes)
__global__ void __launch_bounds__(WAVE * WPB)
control_kernel(const uint8_t* __restrict__ op, const uint8_t* __restrict__ ctl, const uint8_t* __restrict__ ctl_len,
               const uint16_t* __restrict__ close_code, const uint32_t* __restrict__ key, uint32_t n,
               uint8_t* __restrict__ wire, uint32_t* __restrict__ wire_len, int32_t* __restrict__ status)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const uint32_t o = op[m], sl = ctl_len ? ctl_len[m] : 0u, code = close_code ? close_code[m] : 0u;
        const bool masked = key != nullptr;
        const uint32_t k = masked ? key[m] : 0u;
        uint32_t pl;
        const int32_t st = sp::control_plan(o, sl, code, pl);
        const uint32_t size = st ? 0u : sp::control_size(pl, masked);
        const uint8_t* slot = ctl + (uint64_t)sp::CTL_SLOT * m;
        uint8_t* dst = wire + (uint64_t)sp::CTL_WIRE * m;
        for (uint32_t t = lane; t < size; t += WAVE) dst[t] = sp::control_byte(t, o, pl, code, slot, masked, k);
        if (lane == 0) {
            wire_len[m] = size;
            status[m] = st;
        }
    }
}

static_assert(sp::E_NEED_BUFFERS == BPMD_NEED_BUFFERS && sp::E_BUFFER_OVERFLOW == BPMD_WS_BUFFER_OVERFLOW &&
                  sp::E_BAD_OPCODE == BPMD_WS_BAD_OPCODE && sp::E_BAD_CONTROL_SIZE == BPMD_WS_BAD_CONTROL_SIZE &&
                  sp::ROLE_SERVER == BPMD_ROLE_SERVER && sp::ROLE_CLIENT == BPMD_ROLE_CLIENT,
              "send_plan.h and beast_pmd.h name the same values");
static_assert(sp::CTL_MAX + 6 <= sp::CTL_WIRE, "a control frame fits its wire slot");

}  // namespace send
}  // namespace bpmd

using namespace bpmd;

namespace {
unsigned elem_grid(uint32_t n) { return (n + 255u) / 256u; }
unsigned wave_grid(uint32_t n)
{
    const unsigned want = (n + send::WPB - 1) / send::WPB, cap = (unsigned)cu_count() * 8u;
    return want < cap ? want : cap;
}
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace

extern "C" uint64_t bpmd_send_frame_bound(uint64_t len, uint32_t frame_max, int may_compress, int frag)
{
    return frame_max ? sp::frame_bound(len, frame_max, may_compress != 0, frag != 0) : 0;
}

extern "C" uint64_t bpmd_send_wire_bound(uint64_t len, uint32_t frame_max, int masked, int may_compress, int frag)
{
    return frame_max ? sp::wire_bound(len, frame_max, masked != 0, may_compress != 0, frag != 0) : 0;
}

// Steps 3-5 (the framing part) on their own: bpmd_send_batch after its
// deflate step, with the decision already in d_compressed and the deflate
// statuses in d_status.  scripts/bench_send.py times it beside
// bpmd_frame_batch.
extern "C" int bpmd_internal_send_frames(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                         uint32_t n, int role, int have_z, int frag, uint32_t frame_max,
                                         const uint8_t* d_op, const uint8_t* d_z, const uint64_t* d_z_off,
                                         const uint32_t* d_z_len, const uint32_t* d_keys, const uint32_t* d_key_base,
                                         uint8_t* d_wire, uint64_t wire_cap, uint64_t* d_wire_off,
                                         uint32_t* d_wire_len, uint8_t* d_compressed, int32_t* d_status,
                                         uint64_t* d_total, void* stream)
{
    const bool masked = role == BPMD_ROLE_CLIENT;
    const SendFrames a{d_in, d_in_off, d_in_len, n, masked, frag != 0, frame_max, d_op, d_z, d_z_off, d_z_len,
                       masked ? d_keys : nullptr, d_key_base, d_wire, wire_cap, d_wire_off, d_wire_len, d_compressed,
                       d_status, d_total};
    const hipStream_t s = (hipStream_t)stream;
    return send_scan_frames(
        a,
        [&](uint64_t* sizes) {
            hipLaunchKernelGGL(send::send_size_kernel, dim3(elem_grid(n)), dim3(256), 0, s, d_in_len, d_z_len, d_op,
                               d_compressed, have_z ? 1u : 0u, masked ? 1u : 0u, frag ? 1u : 0u, frame_max, n, d_status,
                               sizes);
        },
        s);
}

int bpmd::send_scan_frames(const SendFrames& a, const std::function<void(uint64_t* sizes)>& launch_size, hipStream_t s)
{
    const uint32_t n = a.n;
    std::mutex* mu = stream_mutex(s);
    if (!mu) return BPMD_R_HIP_ERROR;
    std::lock_guard<std::mutex> launch(*mu);
    size_t cub_bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n, s) !=
        hipSuccess)
        return BPMD_R_HIP_ERROR;
    const size_t o_cub = align256((size_t)n * sizeof(uint64_t));
    uint8_t* ws = scratch_block(s, o_cub + align256(cub_bytes ? cub_bytes : 1), SCR_SEND);
    if (!ws) return BPMD_R_HIP_ERROR;
    uint64_t* sizes = (uint64_t*)ws;
    launch_size(sizes);
    if (hipGetLastError() != hipSuccess) return BPMD_R_HIP_ERROR;
    if (hipcub::DeviceScan::ExclusiveSum(ws + o_cub, cub_bytes, (const uint64_t*)sizes, a.wire_off, (int)n, s) !=
        hipSuccess)
        return BPMD_R_HIP_ERROR;
    hipLaunchKernelGGL(send::send_frame_kernel, dim3(wave_grid(n)), dim3(send::WAVE * send::WPB), 0, s, a.in, a.in_off,
                       a.in_len, a.z, a.z_off, a.z_len, a.op, a.compressed, a.keys, a.key_base, a.frag ? 1u : 0u,
                       a.frame_max, n, sizes, a.wire, a.wire_cap, a.wire_off, a.wire_len, a.status, a.total, a.first,
                       a.fin);
    return hipGetLastError() != hipSuccess ? BPMD_R_HIP_ERROR : BPMD_R_OK;
}

// Inherited from bpmd_deflate_batch: with a message longer than 4 KiB among
// those that are compressed, the deflater reads its chunk count back and so
// returns only once the work queued on the stream before it has run
// (pmd_deflate.hip).  No step added here reads anything back.
extern "C" int bpmd_send_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                               const uint32_t* d_in_len, uint32_t n, int role, int pmd_on, uint64_t threshold, int frag,
                               uint32_t frame_max, const uint8_t* d_op, const uint8_t* d_opt, uint8_t* d_z,
                               const uint64_t* d_z_off, const uint32_t* d_z_cap, uint32_t* d_z_len,
                               const uint32_t* d_keys, const uint32_t* d_key_base, uint8_t* d_wire, uint64_t wire_cap,
                               uint64_t* d_wire_off, uint32_t* d_wire_len, uint8_t* d_compressed, int32_t* d_status,
                               uint64_t* d_total, void* stream)
{
    if (frame_max == 0 || (role != BPMD_ROLE_SERVER && role != BPMD_ROLE_CLIENT) || n > (uint32_t)INT_MAX)
        return BPMD_R_INVALID_ARGUMENT;
    if (pmd_on) {   // the deflater's own check of cfg, which touches no device
        const int r = bpmd_deflate_batch(cfg, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         stream);
        if (r) return r;
    }
    if (n == 0) return BPMD_R_OK;
    if (!d_in || !d_in_off || !d_in_len || (!d_wire && wire_cap) || !d_wire_off || !d_wire_len || !d_compressed ||
        !d_status || !d_total)
        return BPMD_R_INVALID_ARGUMENT;
    if (pmd_on && (!d_z || !d_z_off || !d_z_cap || !d_z_len)) return BPMD_R_INVALID_ARGUMENT;
    if (role == BPMD_ROLE_CLIENT && (!d_keys || !d_key_base)) return BPMD_R_INVALID_ARGUMENT;
    int r = bpmd_init();
    if (r) return r;
    const hipStream_t s = (hipStream_t)stream;
    if (pmd_on) {
        hipLaunchKernelGGL(send::send_select_kernel, dim3(elem_grid(n)), dim3(256), 0, s, d_in_len, d_opt, threshold, n,
                           d_compressed, d_wire_len);
        if (hipGetLastError() != hipSuccess) return BPMD_R_HIP_ERROR;
        // not under this stream's launch lock: the deflater takes it itself
        r = bpmd_deflate_batch(cfg, d_in, d_in_off, d_wire_len, n, d_z, d_z_off, d_z_cap, d_z_len, d_status, stream);
        if (r) return r;
    }
    return bpmd_internal_send_frames(d_in, d_in_off, d_in_len, n, role, pmd_on, frag, frame_max, d_op, d_z, d_z_off,
                                     d_z_len, d_keys, d_key_base, d_wire, wire_cap, d_wire_off, d_wire_len,
                                     d_compressed, d_status, d_total, stream);
}

extern "C" int bpmd_control_batch(const uint8_t* d_op, const uint8_t* d_ctl, const uint8_t* d_ctl_len,
                                  const uint16_t* d_close_code, const uint32_t* d_key, uint32_t n, uint8_t* d_wire,
                                  uint32_t* d_wire_len, int32_t* d_status, void* stream)
{
    if (n == 0) return BPMD_R_OK;
    if (!d_op || !d_ctl || !d_ctl_len || !d_close_code || !d_wire || !d_wire_len || !d_status)
        return BPMD_R_INVALID_ARGUMENT;
    int r = bpmd_init();
    if (r) return r;
    hipLaunchKernelGGL(send::control_kernel, dim3(wave_grid(n)), dim3(send::WAVE * send::WPB), 0, (hipStream_t)stream,
                       d_op, d_ctl, d_ctl_len, d_close_code, d_key, n, d_wire, d_wire_len, d_status);
    return hipGetLastError() != hipSuccess ? BPMD_R_HIP_ERROR : BPMD_R_OK;
}
