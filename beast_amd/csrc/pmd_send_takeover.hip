// pmd_send_takeover.hip -- the batch send side in one chained call for
// connections with context takeover (no_context_takeover not negotiated, which
// is Beast's default): bpmd_send_batch's path from messages to packed wire
// bytes, with the deflater's history kept from message to message in one
// device buffer per connection, as pmd.py's TakeoverDeflater keeps it -- but
// with the connection's bookkeeping (begin_msg's decision, where the message
// goes, when the kept plaintext slides, how far the position advances) on the
// device, so nothing is read back.  The per-message rules are send_plan.h, the
// per-connection rules send_takeover_plan.h, both shared with the CPU tests.
//
// bpmd_send_takeover_batch enqueues, all on the caller's stream:
//   1. send_tk_place_kernel   per entry the decision, the provisional status,
//                             the deflater's input length, history and input
//                             offset; a connection whose buffer cannot take
//                             the message has its last K bytes moved to the
//                             front, and a message that is compressed is
//                             copied behind its connection's plaintext, both
//                             by the same wave; d_pos after a slide;
//   2. the deflater           bpmd_deflate_takeover_batch's work over all n
//                             entries from the connections' buffers, its
//                             chunk workspace sized by a bound on the host
//                             instead of a count read back;
//   3. send_tk_size_kernel    the status so far and each message's wire size;
//      then bpmd_send_batch's 64-bit exclusive sum and send_frame_kernel
//      (pmd_send.hip send_scan_frames), which frames a compressed message
//      from its staging slot and any other straight from the caller's input;
//   4. send_tk_finish_kernel  the advanced d_pos, from the final status.
// Place, slide and copy are one kernel: which connections slide and which
// messages are compressed is known only on the device.  What the steps hand
// each other lives in the caller's workspace, as in pmd_receive_takeover.hip
// and for its reason: the deflater and the frame step take the stream's
// launch lock themselves.
//
// The place kernel is a byte mover, one wave per entry, no LDS: 16 bytes per
// lane per step in unaligned 16-byte accesses and a byte tail (slide_kernel's
// move, pmd_frame.hip).  No wave waits for another.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/beast_pmd.h"
#include "pmd_internal.h"
#include "send_plan.h"
#include "send_takeover_plan.h"
#include "wave_util.h"

namespace bpmd {
namespace sendtk {

constexpr unsigned WAVE = 64;
constexpr unsigned WPB = 4;   // waves (entries in flight) per block

// len bytes from src to dst, which do not overlap: whole 16-byte units, one
// per lane per step, then the tail's bytes
__device__ __forceinline__ void wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t len,
                                          unsigned lane)
{
    const uint32_t full = len >> 4;
    for (uint32_t u = lane; u < full; u += WAVE) {
        uint4 v;   // unaligned 16-byte load and store
        __builtin_memcpy(&v, src + 16ull * u, 16);
        __builtin_memcpy(dst + 16ull * u, &v, 16);
    }
    const uint32_t t = 16 * full + lane;
    if (t < len) dst[t] = src[t];
}

struct Work {
    uint32_t* z_in_len;   // the deflater's input length
    uint32_t* z_hist;     // its history
    int32_t* prov;        // the status before the deflater
    uint64_t* z_off;      // d_base[i] + new_pos
};

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline Work carve(void* d_work, uint32_t n)
{
    uint8_t* p = (uint8_t*)d_work;
    const size_t a4 = align256((size_t)n * sizeof(uint32_t));
    return Work{(uint32_t*)p, (uint32_t*)(p + a4), (int32_t*)(p + 2 * a4), (uint64_t*)(p + 3 * a4)};
}

// step 1.  Stores: the four workspace arrays and compressed of every entry; of
// a connection that slides, the bytes [base, base + K) of its buffer (read
// from [base + pos - K, base + pos), which send_takeover_plan.h keeps apart)
// and pos = K; of an entry that enters the deflater, its message's bytes at
// [base + new_pos, base + new_pos + len).  The message may land on the bytes
// the slide has just read: the wave's slide loads are complete before its
// slide stores, and those come before the copy.
__global__ void __launch_bounds__(WAVE * WPB)
send_tk_place_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                     const uint32_t* __restrict__ in_len, const uint8_t* __restrict__ op,
                     const uint8_t* __restrict__ opt, uint64_t threshold, uint32_t L, uint8_t* buf,
                     const uint64_t* __restrict__ base, uint32_t slot, uint32_t n, uint32_t* __restrict__ pos,
                     uint8_t* __restrict__ compressed, uint32_t* __restrict__ z_in_len, uint32_t* __restrict__ z_hist,
                     int32_t* __restrict__ prov, uint64_t* __restrict__ z_off)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const uint32_t len = in_len[m], o = op ? op[m] : (uint32_t)sp::OP_BINARY;
        const bool c = stp::deflates(o, opt ? opt[m] != 0 : true, len, threshold);
        const int32_t st = stp::provisional(o, c, len, L);
        const bool enters = c && st == 0;
        const uint32_t p0 = pos[m] < slot ? pos[m] : slot;   // a fill never exceeds the slot
        const stp::Place pl = stp::place(p0, len, slot, stp::K, enters);
        uint8_t* dst = buf + base[m];
        if (pl.slide) {   // wave-uniform
            wave_copy(dst, dst + p0 - stp::K, stp::K, lane);
            wave_sync();
        }
        if (enters) wave_copy(dst + pl.new_pos, in + in_off[m], len, lane);
        if (lane == 0) {
            compressed[m] = c ? 1 : 0;
            z_in_len[m] = pl.z_len;
            z_hist[m] = pl.hist;
            prov[m] = st;
            z_off[m] = base[m] + pl.new_pos;
            if (pl.slide) pos[m] = pl.new_pos;
        }
    }
}

// step 3: the status so far, by precedence the provisional one, then the
// deflater's (status holds it), and the wire size: 0 for an idle or refused
// entry, which send_frame_kernel then leaves out
__global__ void __launch_bounds__(256)
send_tk_size_kernel(const uint32_t* __restrict__ in_len, const uint32_t* __restrict__ z_len,
                    const uint8_t* __restrict__ op, const uint8_t* __restrict__ compressed,
                    const int32_t* __restrict__ prov, uint32_t masked, uint32_t frag, uint32_t frame_max, uint32_t n,
                    int32_t* __restrict__ status, uint64_t* __restrict__ sizes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool c = compressed[i] != 0;
    const uint32_t o = op ? op[i] : (uint32_t)sp::OP_BINARY;
    const int32_t st = stp::merge(prov[i], c && prov[i] == 0, status[i]);
    const uint32_t len = c ? z_len[i] : in_len[i];
    sizes[i] = st || o == stp::OP_IDLE ? 0 : sp::wire_size(sp::split(len, frame_max, c, frag != 0), masked != 0);
    status[i] = st;
}

// step 4: a message joins its connection's history iff its frames went out
__global__ void __launch_bounds__(256)
send_tk_finish_kernel(const uint32_t* __restrict__ z_in_len, const uint8_t* __restrict__ compressed,
                      const int32_t* __restrict__ prov, const int32_t* __restrict__ status, uint32_t n,
                      uint32_t* __restrict__ pos)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p0 = pos[i], p1 = stp::advance(p0, z_in_len[i], compressed[i] != 0 && prov[i] == 0, status[i]);
    if (p1 != p0) pos[i] = p1;
}

static_assert(stp::E_MESSAGE_TOO_BIG == BPMD_WS_MESSAGE_TOO_BIG, "send_takeover_plan.h and beast_pmd.h name the same value");
static_assert(stp::K % 16 == 0, "a slide is whole 16-byte units");

}  // namespace sendtk
}  // namespace bpmd

using namespace bpmd;

// the deflater's input length and history, the provisional status, then the
// 64-bit input offset
extern "C" size_t bpmd_send_takeover_work_bytes(uint32_t n)
{
    return 3 * sendtk::align256((size_t)n * sizeof(uint32_t)) + sendtk::align256((size_t)n * sizeof(uint64_t));
}

// No step of this call reads anything back: the deflater gets the bound
// n * ceil(L / 4096) in place of its chunk count.
extern "C" int bpmd_send_takeover_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                                        const uint32_t* d_in_len, uint32_t n, int role, uint64_t threshold, int frag,
                                        uint32_t frame_max, uint32_t max_len, const uint8_t* d_op,
                                        const uint8_t* d_opt, uint8_t* d_buf, const uint64_t* d_base,
                                        uint32_t slot_bytes, uint32_t* d_pos, uint8_t* d_z, const uint64_t* d_z_off,
                                        const uint32_t* d_z_cap, uint32_t* d_z_len, const uint32_t* d_keys,
                                        const uint32_t* d_key_base, uint8_t* d_wire, uint64_t wire_cap,
                                        uint64_t* d_wire_off, uint32_t* d_wire_len, uint8_t* d_compressed,
                                        int32_t* d_status, uint64_t* d_total, void* d_work, void* stream)
{
    if (frame_max == 0 || (role != BPMD_ROLE_SERVER && role != BPMD_ROLE_CLIENT) || n > (uint32_t)INT_MAX)
        return BPMD_R_INVALID_ARGUMENT;
    if (!cfg || (cfg->flags & (BPMD_F_EXACT | BPMD_F_RAW))) return BPMD_R_INVALID_ARGUMENT;
    // the deflater's own check of cfg, which touches no device
    int r = bpmd_deflate_batch(cfg, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
    if (r) return r;
    if (slot_bytes <= 2u * stp::K || max_len == 0) return BPMD_R_INVALID_ARGUMENT;
    const uint32_t L = stp::room(max_len, slot_bytes, stp::K);
    const uint64_t bound = dfl::chunk_bound(n, L);   // none reaches the deflater with more than L bytes
    if (bound > 0xFFFFFFFFull) return BPMD_R_INVALID_ARGUMENT;
    if (n == 0) return BPMD_R_OK;
    if (!d_in || !d_in_off || !d_in_len || !d_buf || !d_base || !d_pos || !d_z || !d_z_off || !d_z_cap || !d_z_len ||
        (!d_wire && wire_cap) || !d_wire_off || !d_wire_len || !d_compressed || !d_status || !d_total || !d_work)
        return BPMD_R_INVALID_ARGUMENT;
    if (role == BPMD_ROLE_CLIENT && (!d_keys || !d_key_base)) return BPMD_R_INVALID_ARGUMENT;
    r = bpmd_init();
    if (r) return r;
    const hipStream_t s = (hipStream_t)stream;
    const bool masked = role == BPMD_ROLE_CLIENT;
    const sendtk::Work w = sendtk::carve(d_work, n);
    const unsigned want = (n + sendtk::WPB - 1) / sendtk::WPB, cap = (unsigned)cu_count() * 8u;
    hipLaunchKernelGGL(sendtk::send_tk_place_kernel, dim3(want < cap ? want : cap), dim3(sendtk::WAVE * sendtk::WPB), 0, s,
                       d_in, d_in_off, d_in_len, d_op, d_opt, threshold, L, d_buf, d_base, slot_bytes, n, d_pos,
                       d_compressed, w.z_in_len, w.z_hist, w.prov, w.z_off);
    if (hipGetLastError() != hipSuccess) return BPMD_R_HIP_ERROR;
    // not under this stream's launch lock: the deflater takes it itself
    const Batch b{d_buf, w.z_off, w.z_in_len, n, d_z, d_z_off, d_z_cap, d_z_len, d_status};
    DeflateOpts zo;
    zo.hist_len = w.z_hist, zo.chunks = {dfl::ChunkSource::BOUND, bound};
    r = deflate_takeover_bounded(cfg, b, zo, s);
    if (r) return r;
    const dim3 egrid((n + 255u) / 256u), eblock(256);
    const SendFrames a{d_in, d_in_off, d_in_len, n, masked, frag != 0, frame_max, d_op, d_z, d_z_off, d_z_len,
                       masked ? d_keys : nullptr, d_key_base, d_wire, wire_cap, d_wire_off, d_wire_len, d_compressed,
                       d_status, d_total};
    r = send_scan_frames(
        a,
        [&](uint64_t* sizes) {
            hipLaunchKernelGGL(sendtk::send_tk_size_kernel, egrid, eblock, 0, s, d_in_len, d_z_len, d_op, d_compressed,
                               w.prov, masked ? 1u : 0u, frag ? 1u : 0u, frame_max, n, d_status, sizes);
        },
        s);
    if (r) return r;
    hipLaunchKernelGGL(sendtk::send_tk_finish_kernel, egrid, eblock, 0, s, w.z_in_len, d_compressed, w.prov, d_status, n,
                       d_pos);
    return hipGetLastError() != hipSuccess ? BPMD_R_HIP_ERROR : BPMD_R_OK;
}
