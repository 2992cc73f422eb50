// pmd_receive_takeover.hip -- the batch receive side in one chained call for
// connections with context takeover (no_context_takeover not negotiated, which
// is Beast's default): bpmd_receive_batch's path from wire bytes to checked
// messages, with the inflater's window kept from message to message in one
// device buffer per connection, as pmd.py's TakeoverInflater keeps it -- but
// with the connection's bookkeeping (where the next message goes, when the
// window slides, how far the position advances) on the device, so nothing is
// read back.  The per-entry rules are receive_plan.h, the per-connection rules
// receive_takeover_plan.h, both shared with the CPU tests.
//
// bpmd_receive_takeover_batch enqueues, all on the caller's stream:
//   1. the frame pass         bpmd_unframe_batch's launch, unchanged;
//   2. recv_tk_place_kernel   per entry the inflater's input length, effective
//                             capacity, window, output offset and text flag;
//                             a connection whose buffer cannot take the
//                             message has its window moved to the front by
//                             the same wave; d_msg_off, d_pos after a slide;
//   3. the inflater           bpmd_inflate_takeover_batch over all n entries,
//                             from the gathered slots into the connections'
//                             buffers;
//   4. recv_tk_finish_kernel  the merged status, the UTF-8 check of text where
//                             the message lies, d_msg_len of the entries that
//                             were not inflated, the advanced d_pos.
// Place and slide are one kernel: which connections slide is known only on the
// device, and a second launch over just those would need a scan or a
// read-back.  What the steps hand each other lives in the caller's workspace,
// as in pmd_receive.hip and for its reason: the inflater takes the stream's
// launch lock itself.
//
// Both kernels are byte movers, one wave per entry, no LDS: most waves read
// their entry's plan values and go on; a sliding wave copies W bytes, 16 per
// lane per step (slide_kernel's move, pmd_frame.hip); a text entry's wave
// walks its message (utf8_fails, receive_common.h).  No wave waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/beast_pmd.h"
#include "pmd_internal.h"
#include "receive_common.h"
#include "receive_plan.h"
#include "receive_takeover_plan.h"

namespace bpmd {
namespace recv {

typedef uint4 uint4_tu __attribute__((aligned(1)));

// step 2.  Stores: the five workspace arrays and msg_off of every entry; of a
// connection that slides, the bytes [base, base + W) of its buffer (read from
// [base + pos - W, base + pos), which receive_takeover_plan.h keeps apart) and
// pos = W.
__global__ void __launch_bounds__(WAVE * WPB)
recv_tk_place_kernel(const uint8_t* __restrict__ event, const int32_t* __restrict__ status,
                     const uint8_t* __restrict__ compressed, const uint8_t* __restrict__ op,
                     const uint32_t* __restrict__ out_len, const uint32_t* __restrict__ msg_cap, uint64_t msg_max,
                     uint8_t* __restrict__ buf, const uint64_t* __restrict__ base, uint32_t slot, uint32_t W,
                     uint32_t n, uint32_t* __restrict__ pos, uint32_t* __restrict__ z_in_len,
                     uint32_t* __restrict__ z_cap, uint8_t* __restrict__ z_text, uint32_t* __restrict__ z_hist,
                     uint64_t* __restrict__ z_off, uint64_t* __restrict__ msg_off)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const uint32_t ev = event[m], comp = compressed[m];
        const int32_t st = status[m];
        const rp::Select s = rp::select(ev, st, comp, op[m], out_len[m], rtp::room(msg_cap[m], slot, W), msg_max);
        const uint32_t p0 = pos[m];
        const rtp::Place pl = rtp::place(p0, s.eff_cap, slot, W, rp::inflates(ev, st, comp));
        uint8_t* dst = buf + base[m];
        if (pl.slide) {   // wave-uniform; W is a multiple of 256
            const uint8_t* src = dst + p0 - W;
            for (uint32_t j = 16 * lane; j < W; j += 16 * WAVE) *(uint4_tu*)(dst + j) = *(const uint4_tu*)(src + j);
        }
        if (lane == 0) {
            z_in_len[m] = s.in_len;
            z_cap[m] = s.eff_cap;
            z_text[m] = (uint8_t)s.text;
            z_hist[m] = pl.hist;
            z_off[m] = msg_off[m] = base[m] + pl.new_pos;
            if (pl.slide) pos[m] = pl.new_pos;
        }
    }
}

// step 4.  zst, msg_len: the inflater's results (looked at for an inflated
// entry only).  Stores: status of an entry whose status changes, msg_len of an
// entry that was not inflated, pos of a connection that advances; out and buf
// are only read, each inside the bytes its own entry's message occupies
// (rounded out to aligned 16-byte blocks, which stay on the pages of those
// bytes).
__global__ void __launch_bounds__(WAVE * WPB)
recv_tk_finish_kernel(const uint8_t* __restrict__ event, const uint8_t* __restrict__ compressed,
                      const uint8_t* __restrict__ op, const uint8_t* __restrict__ out,
                      const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ out_len,
                      const uint8_t* __restrict__ buf, const uint64_t* __restrict__ msg_off,
                      const uint32_t* __restrict__ msg_cap, uint64_t msg_max, uint32_t slot, uint32_t W,
                      const int32_t* __restrict__ zst, uint32_t n, uint32_t* __restrict__ msg_len,
                      int32_t* __restrict__ status, uint32_t* __restrict__ pos)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const int32_t st = status[m];
        const bool z = rp::inflates(event[m], st, compressed[m]);
        const int32_t zs = z ? zst[m] : 0;
        const uint32_t zl = z ? msg_len[m] : 0u;
        const rp::Merge g = rp::merge(event[m], st, compressed[m], op[m], out_len[m],
                                      z ? rtp::room(msg_cap[m], slot, W) : 0u, msg_max, zs, zl);
        int32_t res = g.status;
        if (g.src != rp::SRC_NONE) {
            const uint8_t* p = g.src == rp::SRC_INFLATED ? buf + msg_off[m] : out + out_off[m];
            if (utf8_fails(p, g.msg_len, lane)) res = rp::E_BAD_FRAME_PAYLOAD;
        }
        if (lane == 0) {
            if (res != st) status[m] = res;
            if (!z) msg_len[m] = g.msg_len;
            const uint32_t p0 = pos[m], p1 = rtp::advance(p0, z, zs, zl);
            if (p1 != p0) pos[m] = p1;
        }
    }
}

}  // namespace recv
}  // namespace bpmd

using namespace bpmd;

// bpmd_receive_batch's workspace, then the window and the 64-bit offset arrays
extern "C" size_t bpmd_receive_takeover_work_bytes(uint32_t n)
{
    return bpmd_receive_work_bytes(n) + recv::align256((size_t)n * sizeof(uint32_t)) +
           recv::align256((size_t)n * sizeof(uint64_t));
}

// No step of this call reads anything back; with a window every entry is
// decoded by the lane kernel (inflate_plan.h), which only enqueues.
extern "C" int bpmd_receive_takeover_batch(const bpmd_cfg* cfg, int role, uint64_t msg_max, const uint8_t* d_wire,
                                           const uint64_t* d_wire_off, const uint32_t* d_wire_len, uint32_t n,
                                           bpmd_rd_state* d_state, uint8_t* d_out, const uint64_t* d_out_off,
                                           const uint32_t* d_out_cap, uint32_t* d_out_len, uint8_t* d_op,
                                           uint8_t* d_compressed, uint8_t* d_event, int32_t* d_status,
                                           uint32_t* d_consumed, uint8_t* d_ctl, uint8_t* d_ctl_len,
                                           uint16_t* d_close_code, uint8_t* d_buf, const uint64_t* d_base,
                                           uint32_t slot_bytes, uint32_t* d_pos, const uint32_t* d_msg_cap,
                                           uint64_t* d_msg_off, uint32_t* d_msg_len, void* d_work, void* stream)
{
    if (role != BPMD_ROLE_SERVER && role != BPMD_ROLE_CLIENT) return BPMD_R_INVALID_ARGUMENT;
    if (cfg && (cfg->flags & BPMD_F_RAW)) return BPMD_R_INVALID_ARGUMENT;
    // the inflater's own check of cfg, which touches no device
    int r = bpmd_inflate_batch(cfg, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
    if (r) return r;
    const uint32_t W = 1u << cfg->window_bits;
    if (slot_bytes <= 2u * W) return BPMD_R_INVALID_ARGUMENT;
    if (n == 0) return BPMD_R_OK;
    if (!d_wire || !d_wire_off || !d_wire_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_op ||
        !d_compressed || !d_event || !d_status || !d_consumed || !d_ctl || !d_ctl_len || !d_close_code || !d_buf ||
        !d_base || !d_pos || !d_msg_cap || !d_msg_off || !d_msg_len || !d_work)
        return BPMD_R_INVALID_ARGUMENT;
    r = bpmd_init();
    if (r) return r;
    const hipStream_t s = (hipStream_t)stream;
    if (launch_unframe((uint32_t)role, 1u, msg_max, d_wire, d_wire_off, d_wire_len, n, d_state, d_out, d_out_off,
                       d_out_cap, d_out_len, d_op, d_compressed, d_event, d_status, d_consumed, d_ctl, d_ctl_len,
                       d_close_code, s))
        return BPMD_R_HIP_ERROR;
    const recv::Work w = recv::carve(d_work, n);
    uint32_t* z_hist = (uint32_t*)((uint8_t*)d_work + bpmd_receive_work_bytes(n));
    uint64_t* z_off = (uint64_t*)((uint8_t*)z_hist + recv::align256((size_t)n * sizeof(uint32_t)));
    const dim3 grid(recv::wave_grid(n)), block(recv::WAVE * recv::WPB);
    hipLaunchKernelGGL(recv::recv_tk_place_kernel, grid, block, 0, s, d_event, d_status, d_compressed, d_op, d_out_len,
                       d_msg_cap, msg_max, d_buf, d_base, slot_bytes, W, n, d_pos, w.z_in_len, w.z_cap, w.z_text,
                       z_hist, z_off, d_msg_off);
    if (hipGetLastError() != hipSuccess) return BPMD_R_HIP_ERROR;
    // not under this stream's launch lock: the inflater takes it itself
    r = bpmd_inflate_takeover_batch(cfg, d_out, d_out_off, w.z_in_len, z_hist, n, d_buf, z_off, w.z_cap, d_msg_len,
                                    w.zst, stream);
    if (r) return r;
    hipLaunchKernelGGL(recv::recv_tk_finish_kernel, grid, block, 0, s, d_event, d_compressed, d_op, d_out, d_out_off,
                       d_out_len, d_buf, d_msg_off, d_msg_cap, msg_max, slot_bytes, W, w.zst, n, d_msg_len, d_status,
                       d_pos);
    return hipGetLastError() != hipSuccess ? BPMD_R_HIP_ERROR : BPMD_R_OK;
}
