// pmd_receive.hip -- the batch receive side: from wire bytes to checked
// messages in one chained call, as read_some delivers a message (websocket/
// impl/read.hpp:1063-1385): the frame loop over parse_fh, the inflater with
// rd_msg_max applied to the inflated size (:1357-1367) and the UTF-8 check of
// text (:1372-1384).  The per-entry rules -- who is inflated and with what
// room, how the statuses merge -- are receive_plan.h, shared with the CPU
// tests.
//
// bpmd_receive_batch enqueues, all on the caller's stream and with nothing
// read back by any step of its own:
//   1. the frame pass       bpmd_unframe_batch's launch, unchanged;
//   2. recv_select_kernel   the inflater's length and capacity arrays (the
//                           gathered length and the effective capacity for an
//                           entry that completed a compressed message, 0 and 0
//                           for every other);
//   3. the inflater         bpmd_inflate_batch over all n entries, straight
//                           from the gathered slots into the message slots;
//   4. recv_finish_kernel   the merged status, the UTF-8 check of text from
//                           whichever slot holds the message, d_msg_len of
//                           the entries that were not inflated.
// What steps 2-4 hand each other lives in the caller's workspace, so nothing
// of a call lives in the stream's shared scratch while the stream's launch
// lock is released around step 3 (bpmd_inflate_batch takes that lock itself).
//
// The finish kernel follows utf8_kernel's data path (pmd_frame.hip; the walk
// is utf8_fails in receive_common.h, shared with pmd_receive_takeover.hip):
// one wave per entry, 16 bytes per lane per step in aligned 16-byte loads plus
// 4 look-ahead bytes, the all-ASCII early out, span flags at the two ragged
// edges.  Most entries of a batch need no byte pass at all (binary, refused,
// incomplete): their wave reads the entry's plan and goes on.  No wave waits
// for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/beast_pmd.h"
#include "pmd_internal.h"
#include "receive_common.h"
#include "receive_plan.h"

namespace bpmd {
namespace recv {

// step 2: receive_plan.h's select per entry
__global__ void __launch_bounds__(256)
recv_select_kernel(const uint8_t* __restrict__ event, const int32_t* __restrict__ status,
                   const uint8_t* __restrict__ compressed, const uint8_t* __restrict__ op,
                   const uint32_t* __restrict__ out_len, const uint32_t* __restrict__ msg_cap, uint64_t msg_max,
                   uint32_t n, uint32_t* __restrict__ z_in_len, uint32_t* __restrict__ z_cap, uint8_t* __restrict__ z_text)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rp::Select s = rp::select(event[i], status[i], compressed[i], op[i], out_len[i], msg_cap[i], msg_max);
    z_in_len[i] = s.in_len;
    z_cap[i] = s.eff_cap;
    z_text[i] = (uint8_t)s.text;
}

// step 4: one wave per entry.  zst == nullptr: permessage-deflate is off,
// nothing was inflated (the frame pass refuses RSV1) and msg_len may be null.
// Stores: status of an entry whose status changes, msg_len of an entry that
// was not inflated; out and msg are only read, each inside the bytes its own
// entry's message occupies (rounded out to aligned 16-byte blocks, which stay
// on the pages of those bytes).
__global__ void __launch_bounds__(WAVE * WPB)
recv_finish_kernel(const uint8_t* __restrict__ event, const uint8_t* __restrict__ compressed,
                   const uint8_t* __restrict__ op, const uint8_t* __restrict__ out,
                   const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ out_len,
                   const uint8_t* __restrict__ msg, const uint64_t* __restrict__ msg_off,
                   const uint32_t* __restrict__ msg_cap, uint64_t msg_max, const int32_t* __restrict__ zst, uint32_t n,
                   uint32_t* __restrict__ msg_len, int32_t* __restrict__ status)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const int32_t st = status[m];
        const bool z = zst && rp::inflates(event[m], st, compressed[m]);
        const rp::Merge g = rp::merge(event[m], st, compressed[m], op[m], out_len[m], z ? msg_cap[m] : 0u, msg_max,
                                      z ? zst[m] : 0, z ? msg_len[m] : 0u);
        int32_t res = g.status;
        if (g.src != rp::SRC_NONE) {
            const uint8_t* p = g.src == rp::SRC_INFLATED ? msg + msg_off[m] : out + out_off[m];
            if (utf8_fails(p, g.msg_len, lane)) res = rp::E_BAD_FRAME_PAYLOAD;
        }
        if (lane == 0) {
            if (res != st) status[m] = res;
            if (!z && msg_len) msg_len[m] = g.msg_len;
        }
    }
}

static_assert(rp::E_NEED_BUFFERS == BPMD_NEED_BUFFERS && rp::E_BAD_FRAME_PAYLOAD == BPMD_BAD_FRAME_PAYLOAD &&
                  rp::E_BUFFER_OVERFLOW == BPMD_WS_BUFFER_OVERFLOW && rp::E_MESSAGE_TOO_BIG == BPMD_WS_MESSAGE_TOO_BIG &&
                  rp::EV_MESSAGE == BPMD_EV_MESSAGE,
              "receive_plan.h and beast_pmd.h name the same values");

}  // namespace recv
}  // namespace bpmd

using namespace bpmd;

namespace {
unsigned elem_grid(uint32_t n) { return (n + 255u) / 256u; }
}  // namespace

extern "C" size_t bpmd_receive_work_bytes(uint32_t n)
{
    return 3 * recv::align256((size_t)n * sizeof(uint32_t)) + recv::align256((size_t)n);
}

// Inherited from bpmd_inflate_batch: a stream's first block-parallel call
// without bpmd_inflate_reserve reads its workspace totals back once
// (pmd_capi.hip).  No step added here reads anything back.
extern "C" int bpmd_receive_batch(const bpmd_cfg* cfg, int role, int pmd_on, uint64_t msg_max, const uint8_t* d_wire,
                                  const uint64_t* d_wire_off, const uint32_t* d_wire_len, uint32_t n,
                                  bpmd_rd_state* d_state, uint8_t* d_out, const uint64_t* d_out_off,
                                  const uint32_t* d_out_cap, uint32_t* d_out_len, uint8_t* d_op, uint8_t* d_compressed,
                                  uint8_t* d_event, int32_t* d_status, uint32_t* d_consumed, uint8_t* d_ctl,
                                  uint8_t* d_ctl_len, uint16_t* d_close_code, uint8_t* d_msg,
                                  const uint64_t* d_msg_off, const uint32_t* d_msg_cap, uint32_t* d_msg_len,
                                  void* d_work, void* stream)
{
    if (role != BPMD_ROLE_SERVER && role != BPMD_ROLE_CLIENT) return BPMD_R_INVALID_ARGUMENT;
    if (pmd_on) {   // the inflater's own check of cfg, which touches no device
        if (cfg && (cfg->flags & BPMD_F_RAW)) return BPMD_R_INVALID_ARGUMENT;
        const int r = bpmd_inflate_batch(cfg, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         stream);
        if (r) return r;
    }
    if (n == 0) return BPMD_R_OK;
    if (!d_wire || !d_wire_off || !d_wire_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_op ||
        !d_compressed || !d_event || !d_status || !d_consumed || !d_ctl || !d_ctl_len || !d_close_code)
        return BPMD_R_INVALID_ARGUMENT;
    if (pmd_on && (!d_msg || !d_msg_off || !d_msg_cap || !d_msg_len || !d_work)) return BPMD_R_INVALID_ARGUMENT;
    int r = bpmd_init();
    if (r) return r;
    const hipStream_t s = (hipStream_t)stream;
    if (launch_unframe((uint32_t)role, pmd_on ? 1u : 0u, msg_max, d_wire, d_wire_off, d_wire_len, n, d_state, d_out,
                       d_out_off, d_out_cap, d_out_len, d_op, d_compressed, d_event, d_status, d_consumed, d_ctl,
                       d_ctl_len, d_close_code, s))
        return BPMD_R_HIP_ERROR;
    recv::Work w{nullptr, nullptr, nullptr, nullptr};
    if (pmd_on) {
        w = recv::carve(d_work, n);
        hipLaunchKernelGGL(recv::recv_select_kernel, dim3(elem_grid(n)), dim3(256), 0, s, d_event, d_status,
                           d_compressed, d_op, d_out_len, d_msg_cap, msg_max, n, w.z_in_len, w.z_cap, w.z_text);
        if (hipGetLastError() != hipSuccess) return BPMD_R_HIP_ERROR;
        // not under this stream's launch lock: the inflater takes it itself
        r = bpmd_inflate_batch(cfg, d_out, d_out_off, w.z_in_len, n, d_msg, d_msg_off, w.z_cap, d_msg_len, w.zst,
                               stream);
        if (r) return r;
    }
    hipLaunchKernelGGL(recv::recv_finish_kernel, dim3(recv::wave_grid(n)), dim3(recv::WAVE * recv::WPB), 0, s,
                       d_event, d_compressed, d_op, d_out, d_out_off, d_out_len, d_msg, d_msg_off, d_msg_cap, msg_max,
                       w.zst, n, d_msg_len, d_status);
    return hipGetLastError() != hipSuccess ? BPMD_R_HIP_ERROR : BPMD_R_OK;
}
