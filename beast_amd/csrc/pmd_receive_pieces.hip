// pmd_receive_pieces.hip -- the chained receive call that hands a message over
// in pieces (bpmd_receive_pieces_batch): read_some as Beast runs it
// (websocket/impl/read.hpp:1063-1385), one piece per connection per call, with
// rd_remain, the rotated rd_key, the inflater and the UTF-8 checker's cut code
// point carried on the device between calls.  bpmd_send_pieces_batch's
// counterpart; the rules are receive_pieces_plan.h, shared with the CPU tests.
//
// bpmd_receive_pieces_batch enqueues, all on the caller's stream:
//   1. recv_pc_walk_kernel    the piece walk: headers, the payload parts that
//                             have arrived unmasked into the out slot from its
//                             offset 0, 00 00 FF FF behind a compressed
//                             message's last piece, control payloads; then the
//                             entry's call record for the inflater (no state =
//                             nothing to inflate) and the window bits of a
//                             connection's first use;
//   2. the inflater           zstream_write_sel_kernel (pmd_zstream.hip): one
//                             inflate_stream::write(Flush::sync) of the
//                             connection's own state machine per record, piece
//                             (+ tail) -> message slot;
//   3. recv_pc_finish_kernel  the merged status, the UTF-8 check with its
//                             carry where the piece lies, d_msg_len, the
//                             committed state.
// Without the extension (pmd_on == 0) step 2 is left out and step 1 writes no
// record.  Nothing is read back.
//
// Walk and finish are byte movers, one wave per entry (receive_common.h's
// geometry), no LDS, no atomics, and no wave waits for another.  The walk is
// wave-uniform: every lane runs the header step on the same bytes, and the
// lanes share the copies, 16 bytes per lane per step through byte-aligned
// vector accesses -- a resumed payload starts at any wire offset and key
// phase, a piece at any slot alignment; the rotated key makes byte 0 of every
// copy take the key's byte 0, so every dword of a 16-byte unit takes the key
// as it is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/beast_pmd.h"
#include "pmd_internal.h"
#include "receive_common.h"
#include "receive_pieces_plan.h"
#include "zstream.h"

namespace bpmd {
namespace recv {

typedef uint4 uint4_pu __attribute__((aligned(1)));

// len payload bytes from src to dst, XORed with key from its byte 0 on
__device__ __forceinline__ void piece_copy_xor(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t key,
                                               unsigned lane)
{
    const uint32_t full = len >> 4;
    for (uint32_t u = lane; u < full; u += WAVE) {
        uint4 v = *(const uint4_pu*)(src + 16 * u);
        v.x ^= key;
        v.y ^= key;
        v.z ^= key;
        v.w ^= key;
        *(uint4_pu*)(dst + 16 * u) = v;
    }
    const uint32_t t = 16 * full + lane;
    if (t < len) dst[t] = src[t] ^ (uint8_t)(key >> (8 * (t & 3u)));
}

// step 1.  Stores: the entry's ten outputs and its state; inside its out slot
// the piece and the tail (rpp::walk's bounds); its control slot; its call
// record; wbits of its inflater state when that is still zero.
__global__ void __launch_bounds__(WAVE * WPB)
recv_pc_walk_kernel(uint32_t role, uint32_t pmd_on, uint64_t msg_max, uint32_t wbits,
                    const uint8_t* __restrict__ wire, const uint64_t* __restrict__ wire_off,
                    const uint32_t* __restrict__ wire_len, uint32_t n, rpp::PieceState* __restrict__ state,
                    zst::State* __restrict__ zstate, uint8_t* __restrict__ out, const uint64_t* __restrict__ out_off,
                    const uint32_t* __restrict__ out_cap, uint32_t* __restrict__ out_len, uint8_t* __restrict__ op,
                    uint8_t* __restrict__ compressed, uint8_t* __restrict__ event, int32_t* __restrict__ status,
                    uint32_t* __restrict__ consumed, uint8_t* __restrict__ ctl, uint8_t* __restrict__ ctl_len,
                    uint16_t* __restrict__ close_code, uint8_t* __restrict__ msg, const uint64_t* __restrict__ msg_off,
                    const uint32_t* __restrict__ msg_cap, zst::ZCall* __restrict__ calls,
                    zst::Result* __restrict__ results)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const uint8_t* p = wire + wire_off[m];
        const uint32_t wl = wire_len[m], cap = out_cap[m];
        uint8_t* dst = out + out_off[m];
        rpp::PieceState st = state[m];
        uint8_t* c = ctl + 128u * (uint64_t)m;
        rpp::Stop s;
        rpp::walk(
            p, wl, role, pmd_on != 0, msg_max, cap, st,
            [&](uint32_t at, const uint8_t* src, uint32_t len, uint32_t key) {
                piece_copy_xor(dst + at, src, len, key, lane);
            },
            [&](const uint8_t* src, uint32_t len, uint32_t key) {
                for (uint32_t t = lane; t < len; t += WAVE) c[t] = src[t] ^ (uint8_t)(key >> (8 * (t & 3u)));
            },
            [&](uint32_t at) {
                if (lane < rpp::TAIL) dst[at + lane] = lane < 2 ? (uint8_t)0 : (uint8_t)0xff;
            },
            s);
        if (lane == 0) {
            out_len[m] = s.piece_len;
            op[m] = (uint8_t)s.msg_op;
            compressed[m] = (uint8_t)s.msg_deflated;
            event[m] = (uint8_t)s.event;
            status[m] = s.status;
            consumed[m] = s.consumed;
            ctl_len[m] = (uint8_t)s.ctl_len;
            close_code[m] = s.close_code;
            if (s.consumed) state[m] = st;   // an entry that took nothing keeps its state as it is
            if (calls) {
                zst::ZCall z{};
                if (rpp::inflates(s.msg_deflated, s.piece_len, s.tail)) {
                    zst::State* zs = zstate + m;
                    if (zs->h.wbits == 0) zs->h.wbits = wbits;   // all zero otherwise: HEAD, empty reservoir and window
                    z.st = zs;
                    // The slot may start at any residue mod 16, and zstream_run stages its input with
                    // 16-byte vector loads from `in` (pmd_zstream.hip, stage()), written for the 256-byte
                    // aligned inputs of pmd_stream.hip.  Here those loads are misaligned: they rely on
                    // gfx950's unaligned global access (the mode the HSA runtime sets) and on the compiler
                    // emitting one plain global_load_dwordx4 for them, as it does for the aligned(1)
                    // accesses above.  They also read up to 15 bytes past in + n_in: the header asks
                    // for that much readable memory behind every out slot.
                    z.in = dst;
                    z.n_in = s.piece_len + (s.tail ? rpp::TAIL : 0u);
                    z.out = msg + msg_off[m];
                    z.cap = rpp::limit_room(msg_cap[m], msg_max, st.rd_size);
                    z.res = results + m;
                    z.flush = 3;   // Flush::sync
                }
                calls[m] = z;
            }
        }
    }
}

// utf8_fails' walk (receive_common.h) with the two verdicts kept apart: err,
// the nb bytes at p are no prefix of well-formed UTF-8; inc, they end inside a
// code point.  Wave-uniform results.
__device__ __forceinline__ void utf8_scan(const uint8_t* __restrict__ p, uint32_t nb, unsigned lane, bool& any_err,
                                          bool& any_inc)
{
    using frame::H;
    any_err = any_inc = false;
    if (nb == 0) return;
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
        uint32_t v[5];
#pragma unroll
        for (int d = 0; d < 5; ++d)
            v[d] = frame::span_flags((int32_t)s - (int32_t)(b0 + 4 * d), (int32_t)end - (int32_t)(b0 + 4 * d));
        frame::utf8_unit(x, v, err, inc);
        if (u == 0) {   // the first byte must start a code point
            const uint32_t f = x[s >> 2] >> (8 * (s & 3));
            err = err || (f & 0xC0u) == 0x80u;
        }
    }
    any_err = __any(err) != 0;
    any_inc = __any(inc) != 0;
}

// step 3.  results: the inflater's (looked at for an entry that ran it only).
// Stores: msg_len, status of an entry whose status changes, the committed
// state of an entry that consumed something; out and msg are only read, inside
// the piece (rounded out to aligned 16-byte blocks, which stay on its pages).
__global__ void __launch_bounds__(WAVE * WPB)
recv_pc_finish_kernel(uint64_t msg_max, const uint8_t* __restrict__ event, const uint8_t* __restrict__ compressed,
                      const uint8_t* __restrict__ op, const uint32_t* __restrict__ consumed,
                      const uint8_t* __restrict__ out, const uint64_t* __restrict__ out_off,
                      const uint32_t* __restrict__ out_len, const uint8_t* __restrict__ msg,
                      const uint64_t* __restrict__ msg_off, const zst::Result* __restrict__ results, uint32_t n,
                      rpp::PieceState* __restrict__ state, uint32_t* __restrict__ msg_len,
                      int32_t* __restrict__ status)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const bool last = event[m] == fp::EV_MESSAGE;
        const uint32_t comp = compressed[m], got = out_len[m];
        const int32_t fst = status[m];
        rpp::PieceState st = state[m];
        const bool ran = rpp::inflates(comp, got, last && comp ? 1u : 0u);
        int32_t pst = 0;
        uint64_t delivered = comp ? 0u : got;
        const uint8_t* piece = out + out_off[m];
        if (ran) {
            const zst::Result r = results[m];
            const uint64_t n_in = (uint64_t)got + (last ? rpp::TAIL : 0u);
            pst = rpp::merge(r.ec, r.in_used, n_in, r.out_used, st.rd_size, msg_max);
            delivered = r.published ? r.out_used : 0u;   // an error that skipped done() hands nothing over
            piece = msg + msg_off[m];
        }
        const uint32_t len = (uint32_t)delivered;
        uint32_t cn = st.utf8_n;
        uint8_t cb[3] = {st.utf8_b[0], st.utf8_b[1], st.utf8_b[2]};
        // a text piece, or the end of a text message with nothing to deliver
        if (op[m] == fp::OP_TEXT && pst == 0 && (len != 0 || last)) {
            const rpp::Utf8Head h = rpp::utf8_head(cn, cb, [&](uint32_t i) { return (uint32_t)piece[i]; }, len);
            bool err = h.bad != 0, inc = false;
            const uint32_t rest = len - h.skip;
            if (!err) utf8_scan(piece + h.skip, rest, lane, err, inc);   // wave-uniform branch
            rpp::Utf8Head t = h;
            if (!err && h.n == 0) t = rpp::utf8_tail([&](uint32_t i) { return (uint32_t)piece[h.skip + i]; }, rest);
            (void)inc;   // a cut code point is what t carries
            if (err || (last && t.n != 0)) pst = rp::E_BAD_FRAME_PAYLOAD;
            cn = t.n;
            cb[0] = t.b[0], cb[1] = t.b[1], cb[2] = t.b[2];
        }
        if (lane == 0) {
            msg_len[m] = len;
            if (pst != 0 && pst != fst) status[m] = pst;
            if (consumed[m]) {
                rpp::commit(st, last, ran ? delivered : 0u, cn, cb);
                state[m] = st;
            }
        }
    }
}

}  // namespace recv
}  // namespace bpmd

using namespace bpmd;

static_assert(sizeof(bpmd_rd_piece_state) == 32 && sizeof(rpp::PieceState) == sizeof(bpmd_rd_piece_state),
              "receive_pieces_plan.h mirrors bpmd_rd_piece_state");
static_assert(sizeof(zst::State) % 16 == 0, "inflater states follow each other 16-byte aligned");
static_assert(sizeof(zst::ZCall) == 64 && sizeof(zst::Result) == 32, "workspace records");

extern "C" size_t bpmd_receive_pieces_zstate_bytes(void) { return sizeof(zst::State); }

// per entry a call record and a result, each array from a 256-byte boundary
extern "C" size_t bpmd_receive_pieces_work_bytes(uint32_t n)
{
    return recv::align256((size_t)n * sizeof(zst::ZCall)) + recv::align256((size_t)n * sizeof(zst::Result));
}

extern "C" int bpmd_receive_pieces_batch(const bpmd_cfg* cfg, int role, int pmd_on, uint64_t msg_max,
                                         const uint8_t* d_wire, const uint64_t* d_wire_off, const uint32_t* d_wire_len,
                                         uint32_t n, bpmd_rd_piece_state* d_state, void* d_zstate, uint8_t* d_out,
                                         const uint64_t* d_out_off, const uint32_t* d_out_cap, uint32_t* d_out_len,
                                         uint8_t* d_op, uint8_t* d_compressed, uint8_t* d_event, int32_t* d_status,
                                         uint32_t* d_consumed, uint8_t* d_ctl, uint8_t* d_ctl_len,
                                         uint16_t* d_close_code, uint8_t* d_msg, const uint64_t* d_msg_off,
                                         const uint32_t* d_msg_cap, uint32_t* d_msg_len, void* d_work, void* stream)
{
    if (role != BPMD_ROLE_SERVER && role != BPMD_ROLE_CLIENT) return BPMD_R_INVALID_ARGUMENT;
    if (cfg && (cfg->flags & BPMD_F_RAW)) return BPMD_R_INVALID_ARGUMENT;
    if (pmd_on) {   // the inflater's own check of cfg, which touches no device
        const int r =
            bpmd_inflate_batch(cfg, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
        if (r) return r;
    }
    if (n == 0) return BPMD_R_OK;
    if (!d_wire || !d_wire_off || !d_wire_len || !d_state || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_op ||
        !d_compressed || !d_event || !d_status || !d_consumed || !d_ctl || !d_ctl_len || !d_close_code || !d_msg_len)
        return BPMD_R_INVALID_ARGUMENT;
    if (pmd_on && (!d_zstate || !d_msg || !d_msg_off || !d_msg_cap || !d_work || ((uintptr_t)d_zstate & 15u)))
        return BPMD_R_INVALID_ARGUMENT;
    int r = bpmd_init();
    if (r) return r;
    const hipStream_t s = (hipStream_t)stream;
    zst::ZCall* calls = pmd_on ? (zst::ZCall*)d_work : nullptr;
    zst::Result* results =
        pmd_on ? (zst::Result*)((uint8_t*)d_work + recv::align256((size_t)n * sizeof(zst::ZCall))) : nullptr;
    const dim3 grid(recv::wave_grid(n)), block(recv::WAVE * recv::WPB);
    hipLaunchKernelGGL(recv::recv_pc_walk_kernel, grid, block, 0, s, (uint32_t)role, pmd_on ? 1u : 0u, msg_max,
                       pmd_on ? (uint32_t)cfg->window_bits : 0u, d_wire, d_wire_off, d_wire_len, n,
                       (rpp::PieceState*)d_state, (zst::State*)d_zstate, d_out, d_out_off, d_out_cap, d_out_len, d_op,
                       d_compressed, d_event, d_status, d_consumed, d_ctl, d_ctl_len, d_close_code, d_msg, d_msg_off,
                       d_msg_cap, calls, results);
    if (hipGetLastError() != hipSuccess) return BPMD_R_HIP_ERROR;
    if (pmd_on && bpmd_internal_zstream_write_sel(calls, n, s)) return BPMD_R_HIP_ERROR;
    hipLaunchKernelGGL(recv::recv_pc_finish_kernel, grid, block, 0, s, msg_max, d_event, d_compressed, d_op, d_consumed,
                       d_out, d_out_off, d_out_len, d_msg, d_msg_off, results, n, (rpp::PieceState*)d_state, d_msg_len,
                       d_status);
    return hipGetLastError() != hipSuccess ? BPMD_R_HIP_ERROR : BPMD_R_OK;
}
