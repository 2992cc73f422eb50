// pmd_send_pieces.hip -- the chained send call for messages that arrive in
// pieces: bpmd_send_takeover_batch's path (pmd_send_takeover.hip) with Beast's
// write_some(fin, buffers) state -- wr_cont_, wr_compress_ and the opcode --
// kept per connection on the device in a bpmd_wr_state, so a caller streams a
// message as write_some(false, ...) ... write_some(true, ...) one piece per
// call, and a per-connection no_context_takeover flag that resets the history
// at a compressed message's end.  The piece rules are send_pieces_plan.h, on
// top of send_takeover_plan.h and send_plan.h, all shared with the CPU tests.
//
// bpmd_send_pieces_batch enqueues, all on the caller's stream:
//   1. send_pc_place_kernel   per entry the message's decision (the first
//                             piece's begin_msg, later pieces the stored one),
//                             the provisional status, the deflater's input
//                             length, history and input offset; slide and copy
//                             as send_tk_place_kernel; d_pos after a slide;
//   2. the deflater           deflate_takeover_bounded over all n entries;
//   3. send_pc_size_kernel    the status so far, the marker 00 00 FF FF behind
//                             a non-final compressed piece's payload, each
//                             piece's wire size and its first / fin flags;
//      then send_scan_frames (pmd_send.hip) with those flags;
//   4. send_pc_finish_kernel  d_pos and d_state from the final status.
// Nothing is read back.  d_state is read by steps 1, 3 and 4 and written by
// step 4 alone, so every step sees the state the call began with.
//
// The place kernel is send_tk_place_kernel's byte mover: one wave per entry,
// no LDS, 16 bytes per lane per step and a byte tail.  No wave waits for
// another.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/beast_pmd.h"
#include "pmd_internal.h"
#include "send_pieces_plan.h"
#include "send_plan.h"
#include "send_takeover_plan.h"
#include "wave_util.h"

namespace bpmd {
namespace sendpc {

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
    uint8_t* first;       // the piece's first frame opens a message
    uint8_t* fin;         // its last frame ends one
};

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline Work carve(void* d_work, uint32_t n)
{
    uint8_t* p = (uint8_t*)d_work;
    const size_t a4 = align256((size_t)n * sizeof(uint32_t)), a8 = align256((size_t)n * sizeof(uint64_t));
    const size_t a1 = align256((size_t)n);
    return Work{(uint32_t*)p,           (uint32_t*)(p + a4), (int32_t*)(p + 2 * a4), (uint64_t*)(p + 3 * a4),
                p + 3 * a4 + a8, p + 3 * a4 + a8 + a1};
}

__device__ __forceinline__ spp::WrState load_state(const bpmd_wr_state* st, uint32_t i)
{
    spp::WrState s;
    __builtin_memcpy(&s, st + i, sizeof s);
    return s;
}

// step 1.  Stores as send_tk_place_kernel's: the four workspace arrays and
// compressed of every entry; of a connection that slides, [base, base + K) of
// its buffer and pos = K; of an entry that enters the deflater, its piece's
// bytes at [base + new_pos, base + new_pos + len).  The piece may land on the
// bytes the slide has just read: the wave's slide loads are complete before
// its slide stores, and those come before the copy.  state is only read.
__global__ void __launch_bounds__(WAVE * WPB)
send_pc_place_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                     const uint32_t* __restrict__ in_len, const uint8_t* __restrict__ op,
                     const uint8_t* __restrict__ opt, const bpmd_wr_state* __restrict__ state, uint64_t threshold,
                     uint32_t L, uint8_t* buf, const uint64_t* __restrict__ base, uint32_t slot, uint32_t n,
                     uint32_t* __restrict__ pos, uint8_t* __restrict__ compressed, uint32_t* __restrict__ z_in_len,
                     uint32_t* __restrict__ z_hist, int32_t* __restrict__ prov, uint64_t* __restrict__ z_off)
{
    const unsigned lane = threadIdx.x & (WAVE - 1);
    for (uint32_t m = blockIdx.x * WPB + (threadIdx.x / WAVE); m < n; m += gridDim.x * WPB) {
        const uint32_t len = in_len[m], o = op ? op[m] : (uint32_t)sp::OP_BINARY;
        const spp::Begin b = spp::begin(load_state(state, m), o, opt ? opt[m] != 0 : true, len, threshold);
        const bool c = b.compress != 0;
        const int32_t st = spp::provisional(o, c, len, L);
        const bool enters = c && st == 0;
        const uint32_t p0 = pos[m] < slot ? pos[m] : slot;   // a fill never exceeds the slot
        const stp::Place pl = spp::place(p0, len, slot, spp::K, enters);
        uint8_t* dst = buf + base[m];
        if (pl.slide) {   // wave-uniform
            wave_copy(dst, dst + p0 - spp::K, spp::K, lane);
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

// step 3: the status so far (provisional, then the deflater's, then the
// marker's room), the marker, the piece's wire size (0 for an idle or refused
// entry, which send_frame_kernel then leaves out) and its frame flags.  The
// marker's four bytes lie inside the staging slot: z_len + 4 <= z_cap.
__global__ void __launch_bounds__(256)
send_pc_size_kernel(const uint32_t* __restrict__ in_len, uint32_t* __restrict__ z_len, uint8_t* __restrict__ z,
                    const uint64_t* __restrict__ z_off, const uint32_t* __restrict__ z_cap,
                    const uint8_t* __restrict__ op, const uint8_t* __restrict__ compressed,
                    const int32_t* __restrict__ prov, const uint8_t* __restrict__ fin,
                    const bpmd_wr_state* __restrict__ state, uint32_t masked, uint32_t frag, uint32_t frame_max,
                    uint32_t n, int32_t* __restrict__ status, uint64_t* __restrict__ sizes,
                    uint8_t* __restrict__ w_first, uint8_t* __restrict__ w_fin)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool c = compressed[i] != 0, last = fin ? fin[i] != 0 : true;
    const bool enters = c && prov[i] == 0;
    const uint32_t o = op ? op[i] : (uint32_t)sp::OP_BINARY;
    const uint32_t zl = enters ? z_len[i] : 0u;
    const int32_t st = spp::status(prov[i], enters, status[i], last, zl, z_cap[i]);
    uint64_t len = spp::payload_len(c, last, in_len[i], zl);
    if (st == 0 && enters && !last) {
        uint8_t* p = z + z_off[i] + zl;
        p[0] = 0x00, p[1] = 0x00, p[2] = 0xFF, p[3] = 0xFF;
        z_len[i] = (uint32_t)len;
    }
    sizes[i] = st || o == stp::OP_IDLE ? 0 : sp::wire_size(sp::split(len, frame_max, c, frag != 0), masked != 0);
    status[i] = st;
    w_first[i] = spp::frame_first(0, load_state(state, i).wr_cont != 0) ? 1 : 0;
    w_fin[i] = last ? 1 : 0;
}

// step 4: spp::commit from the final status; each of pos and state is written
// only when its value changes
__global__ void __launch_bounds__(256)
send_pc_finish_kernel(const uint32_t* __restrict__ in_len, const uint32_t* __restrict__ z_in_len,
                      const uint8_t* __restrict__ op, const uint8_t* __restrict__ opt,
                      const uint8_t* __restrict__ compressed, const int32_t* __restrict__ prov,
                      const int32_t* __restrict__ status, const uint8_t* __restrict__ fin,
                      const uint8_t* __restrict__ no_takeover, uint64_t threshold, uint32_t n,
                      uint32_t* __restrict__ pos, bpmd_wr_state* __restrict__ state)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const spp::WrState s0 = load_state(state, i);
    const uint32_t o = op ? op[i] : (uint32_t)sp::OP_BINARY, p0 = pos[i];
    const spp::Begin b = spp::begin(s0, o, opt ? opt[i] != 0 : true, in_len[i], threshold);
    const spp::Commit cm =
        spp::commit(s0, p0, z_in_len[i], compressed[i] != 0 && prov[i] == 0, b, o == stp::OP_IDLE, status[i],
                    fin ? fin[i] != 0 : true, no_takeover ? no_takeover[i] != 0 : false);
    if (cm.pos != p0) pos[i] = cm.pos;
    uint32_t a, z;
    __builtin_memcpy(&a, &s0, 4);
    __builtin_memcpy(&z, &cm.state, 4);
    if (a != z) __builtin_memcpy(state + i, &cm.state, 4);
}

static_assert(sizeof(bpmd_wr_state) == sizeof(spp::WrState), "send_pieces_plan.h mirrors bpmd_wr_state");
static_assert(spp::K % 16 == 0, "a slide is whole 16-byte units");

}  // namespace sendpc
}  // namespace bpmd

using namespace bpmd;

extern "C" uint64_t bpmd_send_piece_frame_bound(uint64_t len, uint32_t frame_max, int may_compress, int frag, int fin)
{
    return frame_max ? spp::piece_frame_bound(len, frame_max, may_compress != 0, frag != 0, fin != 0) : 0;
}

extern "C" uint64_t bpmd_send_piece_wire_bound(uint64_t len, uint32_t frame_max, int masked, int may_compress, int frag,
                                               int fin)
{
    return frame_max ? spp::piece_wire_bound(len, frame_max, masked != 0, may_compress != 0, frag != 0, fin != 0) : 0;
}

// bpmd_send_takeover_work_bytes' arrays, then the first and fin flags
extern "C" size_t bpmd_send_pieces_work_bytes(uint32_t n)
{
    return 3 * sendpc::align256((size_t)n * sizeof(uint32_t)) + sendpc::align256((size_t)n * sizeof(uint64_t)) +
           2 * sendpc::align256((size_t)n);
}

// No step of this call reads anything back: the deflater gets the bound
// n * ceil(L / 4096) in place of its chunk count.
extern "C" int bpmd_send_pieces_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                                      const uint32_t* d_in_len, uint32_t n, int role, uint64_t threshold, int frag,
                                      uint32_t frame_max, uint32_t max_len, const uint8_t* d_op, const uint8_t* d_opt,
                                      const uint8_t* d_fin, const uint8_t* d_no_takeover, bpmd_wr_state* d_state,
                                      uint8_t* d_buf, const uint64_t* d_base, uint32_t slot_bytes, uint32_t* d_pos,
                                      uint8_t* d_z, const uint64_t* d_z_off, const uint32_t* d_z_cap,
                                      uint32_t* d_z_len, const uint32_t* d_keys, const uint32_t* d_key_base,
                                      uint8_t* d_wire, uint64_t wire_cap, uint64_t* d_wire_off, uint32_t* d_wire_len,
                                      uint8_t* d_compressed, int32_t* d_status, uint64_t* d_total, void* d_work,
                                      void* stream)
{
    if (frame_max == 0 || (role != BPMD_ROLE_SERVER && role != BPMD_ROLE_CLIENT) || n > (uint32_t)INT_MAX)
        return BPMD_R_INVALID_ARGUMENT;
    if (!cfg || (cfg->flags & (BPMD_F_EXACT | BPMD_F_RAW))) return BPMD_R_INVALID_ARGUMENT;
    // the deflater's own check of cfg, which touches no device
    int r = bpmd_deflate_batch(cfg, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
    if (r) return r;
    if (slot_bytes <= 2u * spp::K || max_len == 0) return BPMD_R_INVALID_ARGUMENT;
    const uint32_t L = spp::room(max_len, slot_bytes, spp::K);
    const uint64_t bound = dfl::chunk_bound(n, L);   // none reaches the deflater with more than L bytes
    if (bound > 0xFFFFFFFFull) return BPMD_R_INVALID_ARGUMENT;
    if (n == 0) return BPMD_R_OK;
    if (!d_in || !d_in_off || !d_in_len || !d_state || !d_buf || !d_base || !d_pos || !d_z || !d_z_off || !d_z_cap ||
        !d_z_len || (!d_wire && wire_cap) || !d_wire_off || !d_wire_len || !d_compressed || !d_status || !d_total ||
        !d_work)
        return BPMD_R_INVALID_ARGUMENT;
    if (role == BPMD_ROLE_CLIENT && (!d_keys || !d_key_base)) return BPMD_R_INVALID_ARGUMENT;
    r = bpmd_init();
    if (r) return r;
    const hipStream_t s = (hipStream_t)stream;
    const bool masked = role == BPMD_ROLE_CLIENT;
    const sendpc::Work w = sendpc::carve(d_work, n);
    const unsigned want = (n + sendpc::WPB - 1) / sendpc::WPB, cap = (unsigned)cu_count() * 8u;
    hipLaunchKernelGGL(sendpc::send_pc_place_kernel, dim3(want < cap ? want : cap), dim3(sendpc::WAVE * sendpc::WPB), 0,
                       s, d_in, d_in_off, d_in_len, d_op, d_opt, d_state, threshold, L, d_buf, d_base, slot_bytes, n,
                       d_pos, d_compressed, w.z_in_len, w.z_hist, w.prov, w.z_off);
    if (hipGetLastError() != hipSuccess) return BPMD_R_HIP_ERROR;
    // not under this stream's launch lock: the deflater takes it itself
    const Batch b{d_buf, w.z_off, w.z_in_len, n, d_z, d_z_off, d_z_cap, d_z_len, d_status};
    DeflateOpts zo;
    zo.hist_len = w.z_hist, zo.chunks = {dfl::ChunkSource::BOUND, bound};
    r = deflate_takeover_bounded(cfg, b, zo, s);
    if (r) return r;
    const dim3 egrid((n + 255u) / 256u), eblock(256);
    SendFrames a{d_in, d_in_off, d_in_len, n, masked, frag != 0, frame_max, d_op, d_z, d_z_off, d_z_len,
                 masked ? d_keys : nullptr, d_key_base, d_wire, wire_cap, d_wire_off, d_wire_len, d_compressed,
                 d_status, d_total};
    a.first = w.first, a.fin = w.fin;
    r = send_scan_frames(
        a,
        [&](uint64_t* sizes) {
            hipLaunchKernelGGL(sendpc::send_pc_size_kernel, egrid, eblock, 0, s, d_in_len, d_z_len, d_z, d_z_off,
                               d_z_cap, d_op, d_compressed, w.prov, d_fin, d_state, masked ? 1u : 0u, frag ? 1u : 0u,
                               frame_max, n, d_status, sizes, w.first, w.fin);
        },
        s);
    if (r) return r;
    hipLaunchKernelGGL(sendpc::send_pc_finish_kernel, egrid, eblock, 0, s, d_in_len, w.z_in_len, d_op, d_opt,
                       d_compressed, w.prov, d_status, d_fin, d_no_takeover, threshold, n, d_pos, d_state);
    return hipGetLastError() != hipSuccess ? BPMD_R_HIP_ERROR : BPMD_R_OK;
}
