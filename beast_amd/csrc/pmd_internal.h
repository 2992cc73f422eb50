// pmd_internal.h -- host-side interfaces between the library's translation
// units: every function one .hip file defines and another calls is declared
// here, once.  What only C++ calls has C++ linkage in namespace bpmd, so a
// declaration that drifts from its definition fails to link; the few symbols
// that tests and scripts load through ctypes keep C linkage (below).
// Device-side helpers live in pmd_common.h.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include <functional>
#include <mutex>

#include "bp.h"
#include "deflate_plan.h"

struct bpmd_cfg;   // include/beast_pmd.h

namespace bpmd {

// A batch as the public calls take it (include/beast_pmd.h): n messages,
// message i at in + in_off[i] (in_len[i] bytes), its output slot at
// out + out_off[i] (out_cap[i] bytes); out_len / status receive the results.
struct Batch {
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    uint32_t n;
    uint8_t* out;
    const uint64_t* out_off;
    const uint32_t* out_cap;
    uint32_t* out_len;
    int32_t* status;
};

// Per (device, stream) scratch blocks (pmd_capi.hip scratch_block): one owner
// each, so no two users of a stream share a workspace.
enum ScratchSlot : int {
    SCR_INFLATE_QUEUE = 0,   // lane inflate work-queue counter
    SCR_DEFLATE_COUNT = 1,   // deflate chunk count and chunk queue
    SCR_DEFLATE_WS = 2,      // deflate chunk workspace
    SCR_EXACT_QUEUE = 3,     // exact deflate message queue
    SCR_EXACT_WS = 4,        // exact deflate per-wave workspace
    SCR_ORDER = 5,           // inflate message order (longest first)
    SCR_WAVE_QUEUE = 6,      // wave inflate work-queue counter
    SCR_DEFLATE_QUEUE = 7,   // deflate single-chunk message counter
    SCR_MULTI_TOTALS = 8,    // multi-device output totals
    SCR_LONG_SPLIT = 9,      // long-payload split
    SCR_BP_STATS = 10,       // block-parallel inflate per-payload stats
    SCR_BP_DECODE = 11,      // block-parallel inflate decode workspace
    SCR_SEND = 12,           // send side: wire sizes and their scan's workspace
};
// Small pinned host blocks per (device, stream): read-back targets
enum PinnedSlot : int {
    PIN_DEFLATE_CHUNKS = 0,   // the deflate chunk count
};

// compute units of the current device (256 when the query fails)
inline int cu_count()
{
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus;
}

// Environment knobs.  Neither helper caches: a caller that reads its knob
// once keeps the value in a static.
inline uint32_t env_uint(const char* name, uint32_t dflt)
{
    const char* e = getenv(name);
    return e ? (uint32_t)strtoul(e, nullptr, 10) : dflt;
}
inline bool env_on(const char* name)   // on unless set to 0
{
    const char* e = getenv(name);
    return !(e && e[0] == '0');
}

// ---- pmd_capi.hip: per-stream resources.  The caller of scratch_block and
// pinned_block holds the stream's launch lock (stream_mutex).
uint8_t* scratch_block(hipStream_t s, size_t bytes, ScratchSlot which);
void* pinned_block(hipStream_t s, size_t bytes, PinnedSlot which);
std::mutex* stream_mutex(hipStream_t s);

// ---- pmd_send.hip: the send side's scan and frame launch, shared by
// bpmd_send_batch and bpmd_send_takeover_batch.  launch_size enqueues the
// caller's size kernel, which fills sizes[n] (0 = not sent) and the status so
// far; then the 64-bit exclusive sum into wire_off and send_frame_kernel.
// Takes the stream's launch lock.  first / fin: per entry, whether the entry's
// first frame opens a message (opcode, RSV1) and its last frame ends one (FIN);
// NULL = every entry is a whole message (bpmd_send_pieces_batch passes both).
struct SendFrames {
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    uint32_t n;
    bool masked, frag;
    uint32_t frame_max;
    const uint8_t* op;
    const uint8_t* z;
    const uint64_t* z_off;
    const uint32_t* z_len;
    const uint32_t* keys;
    const uint32_t* key_base;
    uint8_t* wire;
    uint64_t wire_cap;
    uint64_t* wire_off;
    uint32_t* wire_len;
    const uint8_t* compressed;
    int32_t* status;
    uint64_t* total;
    const uint8_t* first = nullptr;
    const uint8_t* fin = nullptr;
};
int send_scan_frames(const SendFrames& a, const std::function<void(uint64_t* sizes)>& launch_size, hipStream_t s);

// ---- pmd_inflate.hip: one wave per message
int init_fixed();
// min_in != 0: only payloads longer than min_in
int inflate_keyed_split(const Batch& b, uint32_t raw, const uint32_t* mask_key, uint32_t min_in, hipStream_t stream);
int inflate_wave_ordered(const Batch& b, uint32_t raw, const uint32_t* mask_key, const uint32_t* order,
                         const uint32_t* limit, hipStream_t stream);

// ---- pmd_inflate_lane3.hip: one lane per message
int inflate_lane3(const Batch& b, uint32_t raw, const uint32_t* mask_key, const uint32_t* hist_len, uint32_t hist_max,
                  uint32_t max_in, const uint32_t* order, uint32_t* qctr, uint32_t grid_wgs, const uint32_t* skip,
                  hipStream_t stream);
int inflate_lane3_seg(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n_tasks,
                      const bp::SegTask* tasks, uint16_t* sym, bp::SegRes* res, uint32_t raw, uint32_t* qctr,
                      uint32_t grid_wgs, hipStream_t stream, const uint32_t* n_dev);
// the order's keys are in_len >> LANE_ORDER_KEY_SHIFT, descending (exact deflate's queue relies on it: exact_plan.h)
constexpr uint32_t LANE_ORDER_KEY_SHIFT = 6;
const uint32_t* lane_order(const uint32_t* in_len, uint32_t n, hipStream_t stream, const uint32_t** keys_out);

// ---- pmd_inflate_bp.hip: block-parallel decode of long payloads
int inflate_bp(const Batch& b, uint32_t raw, const uint32_t* order, const uint32_t* nlong, hipStream_t s);
void bp_release(hipStream_t s);
int bp_reserve(hipStream_t s, unsigned long long in_bytes, unsigned long long out_bytes, unsigned long long msgs);

// ---- pmd_deflate.hip, pmd_deflate_exact.hip
// what a deflate call is given besides its batch (the arrays: per message, on the device)
struct DeflateOpts {
    int level = 6, window_bits = 15, strategy = 0;
    const int* tune = nullptr;            // deflate_stream::tune's four values, replacing the level's
    const uint32_t* mask_key = nullptr;   // per message; null: unmasked
    const uint32_t* hist_len = nullptr;   // context takeover: bytes of history before each message
    uint32_t* out_bits = nullptr;         // receives each payload's exact bit length
    dfl::ChunkSource chunks;              // (deflate_plan.h) read back unless the caller knows
};
int deflate(const Batch& b, const DeflateOpts& opts, hipStream_t stream);
// pmd_capi.hip: bpmd_deflate_takeover_batch without its wait.  opts carries the
// history lengths and a BOUND on the chunk count, so the call only enqueues; the
// rest comes from cfg, checked, under the stream's launch lock, as in the public call.
int deflate_takeover_bounded(const bpmd_cfg* cfg, const Batch& b, const DeflateOpts& opts, hipStream_t stream);
int deflate_exact(const Batch& b, int level, int window_bits, int mem_level, int strategy, const uint32_t* mask_key,
                  hipStream_t stream);

// ---- pmd_frame.hip
int launch_mask(uint8_t* data, const uint64_t* off, const uint32_t* len, uint32_t n, const uint32_t* key,
                const uint8_t* phase, hipStream_t stream);
int launch_utf8(const uint8_t* data, const uint64_t* off, const uint32_t* len, uint32_t n, int32_t* result,
                const uint8_t* text, int32_t fail_status, hipStream_t stream);
int launch_slide(uint8_t* buf, const uint64_t* base, const uint32_t* pos, const uint32_t* keep, uint32_t n,
                 hipStream_t stream);
int launch_frame(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint8_t* op,
                 const uint8_t* flags, const uint32_t* keys, const uint32_t* key_base, uint32_t frame_max, uint32_t n,
                 uint8_t* wire, const uint64_t* wire_off, hipStream_t stream);
// state: bpmd_rd_state per entry (frame_parse.h RdState), or NULL
int launch_unframe(uint32_t role, uint32_t pmd_on, uint64_t msg_max, const uint8_t* wire, const uint64_t* wire_off,
                   const uint32_t* wire_len, uint32_t n, void* state, uint8_t* out, const uint64_t* out_off,
                   const uint32_t* out_cap, uint32_t* out_len, uint8_t* op, uint8_t* compressed, uint8_t* event,
                   int32_t* status, uint32_t* consumed, uint8_t* ctl, uint8_t* ctl_len, uint16_t* close_code,
                   hipStream_t stream);

}  // namespace bpmd

// C linkage: tests and scripts load these through ctypes (with every
// bpmd_diag_* function, declared where it is defined)
extern "C" {
extern unsigned bpmd_diag_grid_override;   // pmd_capi.hip; 0 = size the grid by occupancy
size_t bpmd_internal_scratch_count(void);
size_t bpmd_internal_pinned_count(void);
void bpmd_internal_scratch_release(hipStream_t s);
int bpmd_internal_zstream_write(void* st, const uint8_t* in, uint64_t n_in, uint8_t* out, uint64_t cap, int flush,
                                void* res, hipStream_t stream);
int bpmd_internal_zstream_write_batch(const void* calls, uint32_t n, hipStream_t stream);
// the same launch over records written on the device; a record whose st is NULL runs nothing
int bpmd_internal_zstream_write_sel(const void* calls, uint32_t n, hipStream_t stream);
const uint32_t* bpmd_internal_lane_long_split(const uint32_t* in_len, const uint32_t* keys, uint32_t n, uint32_t lanes,
                                              uint32_t min_thr, uint32_t share_pct, hipStream_t stream);
}
