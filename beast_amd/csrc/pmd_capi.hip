// pmd_capi.hip -- extern "C" entry points declared in include/beast_pmd.h.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/beast_pmd.h"

#include "inflate_plan.h"
#include "pmd_internal.h"

using namespace bpmd;

namespace {
std::mutex g_init_mu;
uint64_t g_init_devices = 0;   // bit d: device d's symbols are initialised

// Per (device, stream) scratch for batch calls that need device workspace
// (work-queue counters, message order, chunk workspace).  Allocated on first
// use and grown when a larger batch arrives.  A batch call holds its
// stream's launch lock from its first enqueue to its last, so two host
// threads submitting on one stream (the null stream, say) cannot interleave
// their memsets and launches over the same counters and workspace; calls on
// different streams use different scratch.
struct Scratch {
    int dev;
    hipStream_t stream;
    int which;
    uint8_t* p;
    size_t cap;
};
struct StreamLock {
    int dev;
    hipStream_t stream;
    std::mutex* mu;
};
// A side stream per (device, stream): the long payloads of a work-queue
// batch decode block-parallel on it while the lane kernel runs the rest on
// the caller's stream (fork / join events; the caller's stream waits for the
// side stream before anything after the batch call).
struct Side {
    int dev;
    hipStream_t stream;
    hipStream_t side;
    hipEvent_t fork, join;
};
std::mutex g_scratch_mu;
std::vector<Scratch> g_scratch;
std::vector<Scratch> g_pinned;   // small pinned host blocks per (device, stream), same lifetime rules
std::vector<StreamLock> g_locks;
std::vector<Side> g_sides;

bool side_for(hipStream_t s, Side& out)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    for (auto& e : g_sides)
        if (e.dev == dev && e.stream == s) {
            out = e;
            return true;
        }
    Side d{dev, s, nullptr, nullptr, nullptr};
    if (hipStreamCreateWithFlags(&d.side, hipStreamNonBlocking) != hipSuccess) return false;
    if (hipEventCreateWithFlags(&d.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&d.join, hipEventDisableTiming) != hipSuccess) {
        (void)hipStreamDestroy(d.side);
        return false;
    }
    g_sides.push_back(d);
    out = d;
    return true;
}
}  // namespace

// the launch lock of a stream (pmd_multi.hip takes it around its own
// scratch use, as scratch_block requires)
std::mutex* bpmd::stream_mutex(hipStream_t s)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    for (auto& e : g_locks)
        if (e.dev == dev && e.stream == s) return e.mu;
    std::mutex* mu = new (std::nothrow) std::mutex();
    if (mu) g_locks.push_back(StreamLock{dev, s, mu});
    return mu;
}

// the caller holds the stream's launch lock, so nothing else enqueues work
// that could use the block while it is replaced
uint8_t* bpmd::scratch_block(hipStream_t s, size_t bytes, ScratchSlot which)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    uint8_t* old = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_scratch_mu);
        for (auto& e : g_scratch)
            if (e.dev == dev && e.stream == s && e.which == which) {
                if (e.cap >= bytes) return e.p;
                old = e.p;
                e.p = nullptr;
                e.cap = 0;
                break;
            }
    }
    // the stream may still use the old block: free it once the stream is idle
    if (old) {
        if (hipStreamSynchronize(s) != hipSuccess) return nullptr;
        (void)hipFree(old);
    }
    uint8_t* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    for (auto& e : g_scratch)
        if (e.dev == dev && e.stream == s && e.which == which) {
            e.p = p;
            e.cap = bytes;
            return p;
        }
    g_scratch.push_back(Scratch{dev, s, which, p, bytes});
    return p;
}

// A small pinned host block per (device, stream, which) -- the target of a
// read-back that an event then covers.  Kept
// per stream, not per host thread: pmd_multi.hip launches each shard from a
// thread of its own, and a thread_local block would leak one pinned
// allocation per shard thread.  The caller holds the stream's
// launch lock; freed by bpmd_internal_scratch_release.
void* bpmd::pinned_block(hipStream_t s, size_t bytes, PinnedSlot which)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || bytes > 4096) return nullptr;
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    for (auto& e : g_pinned)
        if (e.dev == dev && e.stream == s && e.which == which) return e.p;
    uint8_t* p = nullptr;
    if (hipHostMalloc((void**)&p, 4096, hipHostMallocDefault) != hipSuccess) return nullptr;
    g_pinned.push_back(Scratch{dev, s, which, p, 4096});
    return p;
}
extern "C" size_t bpmd_internal_pinned_count(void)
{
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    return g_pinned.size();
}

// Frees every scratch block and the launch lock of a stream that is about to
// be destroyed (per-stream codecs, batcher slots).  The caller has
// synchronised the stream and no other thread uses it.
extern "C" void bpmd_internal_scratch_release(hipStream_t s)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    bp_release(s);
    hipStream_t side = nullptr;
    {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    for (size_t i = 0; i < g_sides.size(); ++i)
        if (g_sides[i].dev == dev && g_sides[i].stream == s) {
            side = g_sides[i].side;
            (void)hipStreamSynchronize(side);
            (void)hipEventDestroy(g_sides[i].fork);
            (void)hipEventDestroy(g_sides[i].join);
            g_sides[i] = g_sides.back();
            g_sides.pop_back();
            break;
        }
    for (size_t i = 0; i < g_scratch.size();) {
        if (g_scratch[i].dev == dev && (g_scratch[i].stream == s || (side && g_scratch[i].stream == side))) {
            (void)hipFree(g_scratch[i].p);
            g_scratch[i] = g_scratch.back();
            g_scratch.pop_back();
        } else {
            ++i;
        }
    }
    for (size_t i = 0; i < g_pinned.size();) {
        if (g_pinned[i].dev == dev && (g_pinned[i].stream == s || (side && g_pinned[i].stream == side))) {
            (void)hipHostFree(g_pinned[i].p);
            g_pinned[i] = g_pinned.back();
            g_pinned.pop_back();
        } else {
            ++i;
        }
    }
    for (size_t i = 0; i < g_locks.size(); ++i)
        if (g_locks[i].dev == dev && g_locks[i].stream == s) {
            delete g_locks[i].mu;
            g_locks[i] = g_locks.back();
            g_locks.pop_back();
            break;
        }
    }
    if (side) {
        bp_release(side);
        (void)hipStreamDestroy(side);
    }
}

// Number of scratch blocks held (footprint tests)
extern "C" size_t bpmd_internal_scratch_count(void)
{
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    return g_scratch.size();
}

extern "C" const char* bpmd_version(void) { return "beast_pmd 0.2 (gfx950)"; }

// Diagnostics only (scripts/diag_*.py): force the launch grid, e.g. one
// wave, to time a kernel's phases without other waves on the CU.
extern "C" unsigned bpmd_diag_grid_override = 0;
extern "C" void bpmd_diag_set_grid(unsigned grid) { bpmd_diag_grid_override = grid; }

// Kernel choice for a batch: inflate_plan.h.
// BPMD_INFLATE=lane|wave|bp or bpmd_set_inflate_kernel() forces one (the
// tests run all three; "bp" sends every payload of 64 bytes or more through
// the block-parallel path).
static std::atomic<int> g_inflate_kernel{-1};   // -1 unset, 0 auto, 1 lane, 2 wave, 3 bp

extern "C" int bpmd_set_inflate_kernel(int mode)
{
    if (mode < 0 || mode > 3) return BPMD_R_INVALID_ARGUMENT;
    g_inflate_kernel.store(mode);
    return BPMD_R_OK;
}

static int inflate_mode()
{
    int m = g_inflate_kernel.load();
    if (m < 0) {
        const char* e = getenv("BPMD_INFLATE");
        m = (e && !strcmp(e, "lane")) ? 1 : (e && !strcmp(e, "wave")) ? 2 : (e && !strcmp(e, "bp")) ? 3 : 0;
        g_inflate_kernel.store(m);
    }
    return m;
}

extern "C" int bpmd_init(void)
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return BPMD_R_NO_DEVICE;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return BPMD_R_NO_DEVICE;
    std::lock_guard<std::mutex> lk(g_init_mu);
    const uint64_t bit = dev < 64 ? 1ull << dev : 0ull;
    if (g_init_devices & bit) return BPMD_R_OK;
    if (init_fixed() != 0) return BPMD_R_HIP_ERROR;
    g_init_devices |= bit;
    return BPMD_R_OK;
}

// The block-parallel path runs on the caller's stream (batches below 32 Ki
// messages, forced mode) or on its side stream (work-queue batches): both
// get the capacity.
extern "C" int bpmd_inflate_reserve(void* stream, uint64_t in_bytes, uint64_t out_bytes, uint32_t n_long)
{
    int r = bpmd_init();
    if (r) return r;
    const hipStream_t s = (hipStream_t)stream;
    std::mutex* mu = stream_mutex(s);
    if (!mu) return BPMD_R_HIP_ERROR;
    std::lock_guard<std::mutex> launch(*mu);
    Side sd;
    if (!side_for(s, sd)) return BPMD_R_HIP_ERROR;
    if (bp_reserve(s, in_bytes, out_bytes, n_long) || bp_reserve(sd.side, in_bytes, out_bytes, n_long))
        return BPMD_R_HIP_ERROR;
    return BPMD_R_OK;
}

extern "C" size_t bpmd_deflate_upper_bound(size_t n)
{
    // zlib/deflate_stream.hpp:402-410
    return n + ((n + 7) >> 3) + ((n + 63) >> 6) + 11;
}

namespace {

bool batch_has_nulls(const Batch& b)
{
    return !b.in || !b.in_off || !b.in_len || !b.out || !b.out_off || !b.out_cap || !b.out_len || !b.status;
}

// bpmd_inflate_batch and its fused / context-takeover forms.  key: masking
// keys or null; hist: window bytes before each slot (context takeover) or
// null.  inflate_plan.h decides which decoder takes which messages; this
// enqueues the plan's steps in order and returns at the first error.
int inflate_impl(const bpmd_cfg* cfg, const Batch& b, const uint32_t* key, const uint32_t* hist, void* stream)
{
    if (!cfg) return BPMD_R_INVALID_ARGUMENT;
    // inflate_stream.ipp:57-61: windowBits outside 8..15 throws domain_error
    if (cfg->window_bits < 8 || cfg->window_bits > 15) return BPMD_R_DOMAIN_ERROR;
    if (b.n == 0) return BPMD_R_OK;
    if (batch_has_nulls(b)) return BPMD_R_INVALID_ARGUMENT;
    int r = bpmd_init();
    if (r) return r;
    const uint32_t raw = (cfg->flags & BPMD_F_RAW) ? 1u : 0u;
    const hipStream_t s = (hipStream_t)stream;
    std::mutex* mu = stream_mutex(s);
    if (!mu) return BPMD_R_HIP_ERROR;
    std::lock_guard<std::mutex> launch(*mu);
    // every knob is read once, but the split (BPMD_INFLATE_SPLIT) at every call
    static const InflateKnobs latched{env_on("BPMD_INFLATE_BP"), 0u, env_on("BPMD_INFLATE_ORDER"),
                                      env_on("BPMD_INFLATE_LONG"), env_uint("BPMD_LONG_SHARE_PCT", 125u)};
    InflateKnobs knobs = latched;
    knobs.split = env_uint("BPMD_INFLATE_SPLIT", 4096u);
    // 4 workgroups of 64 messages per CU are resident; diagnostics / tests:
    // BPMD_QUEUE_WGS caps the grid so that small batches run through the work
    // queue too
    static const uint32_t q_override = env_uint("BPMD_QUEUE_WGS", 0u);
    const uint32_t wgs = q_override ? q_override : 4u * (uint32_t)cu_count();
    const InflatePlan p = plan_inflate(inflate_mode(), b.n, hist != nullptr, key != nullptr, wgs, knobs);

    uint32_t* qctr = nullptr;
    const uint32_t *order = nullptr, *keys = nullptr, *nlong = nullptr;
    if (p.queue) {
        qctr = (uint32_t*)scratch_block(s, 256, SCR_INFLATE_QUEUE);
        if (!qctr || hipMemsetAsync(qctr, 0, sizeof(uint32_t), s) != hipSuccess) return BPMD_R_HIP_ERROR;
    }
    if (p.order && !(order = lane_order(b.in_len, b.n, s, &keys))) return BPMD_R_HIP_ERROR;
    if (p.longs != InflatePlan::LONG_NONE &&
        !(nlong = bpmd_internal_lane_long_split(b.in_len, keys, b.n, p.split_lanes, p.split_min_thr, p.split_share_pct,
                                                s)))
        return BPMD_R_HIP_ERROR;
    // the long payloads.  On the side stream they decode block-parallel while
    // the lane kernel runs the rest on the caller's stream (it skips the long
    // prefix of the order): each fills the CUs the other's tail leaves idle.
    // (Both enqueue only, except the stream's first block-parallel call
    // without bpmd_inflate_reserve: it reads its workspace totals back once,
    // on the side stream, so it waits for the work queued before it -- and
    // cannot run under stream capture)
    Side sd;
    int e_side = 0;
    if (p.longs == InflatePlan::LONG_BP_INLINE) {
        if (inflate_bp(b, raw, order, nlong, s)) return BPMD_R_HIP_ERROR;
    } else if (p.longs == InflatePlan::LONG_BP_SIDE) {
        if (!side_for(s, sd) || hipEventRecord(sd.fork, s) != hipSuccess ||
            hipStreamWaitEvent(sd.side, sd.fork, 0) != hipSuccess)
            return BPMD_R_HIP_ERROR;
        e_side = inflate_bp(b, raw, order, nlong, sd.side);
    } else if (p.longs == InflatePlan::LONG_WAVE_ORDERED) {
        if (inflate_wave_ordered(b, raw, key, order, nlong, s)) return BPMD_R_HIP_ERROR;
    }
    int e = 0;
    if (p.lanes != InflatePlan::LANES_NONE)
        e = inflate_lane3(b, raw, key, hist, 1u << cfg->window_bits, p.max_in, order, qctr, wgs, nlong, s);
    if (p.longs == InflatePlan::LONG_BP_SIDE) {
        if (hipEventRecord(sd.join, sd.side) != hipSuccess || hipStreamWaitEvent(s, sd.join, 0) != hipSuccess)
            return BPMD_R_HIP_ERROR;
        e = e || e_side;
    }
    if (!e && p.wave != InflatePlan::WAVE_NONE) e = inflate_keyed_split(b, raw, key, p.min_in, s);
    return e ? BPMD_R_HIP_ERROR : BPMD_R_OK;
}

// o: the caller's mask keys, history lengths and chunk-count source; the rest is filled in from cfg
int deflate_impl(const bpmd_cfg* cfg, const Batch& b, DeflateOpts o, void* stream)
{
    if (!cfg) return BPMD_R_INVALID_ARGUMENT;
    // deflate_stream.ipp:235-253: level -1 means 6; windowBits 8 becomes 9;
    // anything outside level 0..9, windowBits 8..15, memLevel 1..9 throws
    // std::invalid_argument.
    int level = cfg->level == -1 ? 6 : cfg->level;
    int wbits = cfg->window_bits == 8 ? 9 : cfg->window_bits;
    if (level < 0 || level > 9 || wbits < 8 || wbits > 15 || cfg->mem_level < 1 || cfg->mem_level > 9)
        return BPMD_R_INVALID_ARGUMENT;
    if (cfg->strategy < BPMD_STRATEGY_NORMAL || cfg->strategy > BPMD_STRATEGY_FIXED) return BPMD_R_INVALID_ARGUMENT;
    if (b.n == 0) return BPMD_R_OK;
    if (batch_has_nulls(b)) return BPMD_R_INVALID_ARGUMENT;
    int r = bpmd_init();
    if (r) return r;
    const hipStream_t s = (hipStream_t)stream;
    std::mutex* mu = stream_mutex(s);
    if (!mu) return BPMD_R_HIP_ERROR;
    std::lock_guard<std::mutex> launch(*mu);
    if (cfg->flags & BPMD_F_EXACT) {
        // the reference's own algorithm, message by message (pmd_deflate_exact.hip)
        if (o.hist_len) return BPMD_R_INVALID_ARGUMENT;
        const int e = deflate_exact(b, level, wbits, cfg->mem_level, cfg->strategy, o.mask_key, s);
        return e ? BPMD_R_HIP_ERROR : BPMD_R_OK;
    }
    o.level = level, o.window_bits = wbits, o.strategy = cfg->strategy;
    return deflate(b, o, s) ? BPMD_R_HIP_ERROR : BPMD_R_OK;
}

}  // namespace

extern "C" int bpmd_inflate_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                                  const uint32_t* d_in_len, uint32_t n_msgs, uint8_t* d_out,
                                  const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                  uint32_t* d_out_len, int32_t* d_status, void* stream)
{
    const Batch b{d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len, d_status};
    return inflate_impl(cfg, b, nullptr, nullptr, stream);
}

extern "C" int bpmd_deflate_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                                  const uint32_t* d_in_len, uint32_t n_msgs, uint8_t* d_out,
                                  const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                  uint32_t* d_out_len, int32_t* d_status, void* stream)
{
    const Batch b{d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len, d_status};
    return deflate_impl(cfg, b, DeflateOpts(), stream);
}

// ------------------------------------------------ frame passes (§8(f) N1)

extern "C" int bpmd_mask_batch(uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len, uint32_t n_msgs,
                               const uint32_t* d_key, const uint8_t* d_phase, void* stream)
{
    if (n_msgs == 0) return BPMD_R_OK;
    if (!d_data || !d_off || !d_len || !d_key) return BPMD_R_INVALID_ARGUMENT;
    int r = bpmd_init();
    if (r) return r;
    return launch_mask(d_data, d_off, d_len, n_msgs, d_key, d_phase, (hipStream_t)stream) ? BPMD_R_HIP_ERROR
                                                                                                 : BPMD_R_OK;
}

// frame.hpp:134-175 header sizes over the write.hpp:463-545 frame loop
extern "C" uint64_t bpmd_frame_wire_size(uint64_t payload_len, uint32_t frame_max, int masked)
{
    if (frame_max == 0) return 0;
    const uint64_t frames = payload_len == 0 ? 1 : (payload_len + frame_max - 1) / frame_max;
    const uint64_t last = payload_len - (frames - 1) * frame_max;
    auto hdr = [&](uint64_t len) -> uint64_t { return (len <= 125 ? 2u : len <= 65535 ? 4u : 10u) + (masked ? 4u : 0u); };
    return payload_len + (frames - 1) * hdr(frame_max) + hdr(last);
}

extern "C" int bpmd_frame_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                const uint8_t* d_op, const uint8_t* d_flags, const uint32_t* d_keys,
                                const uint32_t* d_key_base, uint32_t frame_max, uint32_t n_msgs, uint8_t* d_wire,
                                const uint64_t* d_wire_off, void* stream)
{
    if (n_msgs == 0) return BPMD_R_OK;
    if (!d_in || !d_in_off || !d_in_len || !d_wire || !d_wire_off || frame_max == 0 || (d_keys && !d_key_base))
        return BPMD_R_INVALID_ARGUMENT;
    int r = bpmd_init();
    if (r) return r;
    return launch_frame(d_in, d_in_off, d_in_len, d_op, d_flags, d_keys, d_key_base, frame_max, n_msgs, d_wire,
                               d_wire_off, (hipStream_t)stream)
               ? BPMD_R_HIP_ERROR
               : BPMD_R_OK;
}

// read_some's frame loop over parse_fh (read.hpp:1063-1283, stream_impl.hpp:701-913)
extern "C" int bpmd_unframe_batch(int role, int pmd_on, uint64_t msg_max, const uint8_t* d_wire,
                                  const uint64_t* d_wire_off, const uint32_t* d_wire_len, uint32_t n,
                                  bpmd_rd_state* d_state, uint8_t* d_out, const uint64_t* d_out_off,
                                  const uint32_t* d_out_cap, uint32_t* d_out_len, uint8_t* d_op, uint8_t* d_compressed,
                                  uint8_t* d_event, int32_t* d_status, uint32_t* d_consumed, uint8_t* d_ctl,
                                  uint8_t* d_ctl_len, uint16_t* d_close_code, void* stream)
{
    if (role != BPMD_ROLE_SERVER && role != BPMD_ROLE_CLIENT) return BPMD_R_INVALID_ARGUMENT;
    if (n == 0) return BPMD_R_OK;
    if (!d_wire || !d_wire_off || !d_wire_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_op ||
        !d_compressed || !d_event || !d_status || !d_consumed || !d_ctl || !d_ctl_len || !d_close_code)
        return BPMD_R_INVALID_ARGUMENT;
    int r = bpmd_init();
    if (r) return r;
    return launch_unframe((uint32_t)role, pmd_on ? 1u : 0u, msg_max, d_wire, d_wire_off, d_wire_len, n, d_state, d_out,
                          d_out_off, d_out_cap, d_out_len, d_op, d_compressed, d_event, d_status, d_consumed, d_ctl,
                          d_ctl_len, d_close_code, (hipStream_t)stream)
               ? BPMD_R_HIP_ERROR
               : BPMD_R_OK;
}

extern "C" int bpmd_utf8_check_batch(const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len,
                                     uint32_t n_msgs, int32_t* d_result, void* stream)
{
    if (n_msgs == 0) return BPMD_R_OK;
    if (!d_data || !d_off || !d_len || !d_result) return BPMD_R_INVALID_ARGUMENT;
    int r = bpmd_init();
    if (r) return r;
    return launch_utf8(d_data, d_off, d_len, n_msgs, d_result, nullptr, 0, (hipStream_t)stream)
               ? BPMD_R_HIP_ERROR
               : BPMD_R_OK;
}

extern "C" int bpmd_read_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                               const uint32_t* d_in_len, const uint32_t* d_key, const uint8_t* d_text,
                               uint32_t n_msgs, uint8_t* d_out, const uint64_t* d_out_off,
                               const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status, void* stream)
{
    const Batch b{d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len, d_status};
    int r = inflate_impl(cfg, b, d_key, nullptr, stream);
    if (r || n_msgs == 0 || !d_text) return r;
    // read.hpp:1372-1384: text whose inflated bytes are not UTF-8 fails with bad_frame_payload
    return launch_utf8(d_out, d_out_off, d_out_len, n_msgs, d_status, d_text, BPMD_BAD_FRAME_PAYLOAD,
                              (hipStream_t)stream)
               ? BPMD_R_HIP_ERROR
               : BPMD_R_OK;
}

extern "C" int bpmd_write_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                                const uint32_t* d_in_len, const uint32_t* d_key, uint32_t n_msgs, uint8_t* d_out,
                                const uint64_t* d_out_off, const uint32_t* d_out_cap, uint32_t* d_out_len,
                                int32_t* d_status, void* stream)
{
    const Batch b{d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len, d_status};
    DeflateOpts o;
    o.mask_key = d_key;
    return deflate_impl(cfg, b, o, stream);
}

// ---------------------------------------------- context takeover (§8(f) N3)

extern "C" int bpmd_inflate_takeover_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                                           const uint32_t* d_in_len, const uint32_t* d_hist_len, uint32_t n_msgs,
                                           uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                           uint32_t* d_out_len, int32_t* d_status, void* stream)
{
    const Batch b{d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len, d_status};
    if (n_msgs && !d_hist_len) return BPMD_R_INVALID_ARGUMENT;
    return inflate_impl(cfg, b, nullptr, d_hist_len, stream);
}

extern "C" int bpmd_deflate_takeover_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                                           const uint32_t* d_in_len, const uint32_t* d_hist_len, uint32_t n_msgs,
                                           uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                           uint32_t* d_out_len, int32_t* d_status, void* stream)
{
    const Batch b{d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len, d_status};
    if (n_msgs && !d_hist_len) return BPMD_R_INVALID_ARGUMENT;
    DeflateOpts o;
    o.hist_len = d_hist_len;
    return deflate_impl(cfg, b, o, stream);
}

int bpmd::deflate_takeover_bounded(const bpmd_cfg* cfg, const Batch& b, const DeflateOpts& opts, hipStream_t stream)
{
    if ((b.n && !opts.hist_len) || opts.chunks.kind != dfl::ChunkSource::BOUND || opts.chunks.chunks > 0xFFFFFFFFull)
        return BPMD_R_INVALID_ARGUMENT;
    return deflate_impl(cfg, b, opts, stream);
}

extern "C" int bpmd_slide_batch(uint8_t* d_buf, const uint64_t* d_base, const uint32_t* d_pos, const uint32_t* d_keep,
                                uint32_t n, void* stream)
{
    if (n == 0) return BPMD_R_OK;
    if (!d_buf || !d_base || !d_pos || !d_keep) return BPMD_R_INVALID_ARGUMENT;
    int r = bpmd_init();
    if (r) return r;
    return launch_slide(d_buf, d_base, d_pos, d_keep, n, (hipStream_t)stream) ? BPMD_R_HIP_ERROR : BPMD_R_OK;
}
