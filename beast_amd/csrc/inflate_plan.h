// inflate_plan.h -- which decoder takes which messages of an inflate batch.
// Pure host code without HIP (tests/test_inflate_plan.py compiles it with
// g++); pmd_capi.hip inflate_impl reads the knobs, asks for the plan and
// enqueues its steps.
//
// The decoders: one lane per message (pmd_inflate_lane3.hip) for throughput,
// one wave per message (pmd_inflate.hip) for latency when the batch is too
// small to fill the chip's lanes, and block-parallel decode
// (pmd_inflate_bp.hip) for long payloads.  A lane-kernel wave lasts as long
// as its longest message and a batch of few messages leaves most lanes of
// the chip idle, so in automatic mode only batches of >= 2048 messages use
// lanes at all, and below 32 Ki messages payloads longer than the split
// (compressed bytes; several 4 KiB chunks of output) go elsewhere.  From
// 32 Ki messages on, the lanes fill the chip whatever the sizes: no split,
// and no second launch (C2 +1.6 %, C4 lane-only 23.2 vs 22.6 GiB/s).
#pragma once
#include <stdint.h>

namespace bpmd {

// environment knobs of the automatic choice, with their defaults
struct InflateKnobs {
    bool bp = true;             // BPMD_INFLATE_BP: block-parallel decode of long payloads
    uint32_t split = 4096;      // BPMD_INFLATE_SPLIT: compressed bytes, batches of 2048 to 32 Ki - 1 messages
    bool ordered = true;        // BPMD_INFLATE_ORDER: work-queue batches run longest first
    bool long_split = true;     // BPMD_INFLATE_LONG: payloads too long for one lane leave the work queue
    uint32_t share_pct = 125;   // BPMD_LONG_SHARE_PCT: "too long" for the block-parallel decoder
};

struct InflatePlan {
    // lane kernel: no message, every message (less the long prefix of the
    // order when `longs` is set), or payloads of at most max_in bytes
    enum Lanes { LANES_NONE, LANES_ALL, LANES_UP_TO } lanes = LANES_NONE;
    uint32_t max_in = 0;
    bool queue = false;   // lanes take messages from a work queue, grid of wgs workgroups
    bool order = false;   // the longest-first order is built
    // long payloads (a prefix of the order, counted by
    // bpmd_internal_lane_long_split(split_lanes, split_min_thr, split_share_pct)):
    // block-parallel on the caller's stream before the lane kernel, on the
    // side stream beside it, or one wave each from the order
    enum Longs { LONG_NONE, LONG_BP_INLINE, LONG_BP_SIDE, LONG_WAVE_ORDERED } longs = LONG_NONE;
    uint32_t split_lanes = 0, split_min_thr = 0, split_share_pct = 0;
    // wave kernel after the lanes: nothing, every message, or payloads over min_in bytes
    enum Wave { WAVE_NONE, WAVE_ALL, WAVE_OVER } wave = WAVE_NONE;
    uint32_t min_in = 0;
};

// mode: 0 automatic, 1 lane, 2 wave, 3 bp (every payload of 64 bytes or more
// block-parallel, the rest on lanes; tests).  hist: the batch has takeover
// windows -- only the lane kernel reads a window, so it always runs then.
// key: the batch has masking keys.  wgs: resident lane-kernel workgroups of
// 64 messages.
inline InflatePlan plan_inflate(int mode, uint32_t n_msgs, bool hist, bool key, uint32_t wgs, const InflateKnobs& k)
{
    InflatePlan p;
    auto long_split = [&p](InflatePlan::Longs how, uint32_t lanes, uint32_t min_thr, uint32_t share_pct) {
        p.longs = how;
        p.split_lanes = lanes;
        p.split_min_thr = min_thr;
        p.split_share_pct = share_pct;
    };
    // block-parallel decode applies to plain batches (no takeover window, no
    // masking key: the segment decoder starts mid-payload)
    const bool bp_ok = !hist && !key && ((mode == 0 && k.bp) || mode == 3);
    if (mode == 3 && bp_ok) {
        p.lanes = InflatePlan::LANES_ALL;
        p.order = true;
        long_split(InflatePlan::LONG_BP_INLINE, 0u, 64u, 0u);
        return p;
    }
    if (!(hist || mode == 1 || (mode == 0 && n_msgs >= 2048))) {
        p.wave = InflatePlan::WAVE_ALL;
        return p;
    }
    const uint32_t split = (hist || mode != 0 || n_msgs >= 32768) ? 0u : k.split;
    p.lanes = InflatePlan::LANES_ALL;
    if (n_msgs > wgs * 64u && !split) {
        // more messages than the chip holds lanes: a work queue keeps every
        // lane busy until the batch is done (mixed sizes, configs[3]),
        // longest first, so no lane starts a long message as the batch drains
        p.queue = true;
        p.order = k.ordered;
        // long payloads: block-parallel above 1.25 lanes' share of the batch,
        // from 2 KiB compressed (DESIGN.md 4.1c.  One 8-way C4 shard at 50 /
        // 100 / 150 / 200 %: 9.2 / 8.4-8.9 / 8.3 / 10.5 ms; C4 projected 4- and
        // 8-way speedups at 100 / 125 / 150 %: 3.29-3.30 and 5.29 / 3.36-3.46
        // and 5.30-5.36 / 2.81-2.95 and 5.39-5.45, round 4), or one wave each
        // above twice the share, from 4 KiB
        if (k.ordered && k.long_split && mode == 0 && !hist) {
            if (bp_ok) long_split(InflatePlan::LONG_BP_SIDE, wgs * 64u, 2048u, k.share_pct);
            else long_split(InflatePlan::LONG_WAVE_ORDERED, wgs * 64u, 4096u, 200u);
        }
    } else if (split && bp_ok) {
        // payloads over the split: block-parallel; the rest on lanes, in the
        // same longest-first order after them
        p.order = true;
        long_split(InflatePlan::LONG_BP_INLINE, 0u, split, 0u);
    } else if (split) {
        // payloads over the split: one wave each
        p.lanes = InflatePlan::LANES_UP_TO;
        p.max_in = split;
        p.wave = InflatePlan::WAVE_OVER;
        p.min_in = split;
    }
    return p;
}

}  // namespace bpmd
