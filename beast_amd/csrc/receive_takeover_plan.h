// receive_takeover_plan.h -- the per-connection rules of the chained receive
// call for context-takeover connections (bpmd_receive_takeover_batch,
// pmd_receive_takeover.hip), on top of receive_plan.h's per-entry rules: how
// much of a connection's buffer one message may claim, where the next message
// goes and whether the window slides to the front first (pmd.py's
// TakeoverInflater rule), and how far the position advances afterwards.  Pure
// functions of one connection's values.
// Host-compilable without HIP: tests/test_receive_takeover_plan.py compares it
// with a Python model (tests/receive_takeover_model.py),
// tests/cpp/receive_takeover_plan_main.cpp runs it under the address
// sanitizer; the kernels of pmd_receive_takeover.hip call the same functions.
//
// W = 1 << window_bits; slot = the bytes of a connection's buffer, more than
// 2 * W (the entry point refuses anything else); pos = the buffer's fill, at
// most slot: the connection's latest output ends there, and its last
// min(pos, W) bytes are the inflater's window.
#pragma once
#include <stdint.h>

#include "receive_plan.h"

namespace bpmd {
namespace rtp {

// The most bytes one message may claim: "the message capacity" of every rule
// of receive_plan.h (effective_cap, and merge's choice between
// message_too_big and buffer_overflow) is this clamped value.  With it a
// window and a message always fit behind a slid window: W + room <= slot - W.
BPMD_RP_HD uint32_t room(uint32_t msg_cap, uint32_t slot, uint32_t W)
{
    const uint32_t most = slot > 2u * W ? slot - 2u * W : 0u;
    return msg_cap < most ? msg_cap : most;
}

struct Place {
    uint32_t slide;     // the W bytes before pos move to the buffer's front first
    uint32_t new_pos;   // where the message goes (the fill after any slide)
    uint32_t hist;      // the inflater's window: bytes before new_pos it may copy from
};

// eff_cap: rp::select's effective capacity under room().  Only an entry that
// is inflated can slide, when its capacity does not fit behind pos.  Then
// pos > slot - eff_cap >= 2 * W, so a whole window is kept (new_pos = W) and
// the source [pos - W, pos) lies at or beyond the destination's end W: the two
// never overlap.  An entry that is not inflated leaves the connection alone
// and gives the inflater no window.
BPMD_RP_HD Place place(uint32_t pos, uint32_t eff_cap, uint32_t slot, uint32_t W, bool inflates)
{
    Place p;
    p.slide = 0, p.new_pos = pos, p.hist = 0;
    if (!inflates) return p;
    if ((uint64_t)pos + eff_cap > slot) p.slide = 1, p.new_pos = W;
    p.hist = p.new_pos < W ? p.new_pos : W;
    return p;
}

// The fill after the call.  zst, z_len: the inflater's own status and output
// length.  What it produced with status 0 is in the window whatever the merged
// status says afterwards (message_too_big, bad_frame_payload): Beast's
// inflater has taken those bytes too.  After any other inflater status the
// position stays; the window is undefined from then on.
BPMD_RP_HD uint32_t advance(uint32_t pos, bool inflates, int32_t zst, uint32_t z_len)
{
    return inflates && zst == 0 ? pos + z_len : pos;
}

}  // namespace rtp
}  // namespace bpmd
