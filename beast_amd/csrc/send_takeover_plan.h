// send_takeover_plan.h -- the per-connection rules of the chained send call
// for context-takeover connections (bpmd_send_takeover_batch,
// pmd_send_takeover.hip), on top of send_plan.h's per-message rules: whether
// a message enters the deflater's window at all (begin_msg's decision: an
// uncompressed message never does), how much of a connection's buffer one
// message may claim, where it goes and whether the kept plaintext slides to
// the front first (pmd.py's TakeoverDeflater rule), and how far the position
// advances once the message's frames are on the wire.  Pure functions of one
// connection's values.
// Host-compilable without HIP: tests/test_send_takeover_plan.py compares it
// with a Python model (tests/send_takeover_model.py),
// tests/cpp/send_takeover_plan_main.cpp runs it under the address sanitizer;
// the kernels of pmd_send_takeover.hip call the same functions.
//
// K = the bytes of plaintext a connection's buffer keeps across a slide;
// slot = the bytes of a connection's buffer, more than 2 * K (the entry point
// refuses anything else); pos = the buffer's fill, at most slot: the
// connection's compressed plaintext ends there, and its last min(pos, K) bytes
// are what the next message's matches may reach into.
#pragma once
#include <stdint.h>

#include "deflate_plan.h"
#include "lz_core.h"
#include "send_plan.h"

namespace bpmd {
namespace stp {

constexpr uint32_t K = 4096;   // pmd.TakeoverDeflater.HIST
// the deflater's (deflate_plan.h): chunk_bound(n, L), the most chunks it sees over n entries of <= L bytes
using dfl::CHUNK;
using dfl::chunk_bound;
static_assert(K >= lz::CHUNK_HIST_DEEP && K >= (uint32_t)BPMD_CHUNK_HIST,
              "the buffer keeps at least lz::chunk_hist(level) bytes at every level");

enum : uint32_t { OP_IDLE = 0 };
enum : int32_t { E_MESSAGE_TOO_BIG = 258 };   // BPMD_WS_MESSAGE_TOO_BIG

// The most bytes one compressed message may have: with it the kept plaintext
// and a message always fit behind a slide, K + L <= slot - K.
BPMD_SP_HD uint32_t room(uint32_t max_len, uint32_t slot, uint32_t keep)
{
    const uint32_t most = slot > 2u * keep ? slot - 2u * keep : 0u;
    return max_len < most ? max_len : most;
}

// begin_msg on a takeover connection (pmd_on implied); an idle entry or one
// with a bad opcode decides nothing
BPMD_SP_HD bool deflates(uint32_t op, bool opt, uint64_t len, uint64_t threshold)
{
    return (op == sp::OP_TEXT || op == sp::OP_BINARY) && sp::compress(true, opt, len, threshold);
}

// The status known before the deflater runs.  A message it refuses is not
// sent and reaches the deflater with length 0.
BPMD_SP_HD int32_t provisional(uint32_t op, bool deflates, uint64_t len, uint32_t L)
{
    if (op != OP_IDLE && op != sp::OP_TEXT && op != sp::OP_BINARY) return sp::E_BAD_OPCODE;
    if (deflates && len > L) return E_MESSAGE_TOO_BIG;
    return 0;
}

struct Place {
    uint32_t slide;     // the keep bytes before pos move to the buffer's front first
    uint32_t new_pos;   // where the message goes (the fill after any slide)
    uint32_t z_len;     // the deflater's input length
    uint32_t hist;      // bytes before new_pos its matches may reach into
};

// enters: the entry deflates and was not refused, so len <= L.  It slides
// when the message does not fit behind pos.  Then pos > slot - len >= 2 * keep,
// so keep whole bytes are kept (new_pos = keep) and the source
// [pos - keep, pos) lies at or beyond the destination's end keep: the two
// never overlap.  Any other entry leaves the connection alone and gives the
// deflater nothing: an uncompressed message never passes the peer's inflater,
// so it must not enter this end's window either.
BPMD_SP_HD Place place(uint32_t pos, uint32_t len, uint32_t slot, uint32_t keep, bool enters)
{
    Place p;
    p.slide = 0, p.new_pos = pos, p.z_len = 0, p.hist = 0;
    if (!enters) return p;
    if ((uint64_t)pos + len > slot) p.slide = 1, p.new_pos = keep;
    p.z_len = len;
    p.hist = p.new_pos < keep ? p.new_pos : keep;
    return p;
}

// The status once the deflater has run (zst: its own, looked at for an entry
// that entered only); the wire's E_BUFFER_OVERFLOW comes after it.
BPMD_SP_HD int32_t merge(int32_t provisional, bool enters, int32_t zst)
{
    return provisional ? provisional : enters ? zst : 0;
}

// The fill after the call, from the final status: the message joins the
// history iff its frames are on the wire.  After need_buffers or
// buffer_overflow the peer never saw it, so the history must not hold it.
BPMD_SP_HD uint32_t advance(uint32_t new_pos, uint32_t len, bool enters, int32_t final_status)
{
    return enters && final_status == 0 ? new_pos + len : new_pos;
}

}  // namespace stp
}  // namespace bpmd
