// send_pieces_plan.h -- the rules of the chained send call that takes a
// message in pieces (bpmd_send_pieces_batch, pmd_send_pieces.hip), on top of
// send_plan.h's frame rules and send_takeover_plan.h's connection rules:
// Beast's write_some(fin, buffers) (websocket/impl/write.hpp:625-831) with the
// stream's wr_cont_ / wr_compress_ / opcode kept per connection in a WrState.
// The first piece of a message decides (begin_msg, stream_impl.hpp:225-252,
// with this piece's length as write.hpp:640-652 passes it) and carries the
// opcode; every later piece goes out as continuation frames under the stored
// decision; only the final piece's last frame has FIN.
//
// A compressed piece is deflated like a whole message: its payload ends with
// Flush::sync's empty stored block, the 00 00 FF FF stripped, every block with
// BFINAL = 0 (deflate_plan.h tail_bytes, deflate_writer.h).  A non-final piece
// gets the four bytes back, so the next piece's blocks follow at a byte
// boundary (RFC 7692 7.2.1); the final piece keeps them stripped.  Beast sends
// a non-final piece with Flush::none and may emit nothing (write.hpp:669-678):
// payload bytes differ, the message the peer inflates does not.
// Host-compilable without HIP: tests/test_send_pieces_plan.py compares it with
// a Python model (tests/send_pieces_model.py),
// tests/cpp/send_pieces_plan_main.cpp runs it under the address sanitizer; the
// kernels of pmd_send_pieces.hip call the same functions.
#pragma once
#include <stdint.h>

#include "send_plan.h"
#include "send_takeover_plan.h"

namespace bpmd {
namespace spp {

using stp::K;
using stp::merge;
using stp::place;
using stp::room;

constexpr uint32_t MARKER = 4;   // 00 00 FF FF

// bpmd_wr_state: all zero = no message open
struct WrState {
    uint8_t wr_cont;       // a message is open: the next piece continues it
    uint8_t wr_compress;   // begin_msg's decision for the open message
    uint8_t wr_op;         // its opcode
    uint8_t reserved;
};
static_assert(sizeof(WrState) == 4, "bpmd_wr_state is four bytes");

struct Begin {
    uint32_t compress;   // the message's decision (0 for an idle entry or a bad opcode)
    uint32_t op;         // the message's opcode (the entry's own when it is not 1 or 2)
};

// What this piece is part of.  len: this piece's length.  A continuation
// piece takes the stored decision and opcode: opt is ignored, and op only has
// to be a data opcode.
BPMD_SP_HD Begin begin(const WrState& s, uint32_t op, bool opt, uint64_t len, uint64_t threshold)
{
    Begin b;
    b.compress = 0, b.op = op;
    if (op != sp::OP_TEXT && op != sp::OP_BINARY) return b;
    if (s.wr_cont) b.compress = s.wr_compress != 0, b.op = s.wr_op;
    else b.compress = stp::deflates(op, opt, len, threshold);
    return b;
}

// The status known before the deflater runs: op is the entry's own, len the
// piece's, L stp::room's bound, here on a piece
BPMD_SP_HD int32_t provisional(uint32_t op, bool compress, uint64_t len, uint32_t L)
{
    return stp::provisional(op, compress, len, L);
}

// The status once the deflater has run: stp::merge, and need_buffers for a
// non-final piece whose staging slot cannot take the marker behind the
// deflater's z_len bytes
BPMD_SP_HD int32_t status(int32_t provisional, bool enters, int32_t zst, bool fin, uint64_t z_len, uint64_t z_cap)
{
    const int32_t st = stp::merge(provisional, enters, zst);
    if (st == 0 && enters && !fin && z_len + MARKER > z_cap) return sp::E_NEED_BUFFERS;
    return st;
}

// The bytes of the piece that go on the wire (status 0)
BPMD_SP_HD uint64_t payload_len(bool compress, bool fin, uint64_t len, uint64_t z_len)
{
    return compress ? z_len + (fin ? 0u : MARKER) : len;
}

// Frame f of the piece's `frames`: opcode and RSV1 ride on `first`, see sp::header
BPMD_SP_HD bool frame_first(uint64_t f, bool wr_cont) { return f == 0 && !wr_cont; }
BPMD_SP_HD bool frame_fin(uint64_t f, uint64_t frames, bool fin) { return f + 1 == frames && fin; }

struct Commit {
    uint32_t pos;
    WrState state;
};

// The connection after the call.  new_pos: d_pos after place() (behind any
// slide); idle: the entry's own opcode is 0.  Nothing changes unless the
// piece's frames are on the wire; then the piece joins the history if it
// entered the deflater, the message stays open unless the piece was final,
// and a compressed message's last piece resets the history under
// no_context_takeover (do_context_takeover_write, impl_base.hpp:156-166).
BPMD_SP_HD Commit commit(const WrState& s, uint32_t new_pos, uint32_t len, bool enters, const Begin& b, bool idle,
                         int32_t final_status, bool fin, bool no_takeover)
{
    Commit c;
    c.pos = new_pos, c.state = s;
    if (idle || final_status != 0) return c;
    if (enters) c.pos = new_pos + len;
    c.state.wr_cont = fin ? 0 : 1;
    c.state.wr_compress = b.compress ? 1 : 0;
    c.state.wr_op = (uint8_t)b.op;
    if (fin && b.compress && no_takeover) c.pos = 0;
    return c;
}

// sp::frame_bound / sp::wire_bound for a piece: a non-final compressed piece
// carries the marker.  may_compress: the message may be compressed.
BPMD_SP_HD uint64_t piece_frame_bound(uint64_t len, uint32_t frame_max, bool may_compress, bool frag, bool fin)
{
    const uint64_t plain = sp::split(len, frame_max, false, frag).frames;
    if (!may_compress) return plain;
    const uint64_t z = sp::split(sp::deflate_bound(len) + (fin ? 0u : MARKER), frame_max, true, frag).frames;
    return z > plain ? z : plain;
}
BPMD_SP_HD uint64_t piece_wire_bound(uint64_t len, uint32_t frame_max, bool masked, bool may_compress, bool frag,
                                     bool fin)
{
    const uint64_t plain = sp::wire_size(sp::split(len, frame_max, false, frag), masked);
    if (!may_compress) return plain;
    const uint64_t z =
        sp::wire_size(sp::split(sp::deflate_bound(len) + (fin ? 0u : MARKER), frame_max, true, frag), masked);
    return z > plain ? z : plain;
}

}  // namespace spp
}  // namespace bpmd
