// receive_pieces_plan.h -- the rules of the chained receive call that hands a
// message over in pieces (bpmd_receive_pieces_batch, pmd_receive_pieces.hip):
// read_some's state between calls (websocket/impl/read.hpp:1063-1385 around
// stream_impl.hpp:78-87), on top of frame_parse.h's header step, which is used
// unchanged.  Pure functions of one connection's values:
//
//   rot_key      the frame key after n payload bytes (mask.ipp:29-36)
//   walk         fp::walk for partial data frames: what one call gathers
//   limit_room   the inflater's output room under what is left of rd_msg_max
//   merge        the status of a compressed piece from the inflater's Result
//   utf8_head    the carried code point finished over a piece's first bytes
//   utf8_tail    the carry a piece's last bytes leave
//   commit       the state after the call
//
// A piece is what one call gathered of one message, whatever stopped the walk.
// Host-compilable without HIP: tests/test_receive_pieces_plan.py compares it
// with a Python model (tests/receive_pieces_model.py),
// tests/cpp/receive_pieces_plan_main.cpp fuzzes it under the address
// sanitizer; the kernels of pmd_receive_pieces.hip call the same functions.
#pragma once
#include <stdint.h>

#include "frame_parse.h"
#include "receive_plan.h"

namespace bpmd {
namespace rpp {

// The C ABI's bpmd_rd_piece_state.  All zero = between messages.
struct PieceState {
    uint64_t rd_size;     // bytes of the current message delivered so far (gathered if plain, inflated if compressed)
    uint64_t rd_remain;   // payload bytes of the current data frame still to come
    uint32_t rd_key;      // that frame's key, byte 0 applying to its next payload byte
    uint8_t rd_cont, rd_op, rd_deflated;
    uint8_t rd_fin;       // FIN of the frame rd_remain belongs to
    uint8_t utf8_n;       // 0..3: bytes of a code point the text delivered so far ends inside
    uint8_t utf8_b[3];
    uint8_t reserved[4];
};
static_assert(sizeof(PieceState) == 32, "PieceState is 32 bytes");

constexpr uint32_t TAIL = 4;      // 00 00 FF FF behind a compressed message's last piece
constexpr uint32_t MIN_CAP = 8;   // an out slot below this gathers nothing

// the key for the payload bytes after the first n: prepared-key rotation, n mod 4 bytes
BPMD_HD uint32_t rot_key(uint32_t key, uint64_t n)
{
    const uint32_t r = 8u * (uint32_t)(n & 3u);
    return r ? (key >> r) | (key << (32u - r)) : key;
}

struct Stop {
    uint32_t piece_len;   // payload bytes gathered in this call, from offset 0 of the out slot
    uint32_t consumed;    // wire bytes taken: headers, payload parts, a whole control frame
    uint32_t event;       // fp::EV_*; EV_MESSAGE: the FIN frame's last payload byte was taken
    int32_t status;       // 0, a refused header's error, read_close's, or E_BUFFER_OVERFLOW for a slot below MIN_CAP
    uint32_t msg_op, msg_deflated;
    uint32_t tail;        // TAIL bytes were appended behind the piece
    uint32_t ctl_len;
    uint16_t close_code;
};

// One entry of bpmd_receive_pieces_batch: fp::walk over the wl bytes at p with
// the data frames taken as far as the bytes and the slot go.  put_data(at, src,
// len, key) stores len unmasked payload bytes at offset `at` of the out slot
// (key's byte 0 applies to src[0]); put_ctl(src, len, key) stores a control
// payload; put_tail(at) stores 00 00 FF FF at offset `at`.  Stores stay below
// cap: at + len <= cap - TAIL for data, at + TAIL <= cap for the tail.  On
// EV_MESSAGE the state still names the finished message (rd_fin = 1, rd_remain
// = 0); commit() resets it once the piece has been looked at.
template <class PutData, class PutCtl, class PutTail>
BPMD_HD void walk(const uint8_t* p, uint32_t wl, uint32_t role, bool pmd_on, uint64_t msg_max, uint32_t cap,
                  PieceState& st, PutData put_data, PutCtl put_ctl, PutTail put_tail, Stop& s)
{
    uint32_t pos = 0, got = 0;
    s.event = fp::EV_NEED_MORE;
    s.status = 0;
    s.tail = 0;
    s.ctl_len = 0;
    s.close_code = 0;
    if (cap < MIN_CAP) s.status = fp::E_BUFFER_OVERFLOW;
    const uint32_t room = cap < MIN_CAP ? 0u : cap - TAIL;
    bool in_frame = st.rd_remain > 0;
    while (s.status == 0) {
        if (in_frame) {   // read.hpp:1201-1280: what has arrived of the frame's payload
            uint64_t take = st.rd_remain;
            if (take > wl - pos) take = wl - pos;
            if (take > room - got) take = room - got;
            if (take) {
                put_data(got, p + pos, (uint32_t)take, st.rd_key);
                st.rd_key = rot_key(st.rd_key, take);
                st.rd_remain -= take;
                if (!st.rd_deflated) st.rd_size += take;
                pos += (uint32_t)take, got += (uint32_t)take;
            }
            if (st.rd_remain) break;   // end of bytes or slot full
            in_frame = false;
            if (st.rd_fin) {   // read.hpp:1281-1283
                s.event = fp::EV_MESSAGE;
                if (st.rd_deflated) put_tail(got), s.tail = 1;
                break;
            }
            continue;
        }
        fp::RdState v;
        v.rd_size = st.rd_size, v.rd_cont = st.rd_cont, v.rd_op = st.rd_op, v.rd_deflated = st.rd_deflated;
        fp::Header h;
        const int32_t r = fp::parse_fh(p + pos, wl - pos, role, pmd_on, msg_max, ~(uint64_t)0, v, h);
        if (r == fp::NEED_MORE) break;
        if (r != fp::FRAME) {
            s.status = r;
            break;
        }
        if (fp::is_control(h.op)) {   // stays whole (stream_impl.hpp:817-823)
            if (h.len > (uint64_t)(wl - pos - h.hdr_len)) break;
            const uint8_t* src = p + pos + h.hdr_len;
            const uint32_t len = (uint32_t)h.len, key = h.key;
            pos += h.hdr_len + len;
            put_ctl(src, len, key);
            s.ctl_len = len;
            s.event = h.op == fp::OP_PING ? fp::EV_PING : h.op == fp::OP_PONG ? fp::EV_PONG : fp::EV_CLOSE;
            if (h.op == fp::OP_CLOSE)
                s.status = fp::read_close(
                    [&](uint32_t i) { return (uint32_t)(uint8_t)(src[i] ^ (uint8_t)(key >> (8 * (i & 3u)))); }, len,
                    s.close_code);
            break;
        }
        if (h.op != fp::OP_CONT) {   // stream_impl.hpp:877-909
            st.rd_size = 0;
            st.rd_op = h.op;
            st.rd_deflated = pmd_on && h.rsv1;
        }
        st.rd_cont = !h.fin;
        st.rd_fin = h.fin;
        st.rd_remain = h.len;
        st.rd_key = h.key;
        pos += h.hdr_len;
        in_frame = true;
    }
    s.piece_len = got;
    s.consumed = pos;
    s.msg_op = st.rd_op, s.msg_deflated = st.rd_deflated;
}

// The piece reaches the inflater: compressed, and not an empty piece in the
// middle of a message (an empty last piece still brings the tail).
BPMD_RP_HD bool inflates(uint32_t deflated, uint32_t piece_len, uint32_t tail)
{
    return deflated != 0 && (piece_len != 0 || tail != 0);
}

// rp::effective_cap on what is left of the limit: one byte past it tells a
// message over the limit from one that reaches it.
BPMD_RP_HD uint32_t limit_room(uint32_t msg_cap, uint64_t msg_max, uint64_t rd_size)
{
    if (msg_max == 0) return msg_cap;
    const uint64_t left = rd_size < msg_max ? msg_max - rd_size : 0u;
    if (left >= 0xffffffffull) return msg_cap;
    const uint32_t limit = (uint32_t)left + 1u;
    return msg_cap < limit ? msg_cap : limit;
}

// A compressed piece's status, in stream order: the state machine's error
// (need_buffers is a call without progress, no error of the stream), the limit
// on the inflated running size (read.hpp:1361-1367), the room that ran out
// with input left.
BPMD_RP_HD int32_t merge(int32_t ec, uint64_t in_used, uint64_t n_in, uint64_t out_used, uint64_t rd_size,
                         uint64_t msg_max)
{
    if (ec != 0 && ec != rp::E_NEED_BUFFERS) return ec;
    if (msg_max && (rd_size > msg_max || out_used > msg_max - rd_size)) return rp::E_MESSAGE_TOO_BIG;
    if (in_used < n_in) return rp::E_BUFFER_OVERFLOW;
    return 0;
}

// utf8_checker's valid() and fail_fast() over the k (1..4) bytes b of one code
// point that needs `need` (utf8_checker.ipp:43-157): false when they are no
// prefix of a well-formed code point
BPMD_RP_HD bool utf8_prefix_ok(const uint8_t* b, uint32_t k, uint32_t need)
{
    const uint32_t c = b[0];
    if (need == 2 && c < 0xc2) return false;
    if (need == 4 && c > 0xf4) return false;
    if (k >= 2) {
        uint32_t lo = 0x80, hi = 0xbf;
        if (c == 0xe0) lo = 0xa0;
        if (c == 0xed) hi = 0x9f;
        if (c == 0xf0) lo = 0x90;
        if (c == 0xf4) hi = 0x8f;
        if (b[1] < lo || b[1] > hi) return false;
    }
    for (uint32_t i = 2; i < k; ++i)
        if ((b[i] & 0xc0u) != 0x80u) return false;
    return true;
}

// bytes of the code point a lead byte starts; 0: no lead
BPMD_RP_HD uint32_t utf8_need(uint32_t c) { return c < 0x80 ? 1u : c < 0xc0 ? 0u : c < 0xe0 ? 2u : c < 0xf0 ? 3u : c < 0xf8 ? 4u : 0u; }

struct Utf8Head {
    uint32_t bad;    // the carry and the piece's first bytes are no prefix of a code point
    uint32_t skip;   // piece bytes that finish the carried code point: the wave's check starts behind them
    uint8_t n;       // the carry after the piece, when the piece ends inside the carried code point still
    uint8_t b[3];
};

// utf8_checker::write's "finish up any incomplete code point" (:176-206):
// the carry cb[0..cn) followed by the piece's bytes get(0..len)
template <class Get>
BPMD_RP_HD Utf8Head utf8_head(uint32_t cn, const uint8_t* cb, Get get, uint32_t len)
{
    Utf8Head r;
    r.bad = 0, r.skip = 0, r.n = 0, r.b[0] = r.b[1] = r.b[2] = 0;
    if (cn == 0) return r;
    uint8_t cp[4] = {0, 0, 0, 0};
    uint32_t k = cn > 3 ? 3 : cn;
    for (uint32_t i = 0; i < k; ++i) cp[i] = cb[i];
    const uint32_t need = utf8_need(cp[0]);
    if (need < 2 || k >= need) {   // no carry a call of this library leaves
        r.bad = 1;
        return r;
    }
    while (k < need && r.skip < len) cp[k++] = (uint8_t)get(r.skip++);
    if (!utf8_prefix_ok(cp, k, need)) r.bad = 1;
    else if (k < need) {
        r.n = (uint8_t)k;
        for (uint32_t i = 0; i < k; ++i) r.b[i] = cp[i];
    }
    return r;
}

// The carry a piece leaves: get(0..len) are the piece's bytes behind
// utf8_head's skip, already found to be a prefix of well-formed UTF-8; the
// last code point may be cut.  n = 0: the piece ends on a code point's edge.
template <class Get>
BPMD_RP_HD Utf8Head utf8_tail(Get get, uint32_t len)
{
    Utf8Head r;
    r.bad = 0, r.skip = 0, r.n = 0, r.b[0] = r.b[1] = r.b[2] = 0;
    for (uint32_t k = 1; k <= 3 && k <= len; ++k) {
        const uint32_t c = get(len - k);
        if ((c & 0xc0u) == 0x80u) continue;   // a continuation: the lead lies further back
        if (utf8_need(c) > k) {
            r.n = (uint8_t)k;
            for (uint32_t i = 0; i < k; ++i) r.b[i] = (uint8_t)get(len - k + i);
        }
        break;
    }
    return r;
}

// The state after the call.  last: the walk reported EV_MESSAGE; delivered:
// the inflated bytes of a compressed piece (read.hpp:1369; the walk has counted
// a plain piece itself); n, b: the new UTF-8 carry.  A message's end is
// fp::reset with the carry cleared.
BPMD_RP_HD void commit(PieceState& st, bool last, uint64_t delivered, uint32_t n, const uint8_t* b)
{
    if (last) {
        st = PieceState{};
        return;
    }
    if (st.rd_deflated) st.rd_size += delivered;
    st.utf8_n = (uint8_t)n;
    for (uint32_t i = 0; i < 3; ++i) st.utf8_b[i] = i < n ? b[i] : (uint8_t)0;
}

}  // namespace rpp
}  // namespace bpmd
