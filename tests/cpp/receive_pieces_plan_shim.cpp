// C entry points over beast_amd/csrc/receive_pieces_plan.h for
// tests/test_receive_pieces_plan.py (plain g++, no HIP): each hands one of the
// header's functions its arguments and returns what it gives; rpp_walk runs
// the walk with byte-by-byte callbacks over the caller's slots.
#include <stdint.h>
#include <string.h>

#include "receive_pieces_plan.h"

using namespace bpmd;

struct WalkOut {
    uint32_t piece_len, consumed, event;
    int32_t status;
    uint32_t msg_op, msg_deflated, tail, ctl_len, close_code;
};

extern "C" {

uint32_t rpp_state_bytes() { return (uint32_t)sizeof(rpp::PieceState); }
uint32_t rpp_rot_key(uint32_t key, uint64_t n) { return rpp::rot_key(key, n); }

// out: cap bytes, ctl: 128 bytes
void rpp_walk(const uint8_t* p, uint32_t wl, uint32_t role, int pmd_on, uint64_t msg_max, uint32_t cap, void* state,
              uint8_t* out, uint8_t* ctl, WalkOut* w)
{
    rpp::PieceState st;
    memcpy(&st, state, sizeof st);
    rpp::Stop s;
    rpp::walk(
        p, wl, role, pmd_on != 0, msg_max, cap, st,
        [&](uint32_t at, const uint8_t* src, uint32_t len, uint32_t key) {
            for (uint32_t t = 0; t < len; ++t) out[at + t] = src[t] ^ (uint8_t)(key >> (8 * (t & 3u)));
        },
        [&](const uint8_t* src, uint32_t len, uint32_t key) {
            for (uint32_t t = 0; t < len; ++t) ctl[t] = src[t] ^ (uint8_t)(key >> (8 * (t & 3u)));
        },
        [&](uint32_t at) {
            out[at] = out[at + 1] = 0;
            out[at + 2] = out[at + 3] = 0xff;
        },
        s);
    memcpy(state, &st, sizeof st);
    *w = WalkOut{s.piece_len, s.consumed, s.event, s.status, s.msg_op, s.msg_deflated, s.tail, s.ctl_len, s.close_code};
}

int rpp_inflates(uint32_t deflated, uint32_t piece_len, uint32_t tail) { return rpp::inflates(deflated, piece_len, tail); }
uint32_t rpp_limit_room(uint32_t msg_cap, uint64_t msg_max, uint64_t rd_size)
{
    return rpp::limit_room(msg_cap, msg_max, rd_size);
}
int32_t rpp_merge(int32_t ec, uint64_t in_used, uint64_t n_in, uint64_t out_used, uint64_t rd_size, uint64_t msg_max)
{
    return rpp::merge(ec, in_used, n_in, out_used, rd_size, msg_max);
}

// r: bad, skip, n, b[0..3)
void rpp_utf8_head(uint32_t cn, const uint8_t* cb, const uint8_t* piece, uint32_t len, uint8_t* r)
{
    const rpp::Utf8Head h = rpp::utf8_head(cn, cb, [&](uint32_t i) { return (uint32_t)piece[i]; }, len);
    r[0] = (uint8_t)h.bad, r[1] = (uint8_t)h.skip, r[2] = h.n, r[3] = h.b[0], r[4] = h.b[1], r[5] = h.b[2];
}
void rpp_utf8_tail(const uint8_t* piece, uint32_t len, uint8_t* r)
{
    const rpp::Utf8Head h = rpp::utf8_tail([&](uint32_t i) { return (uint32_t)piece[i]; }, len);
    r[0] = (uint8_t)h.bad, r[1] = (uint8_t)h.skip, r[2] = h.n, r[3] = h.b[0], r[4] = h.b[1], r[5] = h.b[2];
}
void rpp_commit(void* state, int last, uint64_t delivered, uint32_t n, const uint8_t* b)
{
    rpp::PieceState st;
    memcpy(&st, state, sizeof st);
    rpp::commit(st, last != 0, delivered, n, b);
    memcpy(state, &st, sizeof st);
}
}
