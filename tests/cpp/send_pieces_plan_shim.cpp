// C entry points over beast_amd/csrc/send_pieces_plan.h for
// tests/test_send_pieces_plan.py (plain g++, no HIP): each hands one of the
// header's functions to ctypes.  A state travels as its four bytes.
#include <stdint.h>
#include <string.h>

#include "send_pieces_plan.h"

using namespace bpmd;

static spp::WrState st_of(const uint8_t* s)
{
    spp::WrState w;
    memcpy(&w, s, 4);
    return w;
}

extern "C" uint32_t spp_state_bytes(void) { return (uint32_t)sizeof(spp::WrState); }
extern "C" uint32_t spp_keep(void) { return spp::K; }
// o: compress, op
extern "C" void spp_begin(const uint8_t* state, uint32_t op, int opt, uint64_t len, uint64_t threshold, uint32_t* o)
{
    const spp::Begin b = spp::begin(st_of(state), op, opt != 0, len, threshold);
    o[0] = b.compress, o[1] = b.op;
}
extern "C" int32_t spp_provisional(uint32_t op, int compress, uint64_t len, uint32_t L)
{
    return spp::provisional(op, compress != 0, len, L);
}
extern "C" int32_t spp_status(int32_t prov, int enters, int32_t zst, int fin, uint64_t z_len, uint64_t z_cap)
{
    return spp::status(prov, enters != 0, zst, fin != 0, z_len, z_cap);
}
extern "C" uint64_t spp_payload_len(int compress, int fin, uint64_t len, uint64_t z_len)
{
    return spp::payload_len(compress != 0, fin != 0, len, z_len);
}
extern "C" int spp_frame_first(uint64_t f, int wr_cont) { return spp::frame_first(f, wr_cont != 0) ? 1 : 0; }
extern "C" int spp_frame_fin(uint64_t f, uint64_t frames, int fin) { return spp::frame_fin(f, frames, fin != 0) ? 1 : 0; }
// b: begin's compress, op; o: pos, then the state's four bytes
extern "C" void spp_commit(const uint8_t* state, uint32_t new_pos, uint32_t len, int enters, const uint32_t* b, int idle,
                           int32_t final_status, int fin, int no_takeover, uint32_t* o)
{
    spp::Begin bg;
    bg.compress = b[0], bg.op = b[1];
    const spp::Commit c =
        spp::commit(st_of(state), new_pos, len, enters != 0, bg, idle != 0, final_status, fin != 0, no_takeover != 0);
    o[0] = c.pos, o[1] = c.state.wr_cont, o[2] = c.state.wr_compress, o[3] = c.state.wr_op, o[4] = c.state.reserved;
}
extern "C" uint64_t spp_piece_frame_bound(uint64_t len, uint32_t frame_max, int may_compress, int frag, int fin)
{
    return spp::piece_frame_bound(len, frame_max, may_compress != 0, frag != 0, fin != 0);
}
extern "C" uint64_t spp_piece_wire_bound(uint64_t len, uint32_t frame_max, int masked, int may_compress, int frag,
                                         int fin)
{
    return spp::piece_wire_bound(len, frame_max, masked != 0, may_compress != 0, frag != 0, fin != 0);
}
// the header of frame f of a piece, as send_frame_kernel builds it
extern "C" uint32_t spp_header(uint64_t len, uint64_t f, uint64_t frames, int wr_cont, int fin, int rsv1, uint32_t op,
                               int masked, uint32_t key, uint8_t* out)
{
    uint64_t h0, h1;
    const uint32_t hl = sp::header(len, spp::frame_first(f, wr_cont != 0), spp::frame_fin(f, frames, fin != 0),
                                   rsv1 != 0, op, masked != 0, key, h0, h1);
    for (uint32_t i = 0; i < hl; ++i) out[i] = sp::header_byte(h0, h1, i);
    return hl;
}
