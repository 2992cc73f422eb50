// C entry points over beast_amd/csrc/send_plan.h for tests/test_send_plan.py
// (plain g++, no HIP): each hands one of the header's functions to ctypes.
#include <stdint.h>
#include <string.h>

#include "send_plan.h"

using namespace bpmd::sp;

extern "C" int sp_compress(int pmd_on, int opt, uint64_t len, uint64_t threshold)
{
    return compress(pmd_on != 0, opt != 0, len, threshold);
}
extern "C" uint64_t sp_deflate_bound(uint64_t n) { return deflate_bound(n); }
extern "C" void sp_split(uint64_t len, uint32_t fm, int comp, int frag, uint64_t* o)
{
    const Split s = split(len, fm, comp != 0, frag != 0);
    o[0] = s.frames, o[1] = s.unit, o[2] = s.last;
}
extern "C" uint64_t sp_wire_size(uint64_t len, uint32_t fm, int masked, int comp, int frag)
{
    return wire_size(split(len, fm, comp != 0, frag != 0), masked != 0);
}
// frame f by the closed form: payload offset, wire offset, payload length
extern "C" void sp_frame(uint64_t len, uint32_t fm, int masked, int comp, int frag, uint64_t f, uint64_t* o)
{
    const Split s = split(len, fm, comp != 0, frag != 0);
    o[0] = frame_src(s, f), o[1] = frame_off(s, masked != 0, f), o[2] = frame_len(s, f);
}
extern "C" uint32_t sp_header(uint64_t len, int first, int fin, int rsv1, uint32_t op, int masked, uint32_t key,
                              uint8_t* out14)
{
    uint64_t h0, h1;
    const uint32_t hl = header(len, first != 0, fin != 0, rsv1 != 0, op, masked != 0, key, h0, h1);
    for (uint32_t i = 0; i < hl; ++i) out14[i] = header_byte(h0, h1, i);
    return hl;
}
// A whole message as the frame kernel writes it, frames taken last to first
// so that every one is placed by the closed form alone.  keys NULL = unmasked.
extern "C" uint64_t sp_message(const uint8_t* payload, uint64_t len, uint32_t op, int comp, const uint32_t* keys,
                               uint32_t fm, int frag, uint8_t* out)
{
    const bool masked = keys != nullptr;
    const Split s = split(len, fm, comp != 0, frag != 0);
    for (uint64_t f = s.frames; f-- > 0;) {
        const uint64_t fl = frame_len(s, f);
        const uint32_t key = masked ? keys[f] : 0u;
        uint64_t h0, h1;
        const uint32_t hl = header(fl, f == 0, f + 1 == s.frames, comp != 0, op, masked, key, h0, h1);
        uint8_t* p = out + frame_off(s, masked, f);
        for (uint32_t i = 0; i < hl; ++i) p[i] = header_byte(h0, h1, i);
        const uint8_t* src = payload + frame_src(s, f);
        for (uint64_t t = 0; t < fl; ++t) p[hl + t] = src[t] ^ (uint8_t)(key >> (8 * (t & 3)));
    }
    return wire_size(s, masked);
}
extern "C" uint64_t sp_frame_bound(uint64_t len, uint32_t fm, int may, int frag)
{
    return frame_bound(len, fm, may != 0, frag != 0);
}
extern "C" uint64_t sp_wire_bound(uint64_t len, uint32_t fm, int masked, int may, int frag)
{
    return wire_bound(len, fm, masked != 0, may != 0, frag != 0);
}
// the most frames and wire bytes over both decisions (compressed only when
// `may`) and every deflated length up to deflate_bound(len)
extern "C" void sp_most(uint64_t len, uint32_t fm, int masked, int may, int frag, uint64_t* o)
{
    const Split p = split(len, fm, false, frag != 0);
    uint64_t frames = p.frames, bytes = wire_size(p, masked != 0);
    for (uint64_t z = 0; may && z <= deflate_bound(len); ++z) {
        const Split s = split(z, fm, true, frag != 0);
        const uint64_t w = wire_size(s, masked != 0);
        if (s.frames > frames) frames = s.frames;
        if (w > bytes) bytes = w;
    }
    o[0] = frames, o[1] = bytes;
}
// one control entry: returns the status, *size the frame's bytes written to out (144 bytes)
extern "C" int32_t sp_control(uint32_t op, const uint8_t* slot, uint32_t slot_len, uint32_t code, int masked,
                              uint32_t key, uint8_t* out, uint32_t* size)
{
    uint32_t pl;
    const int32_t st = control_plan(op, slot_len, code, pl);
    *size = st ? 0u : control_size(pl, masked != 0);
    for (uint32_t t = 0; t < *size; ++t) out[t] = control_byte(t, op, pl, code, slot, masked != 0, key);
    return st;
}
extern "C" void sp_constants(uint32_t* o)
{
    o[0] = CTL_SLOT, o[1] = CTL_WIRE, o[2] = CTL_MAX, o[3] = REASON_MAX;
    o[4] = E_NEED_BUFFERS, o[5] = E_BUFFER_OVERFLOW, o[6] = E_BAD_OPCODE, o[7] = E_BAD_CONTROL_SIZE;
}
