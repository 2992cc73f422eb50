// A byte-serial stitch on the host over beast_amd/csrc/deflate_plan.h, for
// tests/test_deflate_plan.py (through tests/cpp/deflate_plan_shim.cpp) and
// tests/cpp/deflate_plan_main.cpp.  Which chunk gets a marker, where every
// byte goes, how much room each step asks for, the next bit position and the
// tail are the header's, called in the order stitch_kernel calls them; the
// loops that move the bytes are this file's own (a Huffman-coded block goes
// over bit by bit, not by the kernel's shift-merge).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "deflate_plan.h"

namespace dp_test {

enum : int32_t { OK = 0, NEED_BUFFERS = 1, BROKEN = 99 };   // BROKEN: the plan contradicts itself

struct Stitched {
    int32_t status;
    uint32_t out_len, out_bits;
};

// nk chunk blocks, chunk k's slot at slots + k * stride and its word words[k],
// into o[0, cap) masked with key
inline Stitched stitch(const uint8_t* slots, size_t stride, const uint32_t* words, uint32_t nk, uint8_t* o, uint32_t cap,
                       uint32_t key)
{
    using namespace bpmd::dfl;
    auto km = [&](uint32_t p) { return (uint8_t)(key >> (8 * (p & 3))); };
    uint32_t bit = 0, cv = 0;
    bool overflow = false, broken = false;
    auto head = [&](const StoredSpan& s) {
        if (s.at != bit >> 3 || s.pay - s.at < 1 || s.pay - s.at > 2) broken = true;
        o[s.at] = (uint8_t)(cv ^ km(s.at));
        for (uint32_t p = s.at + 1; p < s.pay; ++p) o[p] = km(p);
        cv = 0;
    };
    for (uint32_t c = 0; c < nk; ++c) {
        const uint32_t w = words[c];
        const uint8_t* t = slots + c * stride;
        const bool stored = (w & W_STORED) != 0;
        const uint32_t nbits = w & ~W_STORED;
        if (w == W_OVERFLOW) { overflow = true; break; }
        if (marker_before(c, stored)) {
            const StoredSpan m = stored_span(bit, 4);
            if (m.room > cap) { overflow = true; break; }
            head(m);
            for (uint32_t j = 0; j < m.nbytes; ++j) o[m.pay + j] = (uint8_t)((j < 2 ? 0x00 : 0xff) ^ km(m.pay + j));
            bit = m.next;
        }
        if (stored) {
            const StoredSpan s = stored_span(bit, nbits / 8 - 1);
            if (s.room > cap) { overflow = true; break; }
            head(s);
            for (uint32_t j = 0; j < s.nbytes; ++j) o[s.pay + j] = (uint8_t)(t[1 + j] ^ km(s.pay + j));
            bit = s.next;
        } else {
            const HuffSpan h = huff_span(bit, nbits);
            if (h.room > cap) { overflow = true; break; }
            if (h.at != bit >> 3 || h.shift != (bit & 7)) broken = true;
            uint32_t done = 0;
            for (uint32_t b = 0; b < nbits; ++b, ++bit) {
                cv |= (uint32_t)((t[b >> 3] >> (b & 7)) & 1) << (bit & 7);
                if ((bit & 7) == 7) {
                    o[bit >> 3] = (uint8_t)(cv ^ km(bit >> 3));
                    cv = 0;
                    ++done;
                }
            }
            if (bit != h.next || done != h.full || h.slot_bytes != (nbits + 7) / 8) broken = true;
        }
    }
    Stitched r = {OK, 0, 0};
    const uint32_t olen = tail_out_len(bit >> 3, bit & 7);
    if (!overflow && olen > cap) overflow = true;
    if (broken) {
        r.status = BROKEN;
    } else if (overflow) {
        r.status = NEED_BUFFERS;
    } else {
        o[bit >> 3] = (uint8_t)(cv ^ km(bit >> 3));
        if (tail_bytes(bit & 7) == 2) o[(bit >> 3) + 1] = km((bit >> 3) + 1);
        r.out_len = olen;
        r.out_bits = bit;
    }
    return r;
}

}  // namespace dp_test
