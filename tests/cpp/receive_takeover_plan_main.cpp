// The connection rules of the chained takeover receive
// (beast_amd/csrc/receive_takeover_plan.h) under -fsanitize=address,undefined:
// place, slide, inflate, advance run on the host for many random rounds with a
// stand-in inflater (it reads its whole window, writes what it produces and
// stops at its capacity with need_buffers, as the real one does).  Every
// connection's buffer is a heap block of exactly `slot` bytes, so one byte
// read or written outside it aborts the program, and the slide is a memcpy,
// whose overlapping arguments the sanitizer reports too.  A second copy of
// each connection's stream, kept as one growing string, says what the window
// must hold.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>

#include "receive_takeover_plan.h"

using namespace bpmd;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            if (failures++ < 10) printf("line %d: %s\n", __LINE__, #c); \
        }                                                         \
    } while (0)

static std::mt19937_64 rng(20241027);
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }

struct Conn {
    uint8_t* buf;         // exactly slot bytes
    uint32_t pos = 0;
    std::string stream;   // everything the inflater has produced with status 0
};

// one call on one connection; total: what the message inflates to; zerr: a zlib error met after `before` bytes
static void one_call(Conn& c, uint32_t slot, uint32_t W, uint32_t event, int32_t fst, uint32_t compressed,
                     uint32_t msg_cap, uint64_t msg_max, uint32_t total, int32_t zerr, uint32_t before, int& slides)
{
    const uint32_t cap = rtp::room(msg_cap, slot, W);
    CHECK(cap <= msg_cap && cap <= slot - 2 * W);
    const bool z = rp::inflates(event, fst, compressed);
    const rp::Select s = rp::select(event, fst, compressed, 2, 10, cap, msg_max);
    const rtp::Place pl = rtp::place(c.pos, s.eff_cap, slot, W, z);
    CHECK(z || (!pl.slide && pl.new_pos == c.pos && pl.hist == 0 && s.eff_cap == 0));
    if (pl.slide) {
        CHECK(pl.new_pos == W && c.pos >= 2 * W && c.pos <= slot);
        memcpy(c.buf, c.buf + c.pos - W, W);   // [pos - W, pos) -> [0, W)
        ++slides;
    }
    CHECK(!z || pl.hist == (pl.new_pos < W ? pl.new_pos : W));
    CHECK((uint64_t)pl.new_pos + s.eff_cap <= slot);
    uint32_t z_len = 0;
    int32_t zst = 0;
    if (z) {
        // the window is the tail of the connection's stream
        const uint8_t* win = c.buf + pl.new_pos - pl.hist;
        const size_t have = c.stream.size() < pl.hist ? c.stream.size() : pl.hist;
        CHECK(have == pl.hist || c.stream.size() == pl.new_pos);
        CHECK(memcmp(win + pl.hist - have, c.stream.data() + c.stream.size() - have, have) == 0);
        uint32_t sum = 0;
        for (uint32_t i = 0; i < pl.hist; ++i) sum += win[i];
        const uint32_t want = zerr ? (before < total ? before : total) : total;
        z_len = want < s.eff_cap ? want : s.eff_cap;
        for (uint32_t i = 0; i < z_len; ++i) c.buf[pl.new_pos + i] = (uint8_t)(sum + 31 * i + rnd(7));
        zst = want > s.eff_cap ? rp::E_NEED_BUFFERS : zerr;
        if (zst == 0) c.stream.append((const char*)c.buf + pl.new_pos, z_len);
    }
    const uint32_t p1 = rtp::advance(pl.new_pos, z, zst, z_len);
    CHECK(p1 == (z && zst == 0 ? pl.new_pos + z_len : pl.new_pos) && p1 <= slot);
    CHECK(z || p1 == c.pos);
    const rp::Merge m = rp::merge(event, fst, compressed, 2, 10, z ? cap : 0u, msg_max, zst, z_len);
    if (z && zst == 0 && msg_max && total > msg_max) CHECK(m.status == rp::E_MESSAGE_TOO_BIG && p1 == pl.new_pos + z_len);
    if (z && zst == rp::E_NEED_BUFFERS)
        CHECK(m.status == (msg_max && msg_max <= cap ? rp::E_MESSAGE_TOO_BIG : rp::E_BUFFER_OVERFLOW) && p1 == pl.new_pos);
    c.pos = p1;
}

int main()
{
    int calls = 0, slides = 0;
    for (uint32_t wbits : {8u, 9u, 12u}) {
        const uint32_t W = 1u << wbits;
        for (uint32_t extra : {1u, 2u, 100u, W, 3 * W + 5}) {
            const uint32_t slot = 2 * W + extra;
            Conn conns[6];
            for (Conn& c : conns) c.buf = (uint8_t*)malloc(slot);
            for (int round = 0; round < 400; ++round)
                for (Conn& c : conns) {
                    const uint32_t caps[] = {0, 1, extra - 1, extra, extra + 1, slot, 0xffffffffu};
                    const uint32_t msg_cap = caps[rnd(7)];
                    const uint64_t maxes[] = {0, 1, extra - 1, extra, extra + 1, 0xffffffffull, ~0ull};
                    const uint32_t total = rnd(4) ? rnd(extra + 3) : rnd(8);
                    const int32_t zerr = rnd(16) ? 0 : 13;
                    const uint32_t event = rnd(8) ? 1u : rnd(5);
                    const std::string kept = c.stream;
                    const uint32_t pos0 = c.pos;
                    one_call(c, slot, W, event, rnd(10) ? 0 : 262, rnd(5) ? 1u : 0u, msg_cap, maxes[rnd(7)], total, zerr,
                             zerr ? rnd(total + 1) : 0u, slides);
                    CHECK(c.pos >= pos0 || c.pos >= W);
                    CHECK(c.stream.size() >= kept.size());
                    ++calls;
                }
            for (Conn& c : conns) free(c.buf);
        }
    }
    CHECK(slides > 100);
    printf("%d calls, %d slides, %d failures\n", calls, slides, failures);
    return failures ? 1 : 0;
}
