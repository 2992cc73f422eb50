// The connection rules of the chained takeover send
// (beast_amd/csrc/send_takeover_plan.h) under -fsanitize=address,undefined:
// decide, place, slide, copy, deflate, advance run on the host for many random
// rounds with a stand-in deflater (it reads its whole history and its whole
// message and reports need_buffers now and then, as the real one can).  Every
// connection's buffer is a heap block of exactly `slot` bytes, so one byte
// read or written outside it aborts the program, and the slide is a memcpy,
// whose overlapping arguments the sanitizer reports too.  A second copy of
// each connection's compressed plaintext, kept as one growing string, says
// what the history must hold.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>

#include "send_takeover_plan.h"

using namespace bpmd;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            if (failures++ < 10) printf("line %d: %s\n", __LINE__, #c); \
        }                                                         \
    } while (0)

static std::mt19937_64 rng(20241103);
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }

struct Conn {
    uint8_t* buf;         // exactly slot bytes
    uint32_t pos = 0;
    std::string stream;   // every message the peer's inflater has seen
};

// one call on one connection; zst: what the deflater reports, wire_ok: the frames fit the wire
static void one_call(Conn& c, uint32_t slot, uint32_t max_len, uint32_t op, bool opt, uint64_t threshold,
                     const std::string& msg, int32_t zst, bool wire_ok, int& slides, uint64_t& chunks)
{
    const uint32_t K = stp::K, len = (uint32_t)msg.size();
    const uint32_t L = stp::room(max_len, slot, K);
    CHECK(L <= max_len && L <= slot - 2 * K);
    const bool d = stp::deflates(op, opt, len, threshold);
    const int32_t prov = stp::provisional(op, d, len, L);
    const bool enters = d && prov == 0;
    CHECK(!enters || len <= L);
    const stp::Place pl = stp::place(c.pos, len, slot, K, enters);
    CHECK(enters || (!pl.slide && pl.new_pos == c.pos && pl.z_len == 0 && pl.hist == 0));
    if (pl.slide) {
        CHECK(pl.new_pos == K && c.pos >= 2 * K && c.pos <= slot);
        memcpy(c.buf, c.buf + c.pos - K, K);   // [pos - K, pos) -> [0, K)
        ++slides;
    }
    if (enters) {
        CHECK(pl.z_len == len && pl.hist == (pl.new_pos < K ? pl.new_pos : K));
        CHECK((uint64_t)pl.new_pos + len <= slot);
        memcpy(c.buf + pl.new_pos, msg.data(), len);
        // the history is the tail of what the peer has seen
        const uint8_t* h = c.buf + pl.new_pos - pl.hist;
        const size_t have = c.stream.size() < pl.hist ? c.stream.size() : pl.hist;
        CHECK(have == pl.hist || c.stream.size() == pl.new_pos);
        CHECK(memcmp(h + pl.hist - have, c.stream.data() + c.stream.size() - have, have) == 0);
        uint32_t sum = 0;
        for (uint32_t i = 0; i < pl.hist + len; ++i) sum += h[i];   // the deflater's reads
        CHECK(sum != 0xffffffffu);
        chunks += (len + stp::CHUNK - 1) / stp::CHUNK;
    }
    int32_t st = stp::merge(prov, enters, zst);
    CHECK(st == (prov ? prov : enters ? zst : 0));
    if (st == 0 && op != stp::OP_IDLE && !wire_ok) st = sp::E_BUFFER_OVERFLOW;
    const uint32_t p1 = stp::advance(pl.new_pos, len, enters, st);
    CHECK(p1 == (enters && st == 0 ? pl.new_pos + len : pl.new_pos) && p1 <= slot);
    CHECK(enters || p1 == c.pos);
    if (enters && st == 0) c.stream += msg;
    c.pos = p1;
}

int main()
{
    int calls = 0, slides = 0;
    for (uint32_t extra : {1u, 2u, 100u, 4096u, 9000u}) {
        const uint32_t slot = 2 * stp::K + extra;
        Conn conns[6];
        for (Conn& c : conns) c.buf = (uint8_t*)malloc(slot);
        for (int round = 0; round < 400; ++round) {
            const uint32_t maxes[] = {1, extra - 1 ? extra - 1 : 1, extra, extra + 1, slot, 0xffffffffu};
            const uint32_t max_len = maxes[rnd(6)];
            const uint32_t L = stp::room(max_len, slot, stp::K);
            uint64_t chunks = 0;
            for (Conn& c : conns) {
                const uint32_t lens[] = {0, 1, L ? L - 1 : 0, L, L + 1, rnd(extra + 3)};
                const uint32_t len = lens[rnd(6)];
                std::string msg(len, '\0');
                for (char& ch : msg) ch = (char)('a' + rnd(26));
                const uint32_t op = rnd(8) ? 1 + rnd(2) : rnd(2) ? 0u : 3u;
                const uint64_t thr[] = {0, 1, len, (uint64_t)len + 1};
                const uint32_t pos0 = c.pos;
                const size_t seen = c.stream.size();
                one_call(c, slot, max_len, op, rnd(4) != 0, thr[rnd(4)], msg, rnd(12) ? 0 : sp::E_NEED_BUFFERS,
                         rnd(12) != 0, slides, chunks);
                CHECK(c.pos >= pos0 || c.pos >= stp::K);
                CHECK(c.stream.size() >= seen);
                ++calls;
            }
            CHECK(chunks <= stp::chunk_bound(6, L));
        }
        for (Conn& c : conns) free(c.buf);
    }
    CHECK(slides > 100);
    printf("%d calls, %d slides, %d failures\n", calls, slides, failures);
    return failures ? 1 : 0;
}
