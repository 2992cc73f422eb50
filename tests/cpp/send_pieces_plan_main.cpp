// The piece rules of the chained send (beast_amd/csrc/send_pieces_plan.h)
// under -fsanitize=address,undefined: begin, place, slide, copy, marker,
// commit run on the host for many random rounds with a stand-in deflater (it
// reads its whole history and its whole piece, leaves a payload of a random
// length in the staging slot and reports need_buffers now and then).  Every
// connection's buffer is a heap block of exactly `slot` bytes and every
// staging slot one of exactly its capacity, so one byte read or written
// outside either aborts the program.  A second record of each connection --
// its history as one growing string, the open message's opcode and decision
// -- says what the state and the buffer must hold.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>

#include "send_pieces_plan.h"

using namespace bpmd;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            if (failures++ < 10) printf("line %d: %s\n", __LINE__, #c); \
        }                                                         \
    } while (0)

static std::mt19937_64 rng(20250311);
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }

struct Conn {
    uint8_t* buf;   // exactly slot bytes
    uint32_t pos = 0;
    spp::WrState st = {0, 0, 0, 0};
    bool no_takeover = false;
    std::string stream;   // the plaintext the peer's inflater has seen since its last reset
    bool open = false;    // this record's own: a message is open, its decision and opcode
    bool open_c = false;
    uint32_t open_op = 0;
};

static int slides, markers, resets, refused;

static void one_call(Conn& c, uint32_t slot, uint32_t max_len, uint32_t op, bool opt, bool fin, uint64_t threshold,
                     const std::string& piece, int32_t zst, bool wire_ok)
{
    const uint32_t K = spp::K, len = (uint32_t)piece.size();
    const uint32_t L = spp::room(max_len, slot, K);
    const spp::Begin b = spp::begin(c.st, op, opt, len, threshold);
    const bool data = op == 1 || op == 2;
    if (data && c.open) CHECK(b.compress == (c.open_c ? 1u : 0u) && b.op == c.open_op);
    if (data && !c.open) CHECK(b.compress == (opt && len >= threshold ? 1u : 0u) && b.op == op);
    if (!data) CHECK(b.compress == 0);
    const int32_t prov = spp::provisional(op, b.compress != 0, len, L);
    const bool enters = b.compress && prov == 0;
    const stp::Place pl = spp::place(c.pos, len, slot, K, enters);
    if (pl.slide) {
        CHECK(pl.new_pos == K && c.pos >= 2 * K && c.pos <= slot);
        memcpy(c.buf, c.buf + c.pos - K, K);
        ++slides;
    }
    // the staging slot: exactly its capacity on the heap
    const uint32_t z_len = rnd(40), z_cap = z_len + rnd(7);
    uint8_t* z = (uint8_t*)malloc(z_cap ? z_cap : 1);
    if (enters) {
        CHECK((uint64_t)pl.new_pos + len <= slot);
        memcpy(c.buf + pl.new_pos, piece.data(), len);
        const uint8_t* h = c.buf + pl.new_pos - pl.hist;
        const size_t have = c.stream.size() < pl.hist ? c.stream.size() : pl.hist;
        CHECK(have == pl.hist || c.stream.size() == pl.new_pos);
        CHECK(memcmp(h + pl.hist - have, c.stream.data() + c.stream.size() - have, have) == 0);
        uint32_t sum = 0;
        for (uint32_t i = 0; i < pl.hist + len; ++i) sum += h[i];   // the deflater's reads
        CHECK(sum != 0xffffffffu);
        if (zst == 0) memset(z, 0x5a, z_len);
    }
    int32_t st = spp::status(prov, enters, zst, fin, z_len, z_cap);
    uint64_t pay = 0;
    if (st == 0) {
        pay = spp::payload_len(b.compress != 0, fin, len, z_len);
        if (enters && !fin) {   // the size kernel's stores
            CHECK(z_len + 4 <= z_cap && pay == z_len + 4);
            z[z_len] = 0, z[z_len + 1] = 0, z[z_len + 2] = 0xff, z[z_len + 3] = 0xff;
            ++markers;
        }
    } else if (enters && zst == 0 && prov == 0) {
        CHECK(!fin && z_len + 4 > z_cap && st == sp::E_NEED_BUFFERS);
    }
    free(z);
    if (st == 0 && op != stp::OP_IDLE && !wire_ok) st = sp::E_BUFFER_OVERFLOW;
    if (st == 0 && data) {   // the piece's frames: opcode once per message, FIN once per message
        const sp::Split s = sp::split(pay, 125, b.compress != 0, true);
        for (uint64_t f = 0; f < s.frames; ++f) {
            uint64_t h0, h1;
            sp::header(sp::frame_len(s, f), spp::frame_first(f, c.st.wr_cont != 0), spp::frame_fin(f, s.frames, fin),
                       b.compress != 0, b.op, false, 0, h0, h1);
            const uint8_t b0 = sp::header_byte(h0, h1, 0);
            CHECK((b0 & 15u) == (f == 0 && !c.open ? b.op : 0u));
            CHECK(((b0 & 0x40u) != 0) == (f == 0 && !c.open && b.compress));
            CHECK(((b0 & 0x80u) != 0) == (f + 1 == s.frames && fin));
        }
    }
    const spp::Commit cm = spp::commit(c.st, pl.new_pos, len, enters, b, op == stp::OP_IDLE, st, fin, c.no_takeover);
    if (st != 0 || op == stp::OP_IDLE) {
        CHECK(cm.pos == pl.new_pos && memcmp(&cm.state, &c.st, 4) == 0);
        refused += st != 0;
    } else {
        if (enters) c.stream += piece;
        c.open = !fin, c.open_c = b.compress != 0, c.open_op = b.op;
        CHECK(cm.state.wr_cont == (fin ? 0 : 1) && cm.state.wr_compress == b.compress && cm.state.wr_op == b.op &&
              cm.state.reserved == 0);
        if (fin && b.compress && c.no_takeover) {
            CHECK(cm.pos == 0);
            c.stream.clear();
            ++resets;
        } else {
            CHECK(cm.pos == (enters ? pl.new_pos + len : pl.new_pos));
        }
    }
    CHECK(cm.pos <= slot);
    c.pos = cm.pos, c.st = cm.state;
}

int main()
{
    int calls = 0;
    for (uint32_t extra : {1u, 2u, 100u, 4097u, 9000u}) {
        const uint32_t slot = 2 * spp::K + extra;
        Conn conns[6];
        for (int i = 0; i < 6; ++i) conns[i].buf = (uint8_t*)malloc(slot), conns[i].no_takeover = i % 3 == 2;
        for (int round = 0; round < 600; ++round) {
            const uint32_t maxes[] = {1, extra - 1 ? extra - 1 : 1, extra, extra + 1, slot, 0xffffffffu};
            const uint32_t max_len = maxes[rnd(6)];
            const uint32_t L = spp::room(max_len, slot, spp::K);
            for (Conn& c : conns) {
                const uint32_t lens[] = {0, 1, L ? L - 1 : 0, L, L + 1, rnd(extra + 3)};
                const uint32_t len = lens[rnd(6)];
                std::string piece(len, '\0');
                for (char& ch : piece) ch = (char)('a' + rnd(26));
                const uint32_t op = rnd(8) ? 1 + rnd(2) : rnd(2) ? 0u : 3u;
                const uint64_t thr[] = {0, 1, len, (uint64_t)len + 1};
                one_call(c, slot, max_len, op, rnd(4) != 0, rnd(3) == 0, thr[rnd(4)], piece,
                         rnd(12) ? 0 : sp::E_NEED_BUFFERS, rnd(12) != 0);
                ++calls;
            }
        }
        for (Conn& c : conns) free(c.buf);
    }
    CHECK(slides > 100 && markers > 500 && resets > 50 && refused > 500);
    printf("%d calls, %d slides, %d markers, %d resets, %d refused, %d failures\n", calls, slides, markers, resets,
           refused, failures);
    return failures ? 1 : 0;
}
