// The send side's plan (beast_amd/csrc/send_plan.h) under
// -fsanitize=address,undefined: every payload, key array, wire buffer and
// control slot is a heap block of exactly the size the plan announces, so one
// byte read or written outside it aborts the program.  Each message is written
// frame by frame with the closed-form offsets, in a shuffled frame order, and
// read back by the receive side's walk (frame_parse.h), which must return the
// payload, consume exactly wire_size bytes and see the opcode and RSV1; the
// two host bounds must cover what was written.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "frame_parse.h"
#include "send_plan.h"

using namespace bpmd;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            if (failures++ < 10) printf("line %d: %s\n", __LINE__, #c); \
        }                                                         \
    } while (0)

static std::mt19937_64 rng(20240917);
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }

static uint8_t* block(size_t n) { return (uint8_t*)malloc(n ? n : 1); }   // malloc(0) may be null

static void one_message(uint32_t len, uint32_t fm, bool masked, bool comp, bool frag, uint32_t in_len)
{
    const sp::Split s = sp::split(len, fm, comp, frag);
    const uint64_t size = sp::wire_size(s, masked);
    uint8_t* payload = block(len);
    for (uint32_t i = 0; i < len; ++i) payload[i] = (uint8_t)rnd(256);
    uint32_t* keys = (uint32_t*)block(masked ? s.frames * 4 : 0);
    for (uint64_t f = 0; masked && f < s.frames; ++f) keys[f] = (uint32_t)rng();
    uint8_t* wire = block(size);
    const uint32_t op = 1 + rnd(2);
    std::vector<uint64_t> order(s.frames);
    for (uint64_t f = 0; f < s.frames; ++f) order[f] = f;
    std::shuffle(order.begin(), order.end(), rng);
    uint64_t written = 0;
    for (uint64_t f : order) {
        const uint64_t fl = sp::frame_len(s, f), at = sp::frame_off(s, masked, f);
        const uint32_t key = masked ? keys[f] : 0u;
        uint64_t h0, h1;
        const uint32_t hl = sp::header(fl, f == 0, f + 1 == s.frames, comp, op, masked, key, h0, h1);
        CHECK(hl == sp::hdr_len(fl, masked) && at + hl + fl <= size);
        for (uint32_t i = 0; i < hl; ++i) wire[at + i] = sp::header_byte(h0, h1, i);
        const uint8_t* src = payload + sp::frame_src(s, f);
        for (uint64_t t = 0; t < fl; ++t) wire[at + hl + t] = src[t] ^ (uint8_t)(key >> (8 * (t & 3)));
        written += hl + fl;
    }
    CHECK(written == size);
    // the receiving end: a server reads a client's masked frames
    uint8_t* out = block(len);
    fp::RdState st;
    fp::reset(st);
    fp::Stop stop;
    fp::walk(
        wire, (uint32_t)size, masked ? fp::ROLE_SERVER : fp::ROLE_CLIENT, true, 0, len, st,
        [&](uint64_t at, const uint8_t* src, uint32_t n, uint32_t key) {
            CHECK(at + n <= len);
            if (at + n <= len)
                for (uint32_t i = 0; i < n; ++i) out[at + i] = src[i] ^ (uint8_t)(key >> (8 * (i & 3)));
        },
        [&](const uint8_t*, uint32_t, uint32_t) { CHECK(false); }, stop);
    CHECK(stop.event == fp::EV_MESSAGE && stop.status == 0 && stop.consumed == size && stop.msg_len == len);
    CHECK(stop.msg_op == op && stop.msg_deflated == (comp ? 1u : 0u));
    CHECK(memcmp(out, payload, len) == 0);
    // in_len: an input length this payload can come from
    CHECK(sp::frame_bound(in_len, fm, comp, frag) >= s.frames);
    CHECK(sp::wire_bound(in_len, fm, masked, comp, frag) >= size);
    free(payload), free(keys), free(wire), free(out);
}

static void messages(int rounds)
{
    static const uint32_t fms[] = {1, 2, 125, 126, 127, 4096, 65535, 65536, 70000};
    for (int it = 0; it < rounds; ++it) {
        const uint32_t fm = fms[rnd(sizeof fms / sizeof fms[0])];
        uint32_t in_len;
        switch (rnd(4)) {
        case 0: in_len = rnd(131); break;
        case 1: in_len = 65530 + rnd(11); break;
        case 2: in_len = fm * (1 + rnd(3)) - 1 + rnd(3); break;
        default: in_len = rnd(80000); break;
        }
        if (fm <= 2 && in_len > 3000) in_len %= 3000;
        const bool comp = rnd(2), frag = rnd(2), masked = rnd(2);
        // a compressed message's payload is any length up to the deflater's bound
        const uint32_t len = comp ? rnd((uint32_t)sp::deflate_bound(in_len) + 1) : in_len;
        one_message(len, fm, masked, comp, frag, in_len);
    }
}

static void controls(int rounds)
{
    for (int it = 0; it < rounds; ++it) {
        static const uint32_t ops[] = {8, 9, 10, 8, 9, 10, 0, 1, 2, 11};
        const uint32_t op = ops[rnd(sizeof ops / sizeof ops[0])];
        const uint32_t sl = rnd(8) ? rnd(126) : 124 + rnd(5);
        static const uint32_t codes[] = {0, 1000, 1001, 3000, 4999};
        const uint32_t code = codes[rnd(5)];
        const bool masked = rnd(2);
        const uint32_t key = (uint32_t)rng();
        uint8_t* slot = block(sl);
        for (uint32_t i = 0; i < sl; ++i) slot[i] = (uint8_t)('a' + rnd(26));
        uint32_t pl;
        const int32_t st = sp::control_plan(op, sl, code, pl);
        if (st) {
            CHECK(st == (op >= 8 && op <= 10 ? sp::E_BAD_CONTROL_SIZE : sp::E_BAD_OPCODE));
            free(slot);
            continue;
        }
        const uint32_t size = sp::control_size(pl, masked);
        CHECK(size <= sp::CTL_WIRE && pl <= sp::CTL_MAX);
        uint8_t* wire = block(size);
        for (uint32_t t = 0; t < size; ++t) wire[t] = sp::control_byte(t, op, pl, code, slot, masked, key);
        uint8_t ctl[128];
        fp::RdState rs;
        fp::reset(rs);
        fp::Stop stop;
        fp::walk(
            wire, size, masked ? fp::ROLE_SERVER : fp::ROLE_CLIENT, true, 0, 0, rs,
            [&](uint64_t, const uint8_t*, uint32_t, uint32_t) { CHECK(false); },
            [&](const uint8_t* src, uint32_t n, uint32_t k) {
                CHECK(n == pl);
                for (uint32_t i = 0; i < n && i < 128; ++i) ctl[i] = src[i] ^ (uint8_t)(k >> (8 * (i & 3)));
            },
            stop);
        CHECK(stop.consumed == size && stop.status == 0 && stop.ctl_len == pl);
        CHECK(stop.event == (op == 8 ? fp::EV_CLOSE : op == 9 ? fp::EV_PING : fp::EV_PONG));
        if (op == 8) {
            CHECK(stop.close_code == (uint16_t)code);
            if (code) CHECK(memcmp(ctl + 2, slot, sl) == 0);
        } else
            CHECK(memcmp(ctl, slot, sl) == 0);
        free(slot), free(wire);
    }
}

int main()
{
    messages(6000);
    controls(20000);
    printf("%d failures\n", failures);
    return failures != 0;
}
