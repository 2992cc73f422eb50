// Fuzz of the receive side's header step and frame walk (beast_amd/csrc/
// frame_parse.h), built with -fsanitize=address,undefined: every input lives
// in a heap block of exactly `avail` bytes, so one byte read at or beyond
// p + avail aborts the program.  Beside that it counts violations of what the
// callers rely on: a FRAME's header lies inside the bytes given, the walk
// consumes no more than it was given, data lands inside the out slot and a
// control payload inside its 128-byte slot.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "frame_parse.h"

using namespace bpmd::fp;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            if (failures++ < 10) printf("line %d: %s\n", __LINE__, #c); \
        }                                                         \
    } while (0)

static std::mt19937_64 rng(20240611);
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }

// a header: mostly well-formed, sometimes with a random byte
static std::vector<uint8_t> make_header(bool masked, uint64_t& len)
{
    static const uint8_t first[] = {0x00, 0x01, 0x02, 0x80, 0x81, 0x82, 0xC1, 0x41, 0x88, 0x89, 0x8A, 0x83, 0x09, 0xB1};
    static const uint64_t lens[] = {0, 1, 2, 3, 16, 17, 125, 126, 127, 300, 65535, 65536, 70001, (1ull << 63) - 1,
                                    1ull << 63};
    std::vector<uint8_t> h;
    h.push_back(rnd(4) ? first[rnd(sizeof first)] : (uint8_t)rnd(256));
    len = lens[rnd(sizeof lens / sizeof lens[0])];
    const uint32_t form = rnd(8) ? (len <= 125 ? 7 : len <= 65535 ? 16 : 64) : (rnd(2) ? 16 : 64);
    const uint8_t m = masked ? 0x80 : 0;
    if (form == 7) h.push_back(m | (uint8_t)len);
    else if (form == 16) {
        h.push_back(m | 126);
        len &= 0xffff;
        h.push_back((uint8_t)(len >> 8)), h.push_back((uint8_t)len);
    } else {
        h.push_back(m | 127);
        for (int i = 7; i >= 0; --i) h.push_back((uint8_t)(len >> (8 * i)));
    }
    if (masked)
        for (int i = 0; i < 4; ++i) h.push_back((uint8_t)rnd(256));
    if (!rnd(6)) h[rnd((uint32_t)h.size())] = (uint8_t)rnd(256);
    return h;
}

static void fuzz_parse(int rounds)
{
    for (int it = 0; it < rounds; ++it) {
        uint64_t len;
        const bool masked = rnd(2);
        std::vector<uint8_t> h = make_header(masked, len);
        h.push_back((uint8_t)rnd(256)), h.push_back((uint8_t)rnd(256));
        RdState st;
        reset(st);
        if (rnd(2)) st.rd_cont = 1, st.rd_op = 1 + rnd(2), st.rd_deflated = rnd(2), st.rd_size = rnd(2) ? rnd(5000) : ~0ull - rnd(200);
        const uint32_t role = rnd(4) ? (masked ? ROLE_SERVER : ROLE_CLIENT) : rnd(2);
        const uint64_t msg_max = rnd(3) ? 0 : rnd(100000), room = rnd(3) ? 0xffffffffu : rnd(70000);
        for (size_t avail = 0; avail <= h.size(); ++avail) {
            uint8_t* p = (uint8_t*)malloc(avail ? avail : 1);   // exactly avail bytes (malloc(0) may be null)
            if (avail) memcpy(p, h.data(), avail);
            Header fh;
            const int32_t r = parse_fh(p, avail, role, rnd(2), msg_max, room, st, fh);
            if (r == FRAME) {
                CHECK(fh.hdr_len <= avail && fh.hdr_len >= 2 && fh.hdr_len <= 14);
                CHECK(is_control(fh.op) ? fh.len <= 125 : fh.len <= room);
                CHECK(!(fh.len >> 63));
            } else
                CHECK(r == NEED_MORE || (r >= E_BUFFER_OVERFLOW && r <= E_BAD_SIZE));
            free(p);
        }
    }
}

// streams of frames with real payloads, cut anywhere, walked to the end
static void fuzz_walk(int rounds)
{
    for (int it = 0; it < rounds; ++it) {
        const bool masked = rnd(2);
        std::vector<uint8_t> w;
        for (uint32_t f = 0, nf = 1 + rnd(6); f < nf; ++f) {
            uint64_t len;
            std::vector<uint8_t> h = make_header(masked, len);
            w.insert(w.end(), h.begin(), h.end());
            if (len <= 70001) w.insert(w.end(), (size_t)len, (uint8_t)rnd(256));
        }
        const uint32_t wl = rnd(3) ? (uint32_t)w.size() : rnd((uint32_t)w.size() + 1);
        const uint32_t cap = rnd(4) ? 200000 : rnd(300);
        uint8_t* p = (uint8_t*)malloc(wl ? wl : 1);
        if (wl) memcpy(p, w.data(), wl);
        uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
        uint8_t* ctl = (uint8_t*)malloc(128);
        RdState st;
        reset(st);
        uint32_t pos = 0;
        for (int call = 0; call < 16; ++call) {
            Stop s;
            walk(
                p + pos, wl - pos, masked ? ROLE_SERVER : ROLE_CLIENT, true, 0, cap, st,
                [&](uint64_t at, const uint8_t* src, uint32_t len, uint32_t key) {
                    CHECK(at + len <= cap);
                    if (at + len <= cap)
                        for (uint32_t i = 0; i < len; ++i) out[at + i] = src[i] ^ (uint8_t)(key >> (8 * (i & 3)));
                },
                [&](const uint8_t* src, uint32_t len, uint32_t key) {
                    CHECK(len <= 125);
                    if (len <= 125)
                        for (uint32_t i = 0; i < len; ++i) ctl[i] = src[i] ^ (uint8_t)(key >> (8 * (i & 3)));
                },
                s);
            CHECK(s.consumed <= wl - pos);
            CHECK(s.msg_len <= cap || s.event != EV_MESSAGE);
            pos += s.consumed;
            if (s.event == EV_NEED_MORE) break;   // the end of the bytes, or a refused header
            CHECK(s.consumed > 0);
        }
        free(p), free(out), free(ctl);
    }
}

int main()
{
    for (uint32_t v = 0; v < 65536; ++v) {
        const bool want = v >= 1000 && !(v >= 1004 && v <= 1006) && !(v >= 1015 && v <= 2999);
        CHECK(close_code_valid((uint16_t)v) == want);
    }
    fuzz_parse(20000);
    fuzz_walk(3000);
    printf("%d failures\n", failures);
    return failures != 0;
}
