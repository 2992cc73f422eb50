// The receive side's plan (beast_amd/csrc/receive_plan.h) under
// -fsanitize=address,undefined: the chain select -> inflater -> merge -> byte
// check runs on the host with a stand-in inflater (a copy that stops at its
// capacity and says need_buffers, as the real one does), every gathered slot
// and message slot a heap block of exactly out_len / the effective capacity
// bytes, so one byte read or written outside what the plan announces aborts
// the program; msg_max takes the values around 2^32 and 2^64 where
// msg_max + 1 must not be formed carelessly.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>

#include "receive_plan.h"

using namespace bpmd;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            if (failures++ < 10) printf("line %d: %s\n", __LINE__, #c); \
        }                                                         \
    } while (0)

static std::mt19937_64 rng(20241020);
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }
static uint8_t* block(size_t n) { return (uint8_t*)malloc(n ? n : 1); }   // malloc(0) may be null

// total: the bytes the message inflates to; zerr: a zlib error met after `before` bytes (0 = none)
static void one_entry(uint32_t event, int32_t fst, uint32_t compressed, uint32_t op, uint32_t out_len, uint32_t msg_cap,
                      uint64_t msg_max, uint32_t total, int32_t zerr, uint32_t before)
{
    const rp::Select s = rp::select(event, fst, compressed, op, out_len, msg_cap, msg_max);
    const bool z = rp::inflates(event, fst, compressed);
    CHECK(s.in_len == (z ? out_len : 0u) && s.eff_cap <= msg_cap && (z || s.eff_cap == 0));
    CHECK(!z || msg_max == 0 || s.eff_cap <= msg_max || s.eff_cap - 1 == msg_max);
    CHECK(!z || msg_max != 0 || s.eff_cap == msg_cap);
    uint8_t* gathered = block(out_len);
    memset(gathered, 'a', out_len);
    uint8_t* slot = block(s.eff_cap);
    // the stand-in inflater: reads in_len bytes, writes at most eff_cap
    uint32_t sum = 0, z_len = 0;
    int32_t zst = 0;
    for (uint32_t i = 0; i < s.in_len; ++i) sum += gathered[i];
    if (z) {
        const uint32_t want = zerr ? (before < total ? before : total) : total;
        z_len = want < s.eff_cap ? want : s.eff_cap;
        for (uint32_t i = 0; i < z_len; ++i) slot[i] = (uint8_t)('b' + (sum & 1));
        zst = want > s.eff_cap ? rp::E_NEED_BUFFERS : zerr;
    }
    const rp::Merge m = rp::merge(event, fst, compressed, op, out_len, msg_cap, msg_max, zst, z_len);
    // the byte check reads msg_len bytes of the slot merge names
    if (m.src != rp::SRC_NONE) {
        CHECK(m.status == 0 && op == rp::OP_TEXT);
        const uint8_t* p = m.src == rp::SRC_INFLATED ? slot : gathered;
        uint32_t acc = 0;
        for (uint32_t i = 0; i < m.msg_len; ++i) acc += p[i];
        CHECK(m.msg_len == 0 || acc != 0);
        CHECK((m.src == rp::SRC_INFLATED) == (compressed != 0));
    }
    if (event != rp::EV_MESSAGE || fst != 0) {
        CHECK(m.status == fst && m.msg_len == 0 && m.src == rp::SRC_NONE);
    } else if (!compressed) {
        CHECK(m.status == 0 && m.msg_len == out_len);
    } else {
        CHECK(m.msg_len == z_len);
        const bool over_max = msg_max && total > msg_max, over_cap = total > msg_cap;
        if (zerr && before <= s.eff_cap && before < total) CHECK(m.status == zerr);   // met before any limit
        else if (!zerr && !over_max && !over_cap) CHECK(m.status == 0 && m.msg_len == total);
        else if (!zerr && over_max && msg_max <= msg_cap) CHECK(m.status == rp::E_MESSAGE_TOO_BIG);
        else if (!zerr && over_cap) CHECK(m.status == rp::E_BUFFER_OVERFLOW);
    }
    free(gathered);
    free(slot);
}

int main()
{
    const uint64_t maxes[] = {0, 1, 2, 99, 100, 101, 4095, 4096, 4097, 0xfffffffeull, 0xffffffffull, 0x100000000ull,
                              1ull << 63, ~0ull};
    const uint32_t caps[] = {0, 1, 99, 100, 101, 4096, 5000};
    int n = 0;
    for (uint64_t msg_max : maxes)
        for (uint32_t cap : caps)
            for (uint32_t event = 0; event <= 4; ++event)
                for (int32_t fst : {0, 262})
                    for (uint32_t comp = 0; comp <= 1; ++comp)
                        for (uint32_t op = 1; op <= 2; ++op)
                            for (uint32_t total : {0u, 1u, 98u, 99u, 100u, 101u, 102u, 4096u, 4097u, 6000u})
                                for (int32_t zerr : {0, 6, 13}) {
                                    one_entry(event, fst, comp, op, rnd(300), cap, msg_max, total, zerr,
                                              zerr ? rnd(total + 1) : 0u);
                                    ++n;
                                }
    // effective_cap at the 32- and 64-bit edges
    CHECK(rp::effective_cap(0xffffffffu, 0xfffffffeull) == 0xffffffffu);
    CHECK(rp::effective_cap(0xffffffffu, 0xfffffffdull) == 0xfffffffeu);
    CHECK(rp::effective_cap(0xffffffffu, 0xffffffffull) == 0xffffffffu);
    CHECK(rp::effective_cap(0xffffffffu, ~0ull) == 0xffffffffu);
    CHECK(rp::effective_cap(7u, 0) == 7u && rp::effective_cap(7u, 6) == 7u && rp::effective_cap(7u, 5) == 6u);
    printf("%d entries, %d failures\n", n, failures);
    return failures ? 1 : 0;
}
