// The chunk-parallel deflater's stitch rules (beast_amd/csrc/deflate_plan.h)
// under -fsanitize=address,undefined: the host stitch of
// deflate_plan_stitch.h over a fixed subset of the sequences of
// tests/test_deflate_plan.py -- every sequence of one and two chunks over
// {stored, Huffman} x 0 to 8 data bytes, and the three-chunk sequences with
// 0, 3 or 8 bytes a chunk -- at every capacity from 0 to two bytes past the
// payload, masked and not.  The output is a heap block of exactly `cap`
// bytes and every slot a heap block of exactly its block's bytes, so one
// byte read or written outside either aborts the program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "deflate_plan_stitch.h"

using namespace bpmd;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            if (failures++ < 10) printf("line %d: %s\n", __LINE__, #c); \
        }                                                         \
    } while (0)

struct Bits {
    std::vector<uint8_t> bytes;
    uint32_t n = 0;
    void put(uint32_t bit)
    {
        if ((n & 7) == 0) bytes.push_back(0);
        bytes[n >> 3] |= (uint8_t)(bit << (n & 7));
        ++n;
    }
    void code(uint32_t v, int len)   // a Huffman code: its high bit first
    {
        for (int i = len - 1; i >= 0; --i) put((v >> i) & 1);
    }
};

struct Chunk {
    bool stored;
    uint32_t len;
};

// a chunk's slot as the chunk kernel leaves it, and its word
static uint32_t make_block(const Chunk& c, uint32_t seed, std::vector<uint8_t>& slot)
{
    if (c.stored) {
        slot = {0, (uint8_t)c.len, 0, (uint8_t)~c.len, 0xff};   // 000 + pad, LEN, NLEN
        for (uint32_t i = 0; i < c.len; ++i) slot.push_back((uint8_t)(37 * seed + 11 * i + 1));
        return dfl::chunk_word(false, true, 8 * (uint32_t)slot.size());
    }
    Bits b;   // a fixed-Huffman block of the literals 65 (8 bits) and 200 (9 bits), BFINAL 0
    b.put(0), b.put(1), b.put(0);
    for (uint32_t i = 0; i < c.len; ++i) {
        if ((seed >> i) & 1) b.code(0x30 + 65, 8);
        else b.code(0x190 + 200 - 144, 9);
    }
    b.code(0, 7);
    slot = b.bytes;
    return dfl::chunk_word(false, false, b.n);
}

static int runs = 0, refused = 0;

static void one_sequence(const std::vector<Chunk>& seq, uint32_t key)
{
    const uint32_t nk = (uint32_t)seq.size();
    size_t stride = 0;
    std::vector<std::vector<uint8_t>> blocks(nk);
    std::vector<uint32_t> words(nk);
    for (uint32_t c = 0; c < nk; ++c) {
        words[c] = make_block(seq[c], 5 * c + seq[c].len, blocks[c]);
        if (blocks[c].size() > stride) stride = blocks[c].size();
    }
    // the slots in one heap block that ends with the last chunk's last byte
    const size_t total = stride * (nk - 1) + blocks[nk - 1].size();
    uint8_t* slots = (uint8_t*)malloc(total);
    memset(slots, 0xEE, total);
    for (uint32_t c = 0; c < nk; ++c) memcpy(slots + c * stride, blocks[c].data(), blocks[c].size());

    // an ample capacity first: the payload every smaller accepted one must equal
    uint8_t* full = (uint8_t*)malloc(256);
    const dp_test::Stitched f = dp_test::stitch(slots, stride, words.data(), nk, full, 256, key);
    CHECK(f.status == dp_test::OK && f.out_len >= 1 && f.out_len == (f.out_bits >> 3) + ((f.out_bits & 7) > 5 ? 2u : 1u));
    // the smallest accepted capacity: the payload, plus a byte when the last
    // block is Huffman-coded and ends 1 to 5 bits into a byte
    const uint32_t ends = seq[nk - 1].stored ? 0u : (f.out_bits & 7);
    const uint32_t need = f.out_len + (ends >= 1 && ends <= 5 ? 1u : 0u);
    for (uint32_t cap = 0; cap <= f.out_len + 2; ++cap) {
        uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
        const dp_test::Stitched r = dp_test::stitch(slots, stride, words.data(), nk, cap ? out : nullptr, cap, key);
        if (cap >= need) {
            CHECK(r.status == dp_test::OK && r.out_len == f.out_len && r.out_bits == f.out_bits);
            CHECK(r.out_len <= cap && memcmp(out, full, r.out_len) == 0);
        } else {
            CHECK(r.status == dp_test::NEED_BUFFERS && r.out_len == 0 && r.out_bits == 0);
            ++refused;
        }
        free(out);
        ++runs;
    }
    // an overflowed chunk in any position refuses the message
    for (uint32_t at = 0; at < nk; ++at) {
        std::vector<uint32_t> w2 = words;
        w2[at] = dfl::chunk_word(true, false, 0);
        const dp_test::Stitched r = dp_test::stitch(slots, stride, w2.data(), nk, full, 256, key);
        CHECK(r.status == dp_test::NEED_BUFFERS && r.out_len == 0);
    }
    free(full);
    free(slots);
}

int main()
{
    std::vector<Chunk> opts, few;
    for (int stored = 0; stored < 2; ++stored)
        for (uint32_t len = 0; len <= 8; ++len) {
            opts.push_back({stored != 0, len});
            if (len == 0 || len == 3 || len == 8) few.push_back({stored != 0, len});
        }
    int sequences = 0;
    for (uint32_t key : {0u, 0xA1B2C3D4u}) {
        for (const Chunk& a : opts) {
            one_sequence({a}, key), ++sequences;
            for (const Chunk& b : opts) one_sequence({a, b}, key), ++sequences;
        }
        for (const Chunk& a : few)
            for (const Chunk& b : few)
                for (const Chunk& c : few) one_sequence({a, b, c}, key), ++sequences;
    }
    CHECK(sequences == 2 * (18 + 324 + 216) && refused > 5000);
    printf("%d sequences, %d runs, %d refused, %d failures\n", sequences, runs, refused, failures);
    return failures ? 1 : 0;
}
