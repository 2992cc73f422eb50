// deflate_plan.h -- the rules of the chunk-parallel deflater (pmd_deflate.hip:
// deflate_chunks_kernel, stitch_kernel and their driver) as
// pure functions the kernels call.  Host-compilable without HIP:
// tests/test_deflate_plan.py stitches hand-built blocks with them at every
// capacity, tests/cpp/deflate_plan_main.cpp under the address sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "send_plan.h"   // BPMD_SP_HD

namespace bpmd {
namespace dfl {

constexpr uint32_t CHUNK = 4096;   // input bytes per chunk
constexpr uint32_t SLOT = 4736;    // scratch bytes per chunk's block
static_assert(SLOT >= CHUNK + CHUNK / 8 + CHUNK / 64 + 11 + 2 && SLOT % 16 == 0,
              "bpmd_deflate_upper_bound(CHUNK) + 2 fits a slot, a 16-byte multiple");

// chunks of the chunk-parallel path: every chunk of a message with a history
// window (all), else only messages over one chunk
BPMD_SP_HD uint32_t chunk_count(uint32_t len, bool all) { return (all || len > CHUNK) ? (len + CHUNK - 1) / CHUNK : 0u; }
// the most chunks n messages of at most L bytes make
BPMD_SP_HD uint64_t chunk_bound(uint32_t n, uint32_t L) { return (uint64_t)n * (((uint64_t)L + CHUNK - 1) / CHUNK); }

// a chunk's word in bits[]: its block's bits in the slot (from bit 0), bit 31
// set for a stored block; all ones when the slot overflowed
constexpr uint32_t W_OVERFLOW = 0xFFFFFFFFu, W_STORED = 0x80000000u;
BPMD_SP_HD uint32_t chunk_word(bool overflow, bool stored, uint32_t nbits)
{
    return overflow ? W_OVERFLOW : ((stored ? W_STORED : 0u) | nbits);
}

// ---- the stitch.  bit: the message's output bits so far; the byte at
// bit >> 3 is partial and not written yet.  A step fits when room <= cap:
// each asks for one byte beyond its own last byte, the tail's.
// a marker (an empty stored block) precedes every Huffman-coded chunk but the
// first, and a stored chunk 1
BPMD_SP_HD bool marker_before(uint32_t c, bool stored) { return c >= 1 && (!stored || c == 1); }

// A stored block at `bit`: 000 and the pad complete the partial byte `at`
// (and take a byte of zeros more when pay - at == 2); nbytes bytes follow
// from `pay`: LEN, NLEN and the data.  The marker: 4 bytes, 00 00 FF FF.  A
// stored chunk, word w: (w & ~W_STORED) / 8 - 1 bytes, from its slot's byte 1.
struct StoredSpan {
    uint32_t at, pay, nbytes, room, next;   // next: the bit position after it
};
BPMD_SP_HD StoredSpan stored_span(uint32_t bit, uint32_t nbytes)
{
    const uint32_t pay = (bit + 3 + 7) >> 3;
    return {bit >> 3, pay, nbytes, pay + nbytes + 1, (pay + nbytes) * 8};
}

// A Huffman-coded block of nbits bits at `bit`: its slot_bytes bytes, shifted
// left by `shift` bits and merged with the partial byte, complete `full`
// output bytes from `at`; its last bits stay in the next partial byte.
struct HuffSpan {
    uint32_t at, shift, full, slot_bytes, room, next;
};
BPMD_SP_HD HuffSpan huff_span(uint32_t bit, uint32_t nbits)
{
    const uint32_t next = bit + nbits;
    return {bit >> 3, bit & 7, (next >> 3) - (bit >> 3), (nbits + 7) >> 3, ((next + 7) >> 3) + 1, next};
}

// The tail behind `at` whole bytes and a partial byte of nbits bits:
// Flush::sync's 000 and the pad, 00 00 FF FF stripped -- two bytes when the
// three bits do not fit the partial byte.  out_len is also the tail's room.
BPMD_SP_HD uint32_t tail_bytes(uint32_t nbits) { return nbits + 3 > 8 ? 2u : 1u; }
BPMD_SP_HD uint32_t tail_out_len(uint32_t at, uint32_t nbits) { return at + tail_bytes(nbits); }

// ---- the workspace: first[n + 1] | items[total] | bits[total] |
// slots[total] | the scan's temporary storage, each 256-aligned
struct Layout {
    size_t first = 0, items, bits, slots, scan, bytes;
    static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
    Layout(uint32_t n, uint32_t total, size_t scan_bytes)
    {
        items = al256(4 * ((size_t)n + 1));
        bits = al256(items + 4 * (size_t)total);
        slots = al256(bits + 4 * (size_t)total);
        scan = al256(slots + (size_t)SLOT * total);
        bytes = al256(scan + scan_bytes);
    }
};

// ---- where the host gets the chunk count from.  The value sizes the workspace
// and the chunk kernel's grid; the kernels take the count from the device, so
// any value at least the count serves -- except for the one-launch setup (one
// message, exact count: no memset, count, scan and fill), which writes it.
struct ChunkSource {
    enum Kind : uint32_t { READ_BACK, EXACT, BOUND } kind = READ_BACK;   // EXACT, BOUND: nothing is read back
    uint64_t chunks = 0;   // EXACT: the sum of chunk_count; BOUND: at least that; over 2^32 - 1 is refused
};
BPMD_SP_HD bool one_launch_setup(const ChunkSource& s, uint32_t n) { return s.kind == ChunkSource::EXACT && n == 1; }

}  // namespace dfl
}  // namespace bpmd
