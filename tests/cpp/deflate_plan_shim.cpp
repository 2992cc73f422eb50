// C entry points over beast_amd/csrc/deflate_plan.h for
// tests/test_deflate_plan.py (plain g++, no HIP): the header's tables, and the
// host stitch of deflate_plan_stitch.h over every capacity of a sweep.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "deflate_plan_stitch.h"

using namespace bpmd;

extern "C" uint32_t dp_chunk(void) { return dfl::CHUNK; }
extern "C" uint32_t dp_slot(void) { return dfl::SLOT; }
extern "C" uint32_t dp_chunk_count(uint32_t len, int all) { return dfl::chunk_count(len, all != 0); }
extern "C" uint64_t dp_chunk_bound(uint32_t n, uint32_t L) { return dfl::chunk_bound(n, L); }
extern "C" uint32_t dp_word(int overflow, int stored, uint32_t nbits)
{
    return dfl::chunk_word(overflow != 0, stored != 0, nbits);
}
// o: overflow, stored, bits
extern "C" void dp_read_word(uint32_t w, uint32_t* o)
{
    o[0] = w == dfl::W_OVERFLOW, o[1] = (w & dfl::W_STORED) != 0, o[2] = w & ~dfl::W_STORED;
}
extern "C" int dp_marker_before(uint32_t c, int stored) { return dfl::marker_before(c, stored != 0); }
// o: first, items, bits, slots, scan, bytes
extern "C" void dp_layout(uint32_t n, uint32_t total, uint64_t scan_bytes, uint64_t* o)
{
    const dfl::Layout l(n, total, (size_t)scan_bytes);
    o[0] = l.first, o[1] = l.items, o[2] = l.bits, o[3] = l.slots, o[4] = l.scan, o[5] = l.bytes;
}
extern "C" int dp_size_t_bytes(void) { return (int)sizeof(size_t); }
// kind: 0 read back, 1 exact, 2 bound
extern "C" int dp_one_launch_setup(int kind, uint64_t chunks, uint32_t n)
{
    const dfl::ChunkSource::Kind kinds[3] = {dfl::ChunkSource::READ_BACK, dfl::ChunkSource::EXACT,
                                             dfl::ChunkSource::BOUND};
    dfl::ChunkSource s;
    s.kind = kinds[kind], s.chunks = chunks;
    return dfl::one_launch_setup(s, n);
}
extern "C" int dp_default_kind_is_read_back(void) { return dfl::ChunkSource().kind == dfl::ChunkSource::READ_BACK; }

// One stitch into out[0, cap); out has room bytes (>= cap), all 0xA5 before
// the call.  res: status, out_len, out_bits, bytes at or past cap that changed.
extern "C" void dp_stitch(const uint8_t* slots, uint64_t stride, const uint32_t* words, uint32_t nk, uint32_t key,
                          uint32_t cap, uint8_t* out, uint32_t room, uint32_t* res)
{
    memset(out, 0xA5, room);
    const dp_test::Stitched r = dp_test::stitch(slots, (size_t)stride, words, nk, out, cap, key);
    uint32_t touched = 0;
    for (uint32_t p = cap; p < room; ++p) touched += out[p] != 0xA5;
    res[0] = (uint32_t)r.status, res[1] = r.out_len, res[2] = r.out_bits, res[3] = touched;
}

// Every cap in [0, max_cap].  res[4 * cap ..]: status, out_len, out_bits, and
// flags: 1 = a byte at or past cap changed, 2 = out[0, out_len) is not
// full[0, out_len) (full: the payload at an ample capacity).
extern "C" void dp_sweep(const uint8_t* slots, uint64_t stride, const uint32_t* words, uint32_t nk, uint32_t key,
                         uint32_t max_cap, const uint8_t* full, uint32_t* res)
{
    std::vector<uint8_t> out(max_cap + 16);
    for (uint32_t cap = 0; cap <= max_cap; ++cap) {
        uint32_t r[4];
        dp_stitch(slots, stride, words, nk, key, cap, out.data(), (uint32_t)out.size(), r);
        res[4 * cap] = r[0], res[4 * cap + 1] = r[1], res[4 * cap + 2] = r[2];
        res[4 * cap + 3] = (r[3] ? 1u : 0u) | (r[1] && memcmp(out.data(), full, r[1]) ? 2u : 0u);
    }
}
