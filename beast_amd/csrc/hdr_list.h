// hdr_list.h -- the compact list of coded runs a dynamic block header's
// code-length pass (pass 1) leaves for symbol placement (pass 2) in the lane
// kernel (pmd_inflate_lane3.hip).  Host-compilable: tests/cpp/hdr_list_main.cpp
// checks the fit rule and the entry format on the CPU.
//
// Pass 1 decodes runs [first, first + rep) of one code length.  Most of a
// header's ~294 symbols have length 0 and place nothing, so every run with a
// non-zero length also becomes one 16-bit entry
//
//   bits 0-8  first symbol (0 .. 315)
//   bits 9-12 code length  (1 .. 15)
//   bits 13-15 rep - 1     (a literal length is 1 long, a `16` repeat 3 .. 6)
//
// and pass 2 walks the entries instead of every symbol.  The list needs no
// LDS of its own: it grows downward from the top of the literal/length symbol
// area (AREA bytes, written by pass 2 only), entry j at byte AREA - 2 (j + 1).
// Placement fills bytes [0, coded_litlen) of the same area from the bottom,
// so list and placed symbols stay apart exactly when
// 2 entries + coded_litlen <= AREA; a header that does not fit keeps the walk
// over the nibble array.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BPMD_HL_FN __host__ __device__ inline
#else
#define BPMD_HL_FN inline
#endif

namespace bpmd {
namespace hl {

constexpr uint32_t AREA = 288;             // bytes of the literal/length symbol area
constexpr uint32_t MAX_ENTRIES = AREA / 2;   // entries the area can hold at all

// byte offset of entry j within the area (j < MAX_ENTRIES)
BPMD_HL_FN uint32_t entry_off(uint32_t j) { return AREA - 2u * (j + 1u); }

BPMD_HL_FN uint32_t entry_pack(uint32_t first, uint32_t len, uint32_t rep)
{
    return first | (len << 9) | ((rep - 1u) << 13);
}
BPMD_HL_FN uint32_t entry_first(uint32_t e) { return e & 0x1ffu; }
BPMD_HL_FN uint32_t entry_len(uint32_t e) { return (e >> 9) & 15u; }
BPMD_HL_FN uint32_t entry_rep(uint32_t e) { return ((e >> 13) & 7u) + 1u; }

// entries: non-zero runs pass 1 saw (counted past MAX_ENTRIES too, though
// only the first MAX_ENTRIES are stored); coded_litlen: literal/length
// symbols with a non-zero length
BPMD_HL_FN bool list_fits(uint32_t entries, uint32_t coded_litlen) { return 2u * entries + coded_litlen <= AREA; }

}  // namespace hl
}  // namespace bpmd
