// zstream_shim.h -- TEST INFRASTRUCTURE.  One-lane meanings of the HIP
// keywords and intrinsics that beast_amd/csrc/pmd_zstream.hip uses, so that
// with BPMD_ZSTREAM_HOST its text compiles as plain C++ (lane 0, WAVE = 1,
// readfirstlane = identity); the wave-cooperative table builder is replaced
// by the serial builder it is slot-for-slot equal to (huff_table.h; the
// equality is tests/test_gpu_tables.py).  Included by
// inflate_reader_backend.cpp ahead of the kernel source.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <stdlib.h>
#include <stdio.h>
#define __device__
#define __host__
#define __forceinline__ inline
#define __constant__
#define __global__
#define __builtin_amdgcn_readfirstlane(v) (v)
// (packed: load_window's 16-byte loads from the window are unaligned, which a plain struct may not be)
struct __attribute__((packed)) uint4 { uint32_t x, y, z, w; };
#include "../../beast_amd/csrc/huff_table.h"
#include "../../beast_amd/csrc/status.h"
namespace bpmd {
constexpr int WAVE = 1;
inline unsigned lane_id() { return 0; }
inline void wave_sync() {}
static const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31,
                                      35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3,
                                      4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193,
                                       257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                       8193, 12289, 16385, 24577};
static const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8,
                                       9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
struct WaveTableScratch { uint16_t sorted[320]; };
// the serial builder the wave-cooperative one equals
template <int TYPE>
inline int build_table_wave(const uint8_t* lens, unsigned n, uint16_t* tab, unsigned req_root,
                            WaveTableScratch& S, unsigned& root_out, unsigned& used_out, unsigned& lmin_out)
{
    unsigned root = req_root, used = 0;
    const int r = build_table(TYPE, lens, n, tab, &root, &used, S.sorted, &lmin_out);
    if (r) return r;
    root_out = root;
    used_out = used;
    return 0;
}
}  // namespace bpmd
