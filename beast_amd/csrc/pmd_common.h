// pmd_common.h -- shared device definitions for the permessage-deflate
// kernels (gfx950 / CDNA4, wave64).
//
// Status values (Beast's zlib::error) are status.h's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "status.h"

namespace bpmd {

constexpr int WAVE = 64;

__device__ __forceinline__ unsigned lane_id() { return __lane_id(); }

// RFC 1951 §3.2.5 tables (index = symbol - 257 / distance symbol)
__constant__ static const uint16_t kLenBase[29] = {
    3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31,
    35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ static const uint8_t kLenExtra[29] = {
    0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ static const uint16_t kDistBase[30] = {
    1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193,
    257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ static const uint8_t kDistExtra[30] = {
    0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

}  // namespace bpmd
