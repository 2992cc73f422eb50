// exact_shim.h -- TEST INFRASTRUCTURE.  One-lane meanings of the HIP keywords
// and intrinsics that beast_amd/csrc/deflate_exact_core.h uses, so that its
// text compiles as plain C++ (lane 0, WAVE = 1, a ballot of one lane,
// readfirstlane = identity, no fences).  Included by exact_host_backend.cpp
// ahead of the core.  The compiler is clang++: the core uses
// __builtin_bitreverse32.
#pragma once
#include <stddef.h>
#include <stdint.h>
#define __device__
#define __forceinline__ inline
#define __constant__
#define __restrict__
#include "../../beast_amd/csrc/status.h"
namespace bpmd {
constexpr int WAVE = 1;
inline unsigned lane_id() { return 0; }
}  // namespace bpmd
static inline uint64_t __ballot(bool b) { return b ? 1ull : 0ull; }
#define __builtin_amdgcn_fence(a, b) ((void)0)
#define __builtin_amdgcn_readfirstlane(v) (v)
