// status.h -- the per-message status values: Beast's zlib::error
// (include/boost/beast/zlib/error.hpp:48-138).  HIP-free: pmd_common.h takes
// them from here, and so do the host models of kernel code (tests/cpp/*_shim.h).
#pragma once
#include <stdint.h>

namespace bpmd {

enum Status : int32_t {
    ST_OK = 0,
    ST_NEED_BUFFERS = 1,
    ST_END_OF_STREAM = 2,
    ST_NEED_DICT = 3,
    ST_STREAM_ERROR = 4,
    ST_INVALID_BLOCK_TYPE = 5,
    ST_INVALID_STORED_LENGTH = 6,
    ST_TOO_MANY_SYMBOLS = 7,
    ST_INVALID_CODE_LENGTHS = 8,
    ST_INVALID_BIT_LENGTH_REPEAT = 9,
    ST_MISSING_EOB = 10,
    ST_INVALID_LITERAL_LENGTH = 11,
    ST_INVALID_DISTANCE_CODE = 12,
    ST_INVALID_DISTANCE = 13,
    ST_OVER_SUBSCRIBED_LENGTH = 14,
    ST_INCOMPLETE_LENGTH_SET = 15,
    ST_GENERAL = 16,
};

}  // namespace bpmd
