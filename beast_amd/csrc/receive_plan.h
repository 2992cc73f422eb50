// receive_plan.h -- the per-entry rules of the batch receive side in one
// chained call (bpmd_receive_batch, pmd_receive.hip): which entries of the
// frame pass reach the inflater and with what room, and how the inflater's
// result, rd_msg_max on the inflated size (websocket/impl/read.hpp:1357-1367)
// and the UTF-8 check of text (read.hpp:1372-1384) merge into the entry's
// status.  Pure functions of one entry's values.
// Host-compilable without HIP: tests/test_receive_plan.py compares it with a
// Python model (tests/receive_model.py), tests/cpp/receive_plan_main.cpp runs
// it under the address sanitizer; the kernels of pmd_receive.hip call the same
// functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BPMD_RP_HD __host__ __device__ inline
#else
#define BPMD_RP_HD inline
#endif

namespace bpmd {
namespace rp {

// the frame pass's event and opcode values this side looks at (frame_parse.h)
enum : uint32_t { EV_MESSAGE = 1, OP_TEXT = 1 };
// per-entry outcomes, numbered as include/beast_pmd.h does
enum : int32_t { E_NEED_BUFFERS = 1, E_BAD_FRAME_PAYLOAD = 256, E_BUFFER_OVERFLOW = 257, E_MESSAGE_TOO_BIG = 258 };
// where the finish pass reads the bytes it checks as UTF-8
enum : uint32_t { SRC_NONE = 0, SRC_GATHERED = 1, SRC_INFLATED = 2 };

// The entry completed a compressed message: the only kind that is inflated.
BPMD_RP_HD bool inflates(uint32_t event, int32_t status, uint32_t compressed)
{
    return event == EV_MESSAGE && status == 0 && compressed != 0;
}

// The room the inflater gets: one byte past msg_max (0 = no limit) is enough
// to tell a message over the limit from one that reaches it, and no more than
// the slot.  msg_max + 1 is not formed when it would not fit 32 bits (nor 64).
BPMD_RP_HD uint32_t effective_cap(uint32_t msg_cap, uint64_t msg_max)
{
    if (msg_max == 0 || msg_max >= 0xffffffffull) return msg_cap;
    const uint32_t limit = (uint32_t)msg_max + 1u;
    return msg_cap < limit ? msg_cap : limit;
}

struct Select {
    uint32_t in_len;    // the inflater's input length (0: the entry is skipped)
    uint32_t eff_cap;   // the inflater's output capacity
    uint32_t text;      // the inflated output is a text message
};

BPMD_RP_HD Select select(uint32_t event, int32_t status, uint32_t compressed, uint32_t op, uint32_t out_len,
                         uint32_t msg_cap, uint64_t msg_max)
{
    Select s;
    const bool z = inflates(event, status, compressed);
    s.in_len = z ? out_len : 0u;
    s.eff_cap = z ? effective_cap(msg_cap, msg_max) : 0u;
    s.text = z && op == OP_TEXT ? 1u : 0u;
    return s;
}

struct Merge {
    int32_t status;     // the entry's status before the UTF-8 check
    uint32_t src;       // SRC_*: the bytes to check as UTF-8 (status 0 and text only)
    uint32_t msg_len;   // the message's length (0 without a complete message)
};

// zst, z_len: the inflater's status and output length at the effective
// capacity (looked at for an inflated entry only).  An entry that did not
// complete a message, or whose frame pass reported an error, keeps its status.
// A zlib error is reported in stream order, so one that precedes the limit
// wins; need_buffers means the message outgrew the effective capacity, which
// is the limit when msg_max <= msg_cap and the slot otherwise.
BPMD_RP_HD Merge merge(uint32_t event, int32_t status, uint32_t compressed, uint32_t op, uint32_t out_len,
                       uint32_t msg_cap, uint64_t msg_max, int32_t zst, uint32_t z_len)
{
    Merge m;
    m.status = status, m.src = SRC_NONE, m.msg_len = 0;
    if (event != EV_MESSAGE || status != 0) return m;
    if (compressed == 0) {
        m.msg_len = out_len;
        if (op == OP_TEXT) m.src = SRC_GATHERED;
        return m;
    }
    m.msg_len = z_len;
    if (zst == E_NEED_BUFFERS) m.status = (msg_max && msg_max <= msg_cap) ? E_MESSAGE_TOO_BIG : E_BUFFER_OVERFLOW;
    else if (zst != 0) m.status = zst;
    else if (msg_max && z_len > msg_max) m.status = E_MESSAGE_TOO_BIG;
    if (m.status == 0 && op == OP_TEXT) m.src = SRC_INFLATED;
    return m;
}

}  // namespace rp
}  // namespace bpmd
