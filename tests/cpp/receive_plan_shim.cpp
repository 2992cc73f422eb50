// C entry points over beast_amd/csrc/receive_plan.h for
// tests/test_receive_plan.py (plain g++, no HIP): each hands one of the
// header's functions to ctypes.
#include <stdint.h>

#include "receive_plan.h"

using namespace bpmd::rp;

extern "C" uint32_t rp_effective_cap(uint32_t msg_cap, uint64_t msg_max) { return effective_cap(msg_cap, msg_max); }
// o: in_len, eff_cap, text
extern "C" void rp_select(uint32_t event, int32_t status, uint32_t compressed, uint32_t op, uint32_t out_len,
                          uint32_t msg_cap, uint64_t msg_max, uint32_t* o)
{
    const Select s = select(event, status, compressed, op, out_len, msg_cap, msg_max);
    o[0] = s.in_len, o[1] = s.eff_cap, o[2] = s.text;
}
// o: src, msg_len; returns the status
extern "C" int32_t rp_merge(uint32_t event, int32_t status, uint32_t compressed, uint32_t op, uint32_t out_len,
                            uint32_t msg_cap, uint64_t msg_max, int32_t zst, uint32_t z_len, uint32_t* o)
{
    const Merge m = merge(event, status, compressed, op, out_len, msg_cap, msg_max, zst, z_len);
    o[0] = m.src, o[1] = m.msg_len;
    return m.status;
}
extern "C" void rp_constants(uint32_t* o)
{
    o[0] = EV_MESSAGE, o[1] = OP_TEXT, o[2] = E_NEED_BUFFERS, o[3] = E_BAD_FRAME_PAYLOAD, o[4] = E_BUFFER_OVERFLOW;
    o[5] = E_MESSAGE_TOO_BIG, o[6] = SRC_NONE, o[7] = SRC_GATHERED, o[8] = SRC_INFLATED;
}
