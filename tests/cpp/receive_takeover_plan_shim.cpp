// C entry points over beast_amd/csrc/receive_takeover_plan.h for
// tests/test_receive_takeover_plan.py (plain g++, no HIP): each hands one of
// the header's functions to ctypes.
#include <stdint.h>

#include "receive_takeover_plan.h"

using namespace bpmd;

extern "C" uint32_t rtp_room(uint32_t msg_cap, uint32_t slot, uint32_t W) { return rtp::room(msg_cap, slot, W); }
// the capacity the place kernel hands to place(): rp::select under room()
extern "C" uint32_t rtp_effective_cap(uint32_t msg_cap, uint64_t msg_max, uint32_t slot, uint32_t W)
{
    return rp::effective_cap(rtp::room(msg_cap, slot, W), msg_max);
}
// o: slide, new_pos, hist
extern "C" void rtp_place(uint32_t pos, uint32_t eff_cap, uint32_t slot, uint32_t W, int inflates, uint32_t* o)
{
    const rtp::Place p = rtp::place(pos, eff_cap, slot, W, inflates != 0);
    o[0] = p.slide, o[1] = p.new_pos, o[2] = p.hist;
}
extern "C" uint32_t rtp_advance(uint32_t pos, int inflates, int32_t zst, uint32_t z_len)
{
    return rtp::advance(pos, inflates != 0, zst, z_len);
}
