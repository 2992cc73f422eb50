// C entry points over beast_amd/csrc/send_takeover_plan.h for
// tests/test_send_takeover_plan.py (plain g++, no HIP): each hands one of the
// header's functions to ctypes.
#include <stdint.h>

#include "send_takeover_plan.h"

using namespace bpmd;

extern "C" uint32_t stp_keep(void) { return stp::K; }
extern "C" uint32_t stp_room(uint32_t max_len, uint32_t slot) { return stp::room(max_len, slot, stp::K); }
extern "C" int stp_deflates(uint32_t op, int opt, uint64_t len, uint64_t threshold)
{
    return stp::deflates(op, opt != 0, len, threshold) ? 1 : 0;
}
extern "C" int32_t stp_provisional(uint32_t op, int deflates, uint64_t len, uint32_t L)
{
    return stp::provisional(op, deflates != 0, len, L);
}
// o: slide, new_pos, z_len, hist
extern "C" void stp_place(uint32_t pos, uint32_t len, uint32_t slot, int enters, uint32_t* o)
{
    const stp::Place p = stp::place(pos, len, slot, stp::K, enters != 0);
    o[0] = p.slide, o[1] = p.new_pos, o[2] = p.z_len, o[3] = p.hist;
}
extern "C" int32_t stp_merge(int32_t provisional, int enters, int32_t zst) { return stp::merge(provisional, enters != 0, zst); }
extern "C" uint32_t stp_advance(uint32_t new_pos, uint32_t len, int enters, int32_t status)
{
    return stp::advance(new_pos, len, enters != 0, status);
}
extern "C" uint64_t stp_chunk_bound(uint32_t n, uint32_t L) { return stp::chunk_bound(n, L); }
