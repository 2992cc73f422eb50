// inflate_reader.h -- the per-stream inflater's call protocol:
// zlib::inflate_stream's write() / reset() / clear() as the C ABI makes them,
// without the device.  Plain C++ (no HIP): the one step that needs the
// decoder -- run inflate_stream.ipp's state machine over this input into this
// room -- is a function the owner supplies (pmd_stream.hip: the inflate
// transport; tests/cpp/inflate_reader_backend.cpp: the kernel's own source
// built for the host).
//
// The decoder's state stays with the step's owner (zstream.h State); a
// write() hands the step the caller's input and bounded output room and
// advances z_params by the step's done() record -- the reference's total_in
// (input left unconsumed stays with the caller), total_out and data_type; an
// error returns without advancing them, as err() does.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/beast_pmd.h"
#include "zstream.h"

namespace bpmd {

// One write() as the decoder sees it, and the record it hands back.
struct InflateStep {
    const uint8_t* in;   // the caller's input
    size_t n;
    uint8_t* out;        // the caller's output room, after the bound
    size_t cap;
    int flush;
    bool reset;          // in: a reset(wbits) to apply first; out: false once it is applied
    int wbits;
    zst::Result res{};
};
// returns 0 or a negative bpmd_result
using InflateFn = int (*)(void* ctx, InflateStep& step);

struct InflateReader {
    InflateFn run = nullptr;
    void* ctx = nullptr;
    int wbits = 15;
    bool zreset = true;   // a reset() to apply before the next write()

    int create(int window_bits)
    {
        if (window_bits < 8 || window_bits > 15) return BPMD_R_DOMAIN_ERROR;   // inflate_stream.ipp:57-61
        wbits = window_bits;
        return BPMD_R_OK;
    }

    int reset(int window_bits)
    {
        if (window_bits < 8 || window_bits > 15) return BPMD_R_DOMAIN_ERROR;
        wbits = window_bits;
        zreset = true;   // applied before the next write()
        return BPMD_R_OK;
    }

    // inflate_stream::clear -> doClear is empty in the reference
    // (inflate_stream.ipp:49-53): state and window persist
    int clear() { return BPMD_R_OK; }

    int write(bpmd_zparams* zs, int flush)
    {
        if (!zs || flush < BPMD_FLUSH_NONE || flush > BPMD_FLUSH_TREES) return BPMD_R_INVALID_ARGUMENT;
        if ((!zs->next_in && zs->avail_in) || (!zs->next_out && zs->avail_out)) return BPMD_STREAM_ERROR;
        InflateStep st;
        st.in = (const uint8_t*)zs->next_in;
        st.n = zs->avail_in;
        // Output room handed to the kernel.  A call cannot produce more than the
        // pending match (<= 258) plus 258 bytes per 2 bits of the input and the
        // reservoir (<= 32 bits), so a room of at least that plus 258 leaves the
        // reference's "avail_out >= 258" fast-path test unchanged.
        const size_t bound = 1040 * st.n + 8192;
        st.out = (uint8_t*)zs->next_out;
        st.cap = std::min<size_t>(zs->avail_out, bound);
        st.flush = flush;
        st.reset = zreset;
        st.wbits = wbits;
        const int r = run(ctx, st);
        zreset = st.reset;   // still pending only if applying it failed
        if (r) return r;
        const zst::Result& res = st.res;
        if (res.published) {
            zs->next_in = (const uint8_t*)zs->next_in + res.in_used;
            zs->avail_in -= res.in_used;
            zs->total_in += res.in_used;
            zs->next_out = (uint8_t*)zs->next_out + res.out_used;
            zs->avail_out -= res.out_used;
            zs->total_out += res.out_used;
            zs->data_type = res.data_type;
        }
        return res.ec;
    }
};

}  // namespace bpmd
