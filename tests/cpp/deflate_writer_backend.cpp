// deflate_writer_backend.cpp -- TEST INFRASTRUCTURE.  The per-stream deflate
// ABI of include/beast_pmd.h over beast_amd/csrc/deflate_writer.h alone: the
// call protocol on the CPU, with a stand-in for the device step.  Built with
// plain g++ by tests/test_deflate_writer.py; nothing under beast_amd/ loads it.
//
// The stand-in emits its input as stored blocks of at most 65,535 bytes
// (BFINAL 0, each padded from bit 0 of the output, as the kernels' are) and
// one empty static block (010 + 0000000), so the bit count it returns,
// 8 * (n + 5 * blocks) + 10, is no multiple of 8.  Level, strategy, tune
// values and history change none of its bytes; it records them per call, and
// dwb_calls() hands the record out.
#include <cassert>
#include <new>

#include "../../beast_amd/csrc/deflate_writer.h"

namespace {

constexpr int REC = 9;   // level, strategy, tuned, tune[4], hist_len, n

}  // namespace

struct bpmd_stream {
    bool is_deflate = true;
    bpmd::DeflateWriter w;
    std::vector<long long> calls;   // REC values per compress call
};

namespace {

int stand_in(void* ctx, bpmd::DeflateStep& st)
{
    bpmd_stream* s = (bpmd_stream*)ctx;
    const long long rec[REC] = {st.level,
                                st.strategy,
                                st.tune != nullptr,
                                st.tune ? st.tune[0] : 0,
                                st.tune ? st.tune[1] : 0,
                                st.tune ? st.tune[2] : 0,
                                st.tune ? st.tune[3] : 0,
                                (long long)st.hist_len,
                                (long long)st.n};
    s->calls.insert(s->calls.end(), rec, rec + REC);
    size_t blocks = 0;
    for (size_t at = 0; at < st.n; at += 65535, ++blocks) {
        const size_t len = std::min<size_t>(st.n - at, 65535);
        const uint8_t head[5] = {0, (uint8_t)len, (uint8_t)(len >> 8), (uint8_t)~len, (uint8_t)(~len >> 8)};
        st.out.insert(st.out.end(), head, head + 5);
        st.out.insert(st.out.end(), st.in + at, st.in + at + len);
    }
    st.out.push_back(1u << 1);   // BFINAL 0, BTYPE 01, and 5 of the end-of-block code's 7 zeros
    st.out.push_back(0);         // its last 2
    st.bits = (uint32_t)(8 * (st.n + 5 * blocks) + 10);
    st.status = BPMD_OK;
    assert(st.out.size() <= st.out_cap && st.out_cap == bpmd_deflate_upper_bound(st.n) + 16);
    return BPMD_R_OK;
}

}  // namespace

extern "C" {

// pmd_capi.hip's (zlib/deflate_stream.hpp:402-410)
size_t bpmd_deflate_upper_bound(size_t n) { return n + ((n + 7) >> 3) + ((n + 63) >> 6) + 11; }

int bpmd_deflate_stream_create(int level, int window_bits, int mem_level, int strategy, bpmd_stream** out)
{
    if (!out) return BPMD_R_INVALID_ARGUMENT;
    *out = nullptr;
    bpmd_stream* s = new (std::nothrow) bpmd_stream();
    if (!s) return BPMD_R_INVALID_ARGUMENT;
    const int r = s->w.create(level, window_bits, mem_level, strategy);
    if (r) {
        delete s;
        return r;
    }
    s->w.compress = stand_in;
    s->w.ctx = s;
    *out = s;
    return BPMD_R_OK;
}

int bpmd_deflate_stream_reset(bpmd_stream* s) { return (!s || !s->is_deflate) ? BPMD_R_INVALID_ARGUMENT : s->w.reset(); }

int bpmd_deflate_stream_write(bpmd_stream* s, bpmd_zparams* zs, int flush)
{
    return (!s || !s->is_deflate || !zs) ? BPMD_R_INVALID_ARGUMENT : s->w.write(zs, flush);
}

int bpmd_deflate_stream_params(bpmd_stream* s, bpmd_zparams* zs, int level, int strategy)
{
    return (!s || !s->is_deflate || !zs) ? BPMD_R_INVALID_ARGUMENT : s->w.params(zs, level, strategy);
}

int bpmd_deflate_stream_tune(bpmd_stream* s, int good_length, int max_lazy, int nice_length, int max_chain)
{
    return (!s || !s->is_deflate) ? BPMD_R_INVALID_ARGUMENT : s->w.tune(good_length, max_lazy, nice_length, max_chain);
}

int bpmd_deflate_stream_pending(bpmd_stream* s, unsigned* value, int* bits)
{
    return (!s || !s->is_deflate) ? BPMD_R_INVALID_ARGUMENT : s->w.pending(value, bits);
}

int bpmd_deflate_stream_prime(bpmd_stream* s, int bits, int value)
{
    return (!s || !s->is_deflate) ? BPMD_R_INVALID_ARGUMENT : s->w.prime(bits, value);
}

void bpmd_stream_destroy(bpmd_stream* s) { delete s; }

// test only: the stream's compress calls so far, REC values each (level,
// strategy, tuned, the four tune values, history length, input length); up to
// cap calls are written to out, and the number made is returned
size_t dwb_calls(const bpmd_stream* s, long long* out, size_t cap)
{
    const size_t n = s->calls.size() / REC;
    std::copy(s->calls.begin(), s->calls.begin() + (ptrdiff_t)(std::min(n, cap) * REC), out);
    return n;
}

// test only: the bytes of history the writer keeps (DeflateWriter::HIST_KEEP)
size_t dwb_hist_keep(void) { return bpmd::DeflateWriter::HIST_KEEP; }

}  // extern "C"
