// inflate_reader_backend.cpp -- TEST INFRASTRUCTURE.  The per-stream inflate
// ABI of include/beast_pmd.h over beast_amd/csrc/inflate_reader.h, on the
// CPU: the call protocol is the library's own, and its step is the kernel's
// own decoder (pmd_zstream.hip's zstream_run) compiled for the host through
// zstream_shim.h.  Built with plain g++ by tests/model/zstream_host.py;
// nothing under beast_amd/ loads it.
//
// Every call runs inside watched buffers: the input is followed by 64 bytes
// of the stream's poison value (the 16-byte staging loads read up to 15 of
// them) and the output room by 64 canary bytes.  A result over its room, a
// changed canary or a changed poison byte is recorded, and irb_calls() hands
// the count of calls and the record out.
#ifndef BPMD_ZSTREAM_HOST
#define BPMD_ZSTREAM_HOST
#endif
#include "zstream_shim.h"

#include "../../beast_amd/csrc/pmd_zstream.hip"

#include <new>
#include <vector>

#include "../../beast_amd/csrc/inflate_reader.h"

namespace {

constexpr size_t SLACK = 64;
constexpr uint8_t CANARY = 0xA5;

}  // namespace

struct bpmd_stream {
    bpmd::InflateReader r;
    bpmd::zst::State st{};
    uint8_t poison = 0;
    unsigned long long calls = 0;
    unsigned violations = 0;   // 1: out_used > cap, 2: a store past out + cap, 4: a store past in + n
};

extern "C" size_t zs_host_state_bytes(void) { return sizeof(bpmd::zst::State); }

// inflate_stream::doReset on a State image (also the fresh images of tests/test_gpu_zstream_guard.py)
extern "C" void zs_host_reset(void* st, int wbits)
{
    bpmd::zst::State* s = (bpmd::zst::State*)st;
    memset(&s->h, 0, sizeof s->h);
    s->h.mode = bpmd::zst::HEAD;
    s->h.wbits = (uint32_t)wbits;
}

namespace {

int host_step(void* ctx, bpmd::InflateStep& c)
{
    bpmd_stream* s = (bpmd_stream*)ctx;
    if (c.reset) {
        zs_host_reset(&s->st, c.wbits);
        c.reset = false;
    }
    static thread_local bpmd::zst::Lds L;
    // BPMD_ZSTREAM_PAR=0: the serial inflate_fast loop (default: the parallel one, one lane)
    const char* e = getenv("BPMD_ZSTREAM_PAR");
    const char* hp = getenv("BPMD_ZSTREAM_HPAR");   // 0: the serial code-length loop
    const int par = (e ? atoi(e) != 0 : 1) | (hp && hp[0] == '0' ? 8 : 0);
    std::vector<uint8_t> in(c.n + SLACK, s->poison), out(c.cap + SLACK, CANARY);
    if (c.n) memcpy(in.data(), c.in, c.n);
    bpmd::zst::zstream_run(L, &s->st, in.data(), c.n, out.data(), c.cap, c.flush, &c.res, par);
    ++s->calls;
    unsigned v = c.res.out_used > c.cap ? 1u : 0u;
    for (size_t i = 0; i < SLACK; ++i) v |= (out[c.cap + i] != CANARY ? 2u : 0u) | (in[c.n + i] != s->poison ? 4u : 0u);
    s->violations |= v;
    if (v & 1u) return BPMD_R_INVALID_ARGUMENT;
    // (the output lands in the caller's buffer whether or not done() publishes it)
    if (c.res.out_used) memcpy(c.out, out.data(), c.res.out_used);
    return BPMD_R_OK;
}

}  // namespace

extern "C" {

int bpmd_inflate_stream_create(int window_bits, bpmd_stream** out)
{
    if (!out) return BPMD_R_INVALID_ARGUMENT;
    *out = nullptr;
    bpmd_stream* s = new (std::nothrow) bpmd_stream();
    if (!s) return BPMD_R_INVALID_ARGUMENT;
    const int r = s->r.create(window_bits);
    if (r) {
        delete s;
        return r;
    }
    s->r.run = host_step;
    s->r.ctx = s;
    *out = s;
    return BPMD_R_OK;
}

int bpmd_inflate_stream_reset(bpmd_stream* s, int window_bits) { return !s ? BPMD_R_INVALID_ARGUMENT : s->r.reset(window_bits); }

int bpmd_inflate_stream_clear(bpmd_stream* s) { return !s ? BPMD_R_INVALID_ARGUMENT : s->r.clear(); }

int bpmd_inflate_stream_write(bpmd_stream* s, bpmd_zparams* zs, int flush)
{
    return !s ? BPMD_R_INVALID_ARGUMENT : s->r.write(zs, flush);
}

void bpmd_stream_destroy(bpmd_stream* s) { delete s; }

// test only: the byte that follows every input of the stream from now on
void irb_poison(bpmd_stream* s, int poison) { s->poison = (uint8_t)poison; }

// test only: the number of decoder calls so far; *violations, if given, gets the record's bits
unsigned long long irb_calls(const bpmd_stream* s, unsigned* violations)
{
    if (violations) *violations = s->violations;
    return s->calls;
}

}  // extern "C"
