// pmd_stream.hip -- per-stream entry points behind the C++ compatibility
// facade (include/beast_amd/zlib.hpp, include/boost/beast/zlib/*.hpp):
// zlib::deflate_stream / zlib::inflate_stream write() semantics, executed by
// the GPU kernels.  Host code only.
//
// The C ABI's forwards, the two call protocols' device steps, one Arena and
// two transports, each for a call alone and for a batch of them.
// deflate: the call protocol is deflate_writer.h (no HIP in it); its step
//   compresses a flush's bytes (deflate_group).
// inflate: the call protocol is inflate_reader.h (no HIP in it).  The
//   reference's decoder state lives on the device (zstream.h) and each
//   write() is one workgroup of the per-stream kernel (pmd_zstream.hip),
//   which runs inflate_stream.ipp's state machine with its bit reservoir and
//   window: the step uploads the caller's input, the kernel decodes exactly
//   what the reference would, and the output and the kernel's done() record
//   come back (inflate_batch).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/beast_pmd.h"
#include "deflate_writer.h"
#include "inflate_reader.h"
#include "pmd_internal.h"
#include "zstream.h"

namespace {

// a device block, its pinned mirror and the HIP stream they use: a
// coalescer's leader's, or a stream's own when the batcher is off
struct Arena {
    hipStream_t hs = nullptr;
    uint8_t* d = nullptr;
    uint8_t* h = nullptr;
    size_t cap = 0;
    size_t floor;   // the smallest block allocated
    explicit Arena(size_t floor_) : floor(floor_) {}
    bool reserve(size_t need)
    {
        if (!hs && hipStreamCreateWithFlags(&hs, hipStreamNonBlocking) != hipSuccess) {
            hs = nullptr;
            return false;
        }
        if (need <= cap) return true;
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
        cap = 0;
        const size_t c = std::max<size_t>(need + need / 2, floor);
        if (hipMalloc((void**)&d, c) != hipSuccess) {
            d = nullptr;
            return false;
        }
        if (hipHostMalloc((void**)&h, c, hipHostMallocDefault) != hipSuccess) {
            (void)hipFree(d);
            d = h = nullptr;
            return false;
        }
        cap = c;
        return true;
    }
};

}  // namespace

// a deflater or an inflater
struct bpmd_stream {
    bool is_deflate = true;
    bpmd::DeflateWriter def;
    bpmd::InflateReader inf;
    void* zst = nullptr;   // inflate: the device state (zstream.h State + Result)
    // the batcher off: the stream's own block (64 KiB at least: a server may
    // hold thousands of these), made by its first flush or write
    Arena arena{1 << 16};
};

namespace {

int run_flush(void* stream, bpmd::DeflateStep& st);
int run_inflate(void* stream, bpmd::InflateStep& st);

}  // namespace

extern "C" int bpmd_deflate_stream_create(int level, int window_bits, int mem_level, int strategy,
                                          bpmd_stream** out)
{
    if (!out) return BPMD_R_INVALID_ARGUMENT;
    *out = nullptr;
    bpmd_stream* s = new (std::nothrow) bpmd_stream();
    if (!s) return BPMD_R_INVALID_ARGUMENT;
    const int r = s->def.create(level, window_bits, mem_level, strategy);
    if (r) {
        delete s;
        return r;
    }
    s->def.compress = run_flush;
    s->def.ctx = s;
    *out = s;
    return BPMD_R_OK;
}

extern "C" int bpmd_deflate_stream_reset(bpmd_stream* s)
{
    return (!s || !s->is_deflate) ? BPMD_R_INVALID_ARGUMENT : s->def.reset();
}

extern "C" int bpmd_deflate_stream_write(bpmd_stream* s, bpmd_zparams* zs, int flush)
{
    return (!s || !s->is_deflate || !zs) ? BPMD_R_INVALID_ARGUMENT : s->def.write(zs, flush);
}

extern "C" int bpmd_deflate_stream_params(bpmd_stream* s, bpmd_zparams* zs, int level, int strategy)
{
    return (!s || !s->is_deflate || !zs) ? BPMD_R_INVALID_ARGUMENT : s->def.params(zs, level, strategy);
}

extern "C" int bpmd_deflate_stream_tune(bpmd_stream* s, int good_length, int max_lazy, int nice_length, int max_chain)
{
    return (!s || !s->is_deflate) ? BPMD_R_INVALID_ARGUMENT
                                  : s->def.tune(good_length, max_lazy, nice_length, max_chain);
}

extern "C" int bpmd_deflate_stream_pending(bpmd_stream* s, unsigned* value, int* bits)
{
    return (!s || !s->is_deflate) ? BPMD_R_INVALID_ARGUMENT : s->def.pending(value, bits);
}

extern "C" int bpmd_deflate_stream_prime(bpmd_stream* s, int bits, int value)
{
    return (!s || !s->is_deflate) ? BPMD_R_INVALID_ARGUMENT : s->def.prime(bits, value);
}

extern "C" int bpmd_inflate_stream_create(int window_bits, bpmd_stream** out)
{
    if (!out) return BPMD_R_INVALID_ARGUMENT;
    *out = nullptr;
    bpmd_stream* s = new (std::nothrow) bpmd_stream();
    if (!s) return BPMD_R_INVALID_ARGUMENT;
    const int r = s->inf.create(window_bits);
    if (r) {
        delete s;
        return r;
    }
    s->is_deflate = false;
    s->inf.run = run_inflate;
    s->inf.ctx = s;
    *out = s;
    return BPMD_R_OK;
}

extern "C" int bpmd_inflate_stream_reset(bpmd_stream* s, int window_bits)
{
    return (!s || s->is_deflate) ? BPMD_R_INVALID_ARGUMENT : s->inf.reset(window_bits);
}

extern "C" int bpmd_inflate_stream_clear(bpmd_stream* s)
{
    return (!s || s->is_deflate) ? BPMD_R_INVALID_ARGUMENT : s->inf.clear();
}

extern "C" int bpmd_inflate_stream_write(bpmd_stream* s, bpmd_zparams* zs, int flush)
{
    return (!s || s->is_deflate) ? BPMD_R_INVALID_ARGUMENT : s->inf.write(zs, flush);
}

namespace {

using bpmd::zst::Head;
using bpmd::zst::Result;
using bpmd::zst::State;

// inflate_stream::doReset (inflate_stream.ipp:55-72): HEAD, empty reservoir,
// empty window of 2^windowBits
Head fresh_head(int window_bits)
{
    Head h{};
    h.mode = bpmd::zst::HEAD;
    h.wbits = (uint32_t)window_bits;
    return h;
}

// the stream's device state, and the step's pending reset applied to it
int ensure_zhead(bpmd_stream* s, bpmd::InflateStep& st)
{
    if (!s->zst) {
        if (hipMalloc(&s->zst, sizeof(State) + sizeof(Result)) != hipSuccess) {
            s->zst = nullptr;
            return BPMD_R_HIP_ERROR;
        }
        st.reset = true;
    }
    if (st.reset) {
        const Head h = fresh_head(st.wbits);
        if (hipMemcpy(s->zst, &h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) return BPMD_R_HIP_ERROR;
        st.reset = false;
    }
    return BPMD_R_OK;
}

}  // namespace

// ------------------------------------------------------------ micro-batcher
// write() calls of different streams made at the same time
// -- a server's connections, each reading and writing on its own thread or
// strand (impl_base.hpp:85-190 inflate / deflate calls, write.hpp:463-545)
// -- run as one launch.  A call queues itself; if no batch is running it
// becomes the leader: it takes up to max_calls queued calls (one per stream),
// runs them together and wakes their callers.  Calls that arrive while a
// batch runs form the next one (a group commit: no added latency when a
// stream is alone -- its batch is one call), and
// max_delay_us > 0 lets a leader wait that long for more.  Every call's
// result is its single-call result: the inflate launch runs the same
// per-stream state machine for each stream (one workgroup per call,
// pmd_zstream.hip), the deflate launch the same per-message kernels, whose
// bytes do not depend on the batch's other messages.
namespace {

// a queued call: its stream (one call per stream and batch), the protocol's
// step record, and the call's return code
template <class Step>
struct Job {
    const bpmd_stream* s = nullptr;
    Step* st = nullptr;
    int rc = 0;
    bool done = false;
};
using InflateJob = Job<bpmd::InflateStep>;
using DeflateJob = Job<bpmd::DeflateStep>;

// settings: max_calls < 2 is off
std::atomic<int> g_bmax{-1}, g_bdelay{-1};
// [0] inflate calls, [1] inflate launches, [2] deflate flushes, [3] deflate launches
std::atomic<unsigned long long> g_bstat[4];

int batch_max()
{
    int m = g_bmax.load();
    if (m < 0) {
        const char* e = getenv("BPMD_STREAM_BATCH");
        m = e ? std::max(0, std::min(atoi(e), 4096)) : 256;
        const char* d = getenv("BPMD_STREAM_BATCH_DELAY_US");
        g_bdelay.store(d ? std::max(0, atoi(d)) : 0);
        g_bmax.store(m);
    }
    return m;
}

template <class Job>
class Coalescer {
  public:
    explicit Coalescer(int dev) : dev_(dev) {}
    template <class Exec>
    void run(Job* j, int max_calls, Exec&& exec)
    {
        std::unique_lock<std::mutex> lk(mu_);
        q_.push_back(j);
        if (busy_) arrive_.notify_one();
        while (!j->done) {
            if (busy_) {
                done_.wait(lk);
                continue;
            }
            busy_ = true;
            const int delay = g_bdelay.load();
            if (delay > 0 && q_.size() < (size_t)max_calls)
                arrive_.wait_for(lk, std::chrono::microseconds(delay), [&] { return q_.size() >= (size_t)max_calls; });
            // in arrival order, one call per stream (a stream's calls are
            // its owner's sequence: a second one waits for the next batch)
            std::vector<Job*> take;
            for (auto it = q_.begin(); it != q_.end() && take.size() < (size_t)max_calls;) {
                bool dup = false;
                for (const Job* t : take) dup = dup || t->s == (*it)->s;
                if (dup) {
                    ++it;
                    continue;
                }
                take.push_back(*it);
                it = q_.erase(it);
            }
            lk.unlock();
            // the coalescer's device (its streams' state lives there), whatever
            // this thread had current
            int prev = -1;
            (void)hipGetDevice(&prev);
            if (prev != dev_) (void)hipSetDevice(dev_);
            exec(arena_, take);
            if (prev != dev_ && prev >= 0) (void)hipSetDevice(prev);
            lk.lock();
            for (Job* t : take) t->done = true;
            busy_ = false;
            done_.notify_all();
        }
    }

  private:
    std::mutex mu_;
    std::condition_variable done_, arrive_;
    std::deque<Job*> q_;
    bool busy_ = false;
    Arena arena_{1 << 20};
    int dev_;
};

// one per direction and device: a stream's device state lives on the device
// its owner had current, and calls only batch with calls of the same device.
// Process-lifetime objects (never destroyed: HIP may be torn down first).
constexpr int MAX_DEV = 64;
template <class Job>
Coalescer<Job>* coalescer(int dev)
{
    static std::mutex mu;
    static Coalescer<Job>* tab[MAX_DEV] = {};
    if (dev < 0 || dev >= MAX_DEV) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    Coalescer<Job>*& c = tab[dev];
    if (!c) c = new (std::nothrow) Coalescer<Job>(dev);
    return c;
}

constexpr size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

template <class Job>
void fail_all(std::vector<Job*>& jobs, hipStream_t hs)
{
    if (hs) (void)hipStreamSynchronize(hs);   // no DMA may still use the pinned mirror
    for (Job* j : jobs) j->rc = BPMD_R_HIP_ERROR;
}

// A batch's way back, after its copies in and its launch: one D2H of the
// results at `at` (`head` bytes) and a wait; each call's used output then
// follows in a copy of its own and a second wait, unless results and outputs
// together (`all` bytes from `at`) are at most 4 MiB and came with the first.
// used(i, len, room): call i's output length and room, read from the results
// in the pinned mirror; off[i]: its output's place in the block.
template <class Used>
bool read_back(Arena& A, size_t at, size_t head, size_t all, const std::vector<size_t>& off, Used&& used)
{
    const bool whole = all <= (4u << 20);
    bool ok = hipMemcpyAsync(A.h + at, A.d + at, whole ? all : head, hipMemcpyDeviceToHost, A.hs) == hipSuccess &&
              hipStreamSynchronize(A.hs) == hipSuccess;
    for (size_t i = 0; i < off.size() && ok; ++i) {
        size_t len = 0, room = 0;
        used(i, len, room);
        ok = len <= room;
        if (ok && !whole && len)
            ok = hipMemcpyAsync(A.h + off[i], A.d + off[i], len, hipMemcpyDeviceToHost, A.hs) == hipSuccess;
    }
    if (ok && !whole) ok = hipStreamSynchronize(A.hs) == hipSuccess;
    return ok;
}

// The inflate transport: k write() calls as one launch (a call alone is k = 1).
// Block: [ZCall k][inputs][Result k][outputs]; one H2D of calls + inputs, the
// launch, one D2H of the results and outputs (of the results alone, then each
// call's used output, when the output room is over 4 MiB).  The output lands
// in the caller's buffer whether or not done() publishes it.
void inflate_batch(Arena& A, std::vector<InflateJob*>& jobs)
{
    using bpmd::zst::ZCall;
    const uint32_t k = (uint32_t)jobs.size();
    std::vector<size_t> ioff(k), ooff(k);
    // packed on the kernel's contract (tests/test_gpu_zstream_guard.py): no store at or past out + cap, and
    // results that do not depend on the 64 bytes after in + n_in (stale bytes of earlier batches here)
    size_t o = up256(sizeof(ZCall) * k);
    for (uint32_t i = 0; i < k; ++i) {
        ioff[i] = o;
        o = up256(o + jobs[i]->st->n + 64);   // + the staging loads' slack
    }
    const size_t res_at = o;
    o = up256(res_at + 64ull * k);
    for (uint32_t i = 0; i < k; ++i) {
        ooff[i] = o;
        o = up256(o + jobs[i]->st->cap);
    }
    const size_t total = o;
    if (!A.reserve(total)) return fail_all(jobs, A.hs);
    ZCall* zc = (ZCall*)A.h;
    for (uint32_t i = 0; i < k; ++i) {
        const bpmd::InflateStep& s = *jobs[i]->st;
        if (s.n) std::memcpy(A.h + ioff[i], s.in, s.n);
        ZCall c{};
        c.st = jobs[i]->s->zst;
        c.in = A.d + ioff[i];
        c.n_in = s.n;
        c.out = A.d + ooff[i];
        c.cap = s.cap;
        c.res = A.d + res_at + 64ull * i;
        c.flush = s.flush;
        zc[i] = c;
    }
    const bool ok = hipMemcpyAsync(A.d, A.h, res_at, hipMemcpyHostToDevice, A.hs) == hipSuccess &&
                    bpmd_internal_zstream_write_batch(A.d, k, A.hs) == 0 &&
                    read_back(A, res_at, 64ull * k, total - res_at, ooff, [&](size_t i, size_t& len, size_t& room) {
                        bpmd::InflateStep& s = *jobs[i]->st;
                        std::memcpy(&s.res, A.h + res_at + 64ull * i, sizeof(Result));
                        len = s.res.out_used;
                        room = s.cap;
                    });
    if (!ok) return fail_all(jobs, A.hs);
    for (uint32_t i = 0; i < k; ++i) {
        const bpmd::InflateStep& s = *jobs[i]->st;
        if (s.res.out_used) std::memcpy(s.out, A.h + ooff[i], s.res.out_used);
        jobs[i]->rc = BPMD_R_OK;
    }
}

// (a batch of one too.  With the batcher on, streams use the leaders' blocks
// and HIP streams and allocate none of their own -- creating a HIP stream or
// pinned buffer per connection serializes in the runtime; with it off a call
// is inflate_batch of one on the stream's own arena, run_inflate)
void inflate_exec(Arena& A, std::vector<InflateJob*>& jobs)
{
    g_bstat[1].fetch_add(1);
    inflate_batch(A, jobs);
}

// The deflate transport: flushes with the same parameters (level,
// windowBits, strategy, tune values, history or not) as one call of the
// deflater.  Block: [SoA meta][outputs][history + input, per flush]; H2D of
// meta and inputs, the kernels (the chunk count is known here: nothing is
// read back), one D2H of meta + outputs (meta, then each flush's output, past
// 4 MiB of room).
void deflate_group(Arena& A, std::vector<DeflateJob*>& jobs)
{
    const uint32_t k = (uint32_t)jobs.size();
    const bpmd::DeflateStep& s0 = *jobs[0]->st;
    const bool hist = s0.hist_len != 0;
    const size_t m_in_off = 0, m_out_off = 8ull * k, m_in_len = 16ull * k, m_out_cap = 20ull * k,
                 m_hist = 24ull * k, m_out_len = 28ull * k, m_bits = 32ull * k, m_status = 36ull * k;
    const size_t out_at = up256(40ull * k);
    std::vector<size_t> oo(k), io(k);   // in the block; in the inputs
    size_t o = out_at;
    for (uint32_t i = 0; i < k; ++i) {
        oo[i] = o;
        o = up256(o + jobs[i]->st->out_cap);
    }
    const size_t in_at = o;
    size_t ib = 0;
    uint64_t chunks = 0;
    for (uint32_t i = 0; i < k; ++i) {
        const bpmd::DeflateStep& s = *jobs[i]->st;
        if (s.n + s.hist_len > 0xFFFFFFFFu || s.out_cap > 0xFFFFFFFFu) {
            for (DeflateJob* j : jobs) j->rc = BPMD_R_INVALID_ARGUMENT;
            return;
        }
        io[i] = ib;
        ib = up256(ib + s.hist_len + s.n);
        chunks += bpmd::dfl::chunk_count((uint32_t)s.n, s.hist_len != 0);
    }
    const size_t total = in_at + ib + 16;
    if (!A.reserve(total)) return fail_all(jobs, A.hs);
    uint8_t* h = A.h;
    std::memset(h, 0, out_at);
    for (uint32_t i = 0; i < k; ++i) {
        const bpmd::DeflateStep& s = *jobs[i]->st;
        ((uint64_t*)(h + m_in_off))[i] = io[i] + s.hist_len;
        ((uint64_t*)(h + m_out_off))[i] = oo[i] - out_at;
        ((uint32_t*)(h + m_in_len))[i] = (uint32_t)s.n;
        ((uint32_t*)(h + m_out_cap))[i] = (uint32_t)s.out_cap;
        ((uint32_t*)(h + m_hist))[i] = (uint32_t)s.hist_len;
        if (s.hist_len) std::memcpy(h + in_at + io[i], s.hist, s.hist_len);
        if (s.n) std::memcpy(h + in_at + io[i] + s.hist_len, s.in, s.n);
    }
    uint8_t* d = A.d;
    const bpmd::Batch b{d + in_at, (const uint64_t*)(d + m_in_off), (const uint32_t*)(d + m_in_len), k, d + out_at,
                        (const uint64_t*)(d + m_out_off), (const uint32_t*)(d + m_out_cap), (uint32_t*)(d + m_out_len),
                        (int32_t*)(d + m_status)};
    // exact bit lengths, the stream's earlier plaintext as history, the chunk count known here
    bpmd::DeflateOpts zo;
    zo.level = s0.level, zo.window_bits = s0.wbits, zo.strategy = s0.strategy, zo.tune = s0.tune;
    zo.hist_len = hist ? (const uint32_t*)(d + m_hist) : nullptr, zo.out_bits = (uint32_t*)(d + m_bits);
    zo.chunks = {bpmd::dfl::ChunkSource::EXACT, chunks};
    const bool ok =
        hipMemcpyAsync(d, h, out_at, hipMemcpyHostToDevice, A.hs) == hipSuccess &&
        (ib == 0 || hipMemcpyAsync(d + in_at, h + in_at, ib, hipMemcpyHostToDevice, A.hs) == hipSuccess) &&
        bpmd::deflate(b, zo, A.hs) == 0 &&
        read_back(A, 0, out_at, in_at, oo, [&](size_t i, size_t& len, size_t& room) {
            len = ((const uint32_t*)(h + m_out_len))[i];
            room = jobs[i]->st->out_cap;
        });
    if (!ok) return fail_all(jobs, A.hs);
    for (uint32_t i = 0; i < k; ++i) {
        DeflateJob* j = jobs[i];
        const uint32_t len = ((const uint32_t*)(h + m_out_len))[i];
        j->st->out.assign(h + oo[i], h + oo[i] + len);
        j->st->status = ((const int32_t*)(h + m_status))[i];
        j->st->bits = ((const uint32_t*)(h + m_bits))[i];
        j->rc = BPMD_R_OK;
    }
}

bool same_params(const bpmd::DeflateStep& a, const bpmd::DeflateStep& b)
{
    return a.level == b.level && a.wbits == b.wbits && a.strategy == b.strategy && !a.tune == !b.tune &&
           (!a.tune || std::memcmp(a.tune, b.tune, 4 * sizeof(int)) == 0) && !a.hist_len == !b.hist_len;
}

void deflate_exec(Arena& A, std::vector<DeflateJob*>& jobs)
{
    std::vector<bool> used(jobs.size(), false);
    for (size_t i = 0; i < jobs.size(); ++i) {
        if (used[i]) continue;
        std::vector<DeflateJob*> g{jobs[i]};
        for (size_t j = i + 1; j < jobs.size(); ++j)
            if (!used[j] && same_params(*jobs[i]->st, *jobs[j]->st)) {
                used[j] = true;
                g.push_back(jobs[j]);
            }
        g_bstat[3].fetch_add(1);
        deflate_group(A, g);   // (a group of one too, as inflate_exec)
    }
}

// The call through its device's coalescer.  False with the batcher off (or
// without a coalescer): the caller runs it alone, on the stream's own arena.
template <class J, class Exec>
bool batched(J& j, int stat, Exec&& exec)
{
    const int mx = batch_max();
    if (mx < 2) return false;
    g_bstat[stat].fetch_add(1);
    int dev = 0;
    Coalescer<J>* c = hipGetDevice(&dev) == hipSuccess ? coalescer<J>(dev) : nullptr;
    if (!c) return false;
    c->run(&j, mx, exec);
    return true;
}

// the reader's device step (inflate_reader.h): the pending reset, then the
// call through the coalescer, or as a batch of one
int run_inflate(void* stream, bpmd::InflateStep& st)
{
    bpmd_stream* s = (bpmd_stream*)stream;
    int r = bpmd_init();
    if (r || (r = ensure_zhead(s, st)) != 0) return r;
    InflateJob j;
    j.s = s;
    j.st = &st;
    if (batched(j, 0, inflate_exec)) return j.rc;
    std::vector<InflateJob*> one{&j};
    inflate_batch(s->arena, one);
    return j.rc;
}

// the writer's device step (deflate_writer.h): through the coalescer, or as a
// group of one
int run_flush(void* stream, bpmd::DeflateStep& st)
{
    bpmd_stream* s = (bpmd_stream*)stream;
    DeflateJob j;
    j.s = s;
    j.st = &st;
    if (batched(j, 2, deflate_exec)) return j.rc;
    const int r = bpmd_init();
    if (r) return r;
    std::vector<DeflateJob*> one{&j};
    deflate_group(s->arena, one);
    return j.rc;
}

}  // namespace

extern "C" int bpmd_stream_batching(int max_calls, int max_delay_us)
{
    if (max_calls < 0 || max_calls > 4096 || max_delay_us < 0) return BPMD_R_INVALID_ARGUMENT;
    (void)batch_max();   // the environment's defaults read first, then replaced
    g_bdelay.store(max_delay_us);
    g_bmax.store(max_calls);
    return BPMD_R_OK;
}

extern "C" int bpmd_stream_batching_get(int* max_calls, int* max_delay_us)
{
    const int m = batch_max();   // the environment's defaults, unless replaced
    if (max_calls) *max_calls = m;
    if (max_delay_us) *max_delay_us = g_bdelay.load();
    return BPMD_R_OK;
}

extern "C" int bpmd_stream_batch_stats(unsigned long long* out, int reset)
{
    if (!out) return BPMD_R_INVALID_ARGUMENT;
    for (int i = 0; i < 4; ++i) out[i] = reset ? g_bstat[i].exchange(0) : g_bstat[i].load();
    return BPMD_R_OK;
}

extern "C" int bpmd_inflate_stream_footprint(const bpmd_stream* s, size_t* host_bytes, size_t* device_bytes)
{
    if (!s || s->is_deflate) return BPMD_R_INVALID_ARGUMENT;
    // the state, and with the batcher off the stream's block and its pinned mirror
    if (device_bytes) *device_bytes = (s->zst ? sizeof(State) + sizeof(Result) : 0) + s->arena.cap;
    if (host_bytes) *host_bytes = s->arena.cap;
    return BPMD_R_OK;
}

extern "C" void bpmd_stream_destroy(bpmd_stream* s)
{
    if (!s) return;
    const Arena& A = s->arena;
    if (A.hs) (void)hipStreamSynchronize(A.hs);
    for (void* p : {(void*)A.d, s->zst})
        if (p) (void)hipFree(p);
    if (A.h) (void)hipHostFree(A.h);
    if (A.hs) {
        bpmd_internal_scratch_release(A.hs);
        (void)hipStreamDestroy(A.hs);
    }
    delete s;
}
