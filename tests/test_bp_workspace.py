"""The block-parallel inflate's workspace-capacity policy
(beast_amd/csrc/bp_workspace.h), checked on the CPU: the header compiles with
plain g++ and each rule is compared with values worked out by hand from the
driver's arithmetic (pmd_inflate_bp.hip): growth by a quarter, the 2^32 - 1
task clamp, half of free memory as the budget, halving after a failed
allocation down to none, and the ceiling that holds for 8 to 1024 calls.

A capacity is (tasks, words, ceiling tasks, ceiling words, hold, backoff).
"""
import ctypes
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "beast_amd", "csrc")

SHIM = r"""
#include "bp_workspace.h"
using namespace bpmd::bp;
typedef unsigned long long u64;
static Capacity load(const u64* v)
{
    Capacity c;
    c.tasks = v[0], c.words = v[1], c.ceil_tasks = v[2], c.ceil_words = v[3];
    c.hold = (uint32_t)v[4], c.backoff = (uint32_t)v[5];
    return c;
}
static void store(const Capacity& c, u64* v)
{
    v[0] = c.tasks, v[1] = c.words, v[2] = c.ceil_tasks, v[3] = c.ceil_words, v[4] = c.hold, v[5] = c.backoff;
}
extern "C" void fresh(u64* v) { store(Capacity(), v); }
extern "C" int fresh_sized() { return Capacity().sized; }
extern "C" u64 free_unknown() { return FREE_UNKNOWN; }
extern "C" int wants_free(const u64* v, u64 t, u64 w) { return grows(load(v), {t, w}); }
extern "C" void grow(u64* v, u64 t, u64 w, u64 free_bytes)
{
    Capacity c = load(v);
    grow_to(c, {t, w}, free_bytes);
    store(c, v);
}
extern "C" void begin(u64* v)
{
    Capacity c = load(v);
    begin_call(c);
    store(c, v);
}
extern "C" void failed(u64* v, u64 t, u64 w, u64* next)
{
    Capacity c = load(v);
    const Need x = alloc_failed(c, {t, w});
    store(c, v);
    next[0] = x.tasks, next[1] = x.words;
}
extern "C" int retry(u64* tried)
{
    Need x = {tried[0], tried[1]};
    const bool more = alloc_retry(x);
    tried[0] = x.tasks, tried[1] = x.words;
    return more;
}
extern "C" void settled(u64* v, u64 t, u64 w)
{
    Capacity c = load(v);
    alloc_settled(c, {t, w});
    store(c, v);
}
extern "C" void reserve(u64 in_bytes, u64 out_bytes, u64 msgs, u64* out)
{
    const Need x = reserve_need(in_bytes, out_bytes, msgs);
    out[0] = x.tasks, out[1] = x.words;
}
extern "C" void layout(u64 t, u64 w, uint32_t n, u64* out)
{
    const DwLayout D({t, w}, n);
    const u64 v[7] = {D.tasks, D.res, D.fb, D.map, D.mark, D.sym, D.bytes};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
    if (dw_bytes({t, w}, n) != D.bytes) out[6] = 0;
}
extern "C" void sizes(u64* out) { out[0] = sizeof(SegTask), out[1] = sizeof(SegRes), out[2] = SYM_GUARD; }
"""

U64 = ctypes.c_ulonglong
PER_TASK = 32 + 16 + 4   # a task, its result, its region-map word
MIB = 1 << 20


class Ws:
    def __init__(self, lib):
        self.lib = lib
        lib.free_unknown.restype = U64
        self.unknown = lib.free_unknown()

    def cap(self, tasks=0, words=0, ceil_tasks=0, ceil_words=0, hold=0, backoff=8):
        return (U64 * 6)(tasks, words, ceil_tasks, ceil_words, hold, backoff)

    def grow(self, c, t, w, free=None):
        self.lib.grow(c, U64(t), U64(w), U64(self.unknown if free is None else free))
        return tuple(c)[:2]

    def wants_free(self, c, t, w):
        return bool(self.lib.wants_free(c, U64(t), U64(w)))

    def failed(self, c, t, w):
        nxt = (U64 * 2)()
        self.lib.failed(c, U64(t), U64(w), nxt)
        return tuple(nxt)

    def retry(self, tried):
        x = (U64 * 2)(*tried)
        more = bool(self.lib.retry(x))
        return more, tuple(x)

    def layout(self, t, w, n):
        out = (U64 * 7)()
        self.lib.layout(U64(t), U64(w), n, out)
        return tuple(out)


@pytest.fixture(scope="module")
def ws(tmp_path_factory):
    d = tmp_path_factory.mktemp("bp_workspace")
    src, lib = d / "shim.cpp", d / "libbpws.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC, str(src), "-o",
                    str(lib)], check=True)
    return Ws(ctypes.CDLL(str(lib)))


def test_record_sizes_and_fresh_capacity(ws):
    out = (U64 * 3)()
    ws.lib.sizes(out)
    assert tuple(out) == (32, 16, 64)
    c = ws.cap(1, 1, 1, 1, 1, 1)
    ws.lib.fresh(c)
    assert tuple(c) == (0, 0, 0, 0, 0, 8)
    assert ws.lib.fresh_sized() == 0


def test_growth_by_a_quarter(ws):
    c = ws.cap()
    assert ws.grow(c, 1000, 100000) == (1250, 125000)
    # from a larger capacity: only what is exceeded moves, nothing shrinks
    c = ws.cap(2000, 50000)
    assert ws.grow(c, 1000, 100000) == (2000, 125000)
    assert ws.grow(c, 2001, 3) == (2501, 125000)
    assert ws.grow(c, 2501, 125000) == (2501, 125000)
    assert ws.grow(c, 0, 0) == (2501, 125000)
    assert tuple(c)[2:] == (0, 0, 0, 8)


def test_task_clamp(ws):
    c = ws.cap()
    assert ws.grow(c, 4_000_000_000, 8) == (0xFFFFFFFF, 10)
    assert ws.grow(c, 1 << 40, 8) == (0xFFFFFFFF, 10)
    # at the clamp a larger want moves nothing: the free memory is not asked for
    assert not ws.wants_free(c, 1 << 40, 8)
    assert not ws.wants_free(c, 1 << 40, 10)
    assert ws.wants_free(c, 1 << 40, 11)


def test_budget_is_half_of_free_memory(ws):
    budget = MIB // 2
    # tasks over the budget: as many as fit, and the words that remain
    c = ws.cap()
    nt = budget // PER_TASK
    assert nt == 10082 and (budget - nt * PER_TASK) // 2 == 12
    assert ws.grow(c, 20000, 1000, free=MIB) == (10082, 12)
    # tasks fit, words over: 1250 tasks take 65 000 bytes, the words the rest
    c = ws.cap()
    assert ws.grow(c, 1000, 400000, free=MIB) == (1250, (budget - 65000) // 2) == (1250, 229644)
    # the last want that fits (65 000 + 2 x 229 643 = 524 286 bytes) and the first that does not
    c = ws.cap()
    assert ws.grow(c, 1000, 183715, free=MIB) == (1250, 183715 + 45928) == (1250, 229643)
    c = ws.cap()
    assert ws.grow(c, 1000, 183716, free=MIB) == (1250, 229644)
    # both fit
    c = ws.cap()
    assert ws.grow(c, 1000, 100000, free=MIB) == (1250, 125000)
    # a budget below the present capacity never shrinks it
    c = ws.cap(5000, 300000)
    assert ws.grow(c, 20000, 100, free=MIB) == (10082, 300000)
    assert ws.grow(c, 20000, 400000, free=0) == (10082, 300000)
    # nothing to grow: the free memory plays no part
    assert not ws.wants_free(c, 10082, 300000)
    assert ws.wants_free(c, 10083, 0) and ws.wants_free(c, 0, 300001)
    assert ws.grow(c, 100, 100, free=0) == (10082, 300000)


def test_halving_down_to_none(ws):
    c = ws.cap(4096, 1 << 20)
    assert ws.failed(c, 4096, 1 << 20) == (2048, 1 << 19)
    assert tuple(c)[:2] == (2048, 1 << 19)
    tried, seen = (2048, 1 << 19), []
    while True:
        more, tried = ws.retry(tried)
        if not more:
            break
        seen.append(tried)
    # 2^16 words are still tried; below that, none -- and none is the last
    assert seen == [(1024, 1 << 18), (512, 1 << 17), (256, 1 << 16), (0, 0)]
    assert tried == (0, 0)
    # the retries are the call's own: the stream's capacity waits for the outcome
    assert tuple(c)[:2] == (2048, 1 << 19)
    # the first halving only where the capacity is still the one that failed
    c = ws.cap(4096, 1 << 20)
    assert ws.failed(c, 1000, 1 << 20) == (4096, 1 << 19)
    c = ws.cap(4096, 1 << 20)
    assert ws.failed(c, 4096, 5) == (2048, 1 << 20)
    c = ws.cap(4096, 1 << 20)
    assert ws.failed(c, 7, 5) == (4096, 1 << 20)
    # the floor applies to the first retry too
    c = ws.cap(100, 100000)
    assert ws.failed(c, 100, 100000) == (0, 0)
    assert tuple(c)[:2] == (50, 50000)
    c = ws.cap(0, 0)
    assert ws.failed(c, 0, 0) == (0, 0)
    assert ws.retry((0, 0)) == (False, (0, 0))


def test_ceiling_holds_and_backs_off(ws):
    c = ws.cap(4096, 1 << 20)
    ws.lib.settled(c, U64(256), U64(1 << 16))
    assert tuple(c) == (256, 1 << 16, 256, 1 << 16, 8, 16)
    # while it holds, the ceiling caps growth, and each call counts it down
    for left in range(7, -1, -1):
        assert ws.grow(c, 10000, 1_000_000) == (256, 1 << 16)
        ws.lib.begin(c)
        assert tuple(c)[4] == left
    assert ws.grow(c, 10000, 1_000_000) == (12500, 1_250_000)
    ws.lib.begin(c)
    assert tuple(c)[4:] == (0, 16)
    # the budget and the ceiling together: the smaller wins
    c = ws.cap(10, 10, 20000, 100, 3, 8)
    assert ws.grow(c, 20000, 1000, free=MIB) == (10082, 12)
    c = ws.cap(10, 10, 5000, 100, 3, 8)
    assert ws.grow(c, 20000, 1000, free=None) == (5000, 100)
    # every failure doubles the hold, up to 1024, and there it stays
    c = ws.cap()
    holds = []
    for _ in range(10):
        ws.lib.settled(c, U64(1), U64(1 << 16))
        holds.append(tuple(c)[4:])
    assert holds == [(8, 16), (16, 32), (32, 64), (64, 128), (128, 256), (256, 512), (512, 1024), (1024, 1024),
                     (1024, 1024), (1024, 1024)]


def test_reserve_bounds_c5(ws):
    # C5: 16 Ki payloads of 64 KiB, 1.013 x that compressed (66 388 bytes)
    msgs, out_bytes, in_bytes = 16384, 16384 * 65536, 16384 * 66388
    out = (U64 * 2)()
    ws.lib.reserve(U64(in_bytes), U64(out_bytes), U64(msgs), out)
    # tasks: a region per KiB of input and one more per payload; words: 3.75 per
    # output byte, 15 + 512 per task, 64 + 64 per payload
    assert tuple(out) == (1_062_208 + 16384, 4_026_531_840 + 527 * 1_078_592 + 128 * 16384)
    assert tuple(out) == (1_078_592, 4_597_046_976)
    ws.lib.reserve(U64(0), U64(0), U64(0), out)
    assert tuple(out) == (0, 0)
    ws.lib.reserve(U64(1023), U64(4), U64(1), out)
    assert tuple(out) == (1, 15 + 527 + 128)


def test_layout_is_aligned_and_monotonic(ws):
    # by hand: 3 tasks, 1000 words, 5 messages
    assert ws.layout(3, 1000, 5) == (0, 256, 512, 768, 1024, 1280, 1280 + 2304)
    assert ws.layout(0, 0, 1) == (0, 0, 0, 256, 256, 512, 768)
    prev = None
    for t, w, n in [(0, 0, 1), (1, 0, 1), (1, 1, 1), (1, 1, 64), (9, 1, 65), (9, 130, 65), (1000, 70000, 2048),
                    (1001, 70000, 2048), (1001, 70001, 2049), (1 << 20, 1 << 32, 16384), (0xFFFFFFFF, 1 << 40, 1 << 20)]:
        lay = ws.layout(t, w, n)
        assert all(x % 256 == 0 for x in lay), lay
        assert list(lay) == sorted(lay)
        # the symbol area keeps its guard and the 64 symbols of tail
        assert lay[6] - lay[5] >= 2 * (w + 64 + 64)
        assert lay[1] >= 32 * t and lay[2] - lay[1] >= 16 * t and lay[4] - lay[3] >= 4 * t
        assert lay[3] - lay[2] >= 4 * n and lay[5] - lay[4] >= 4 * n
        if prev is not None:
            assert lay[6] >= prev
        prev = lay[6]
    # growing any one of the three never shrinks the block
    for t, w, n in [(5, 5, 5), (64, 1000, 63), (4096, 1 << 20, 2048)]:
        b = ws.layout(t, w, n)[6]
        assert ws.layout(t + 1, w, n)[6] >= b and ws.layout(t, w + 1, n)[6] >= b and ws.layout(t, w, n + 1)[6] >= b
