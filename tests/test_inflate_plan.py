"""The inflate kernel choice (beast_amd/csrc/inflate_plan.h plan_inflate),
checked on the CPU: the header compiles with plain g++ and the plan for each
(mode, takeover window, masking key, batch size, knobs) is compared with the
decision table below, written out by hand from pmd_capi.hip's policy.

A plan is (lanes, max_in, queue, order, long, (lanes, min_thr, share_pct) of
bpmd_internal_lane_long_split, wave, min_in).
"""
import ctypes
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "beast_amd", "csrc")

SHIM = r"""
#include "inflate_plan.h"
extern "C" void plan(int mode, uint32_t n, int hist, int key, uint32_t wgs, int bp, uint32_t split, int ordered,
                     int long_split, uint32_t share_pct, uint32_t* out)
{
    bpmd::InflateKnobs k;
    k.bp = bp;
    k.split = split;
    k.ordered = ordered;
    k.long_split = long_split;
    k.share_pct = share_pct;
    const bpmd::InflatePlan p = bpmd::plan_inflate(mode, n, hist, key, wgs, k);
    const uint32_t v[10] = {(uint32_t)p.lanes, p.max_in, p.queue, p.order, (uint32_t)p.longs, p.split_lanes,
                            p.split_min_thr, p.split_share_pct, (uint32_t)p.wave, p.min_in};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
}
extern "C" void defaults(uint32_t* out)
{
    const bpmd::InflateKnobs k;
    out[0] = k.bp, out[1] = k.split, out[2] = k.ordered, out[3] = k.long_split, out[4] = k.share_pct;
}
"""

AUTO, LANE, WAVE, BP = 0, 1, 2, 3
# InflatePlan::Lanes / Longs / Wave
L_NONE, L_ALL, L_UP_TO = 0, 1, 2
G_NONE, G_BP_INLINE, G_BP_SIDE, G_WAVE_ORDERED = 0, 1, 2, 3
W_NONE, W_ALL, W_OVER = 0, 1, 2

WGS = 1024          # 4 workgroups on each of 256 CUs
Q = WGS * 64        # messages the chip's lanes hold
NO3 = (0, 0, 0)


def wave_only():
    return (L_NONE, 0, False, False, G_NONE, NO3, W_ALL, 0)


def lanes_plain():
    return (L_ALL, 0, False, False, G_NONE, NO3, W_NONE, 0)


def lanes_queue(order=True, long=G_NONE, args=NO3):
    return (L_ALL, 0, True, order, long, args, W_NONE, 0)


def lanes_bp_inline(min_thr):
    return (L_ALL, 0, False, True, G_BP_INLINE, (0, min_thr, 0), W_NONE, 0)


def lanes_wave_split(split):
    return (L_UP_TO, split, False, False, G_NONE, NO3, W_OVER, split)


def load_plan(d):
    """Compile the shim over inflate_plan.h into directory `d` (a pathlib
    path) and return the plan function; tests/test_read_keyed_cases.py and
    tests/test_gpu_read_keyed.py ask it which branch their batches take."""
    src, lib = d / "shim.cpp", d / "libplan.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC, str(src), "-o",
                    str(lib)], check=True)
    L = ctypes.CDLL(str(lib))

    def call(mode, n, hist=False, key=False, wgs=WGS, bp=True, split=4096, ordered=True, long_split=True, share=125):
        out = (ctypes.c_uint32 * 10)()
        L.plan(mode, n, int(hist), int(key), wgs, int(bp), split, int(ordered), int(long_split), share, out)
        v = list(out)
        return (v[0], v[1], bool(v[2]), bool(v[3]), v[4], tuple(v[5:8]), v[8], v[9])

    call.lib = L
    return call


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return load_plan(tmp_path_factory.mktemp("inflate_plan"))


def test_knob_defaults(plan):
    out = (ctypes.c_uint32 * 5)()
    plan.lib.defaults(out)
    assert list(out) == [1, 4096, 1, 1, 125]


@pytest.mark.parametrize("n", [1, 2047, 2048, 32768, Q, Q + 1])
def test_forced_bp(plan, n):
    # every payload of 64 bytes or more block-parallel on the caller's stream, the rest on lanes
    assert plan(BP, n) == lanes_bp_inline(64)
    assert plan(BP, n, bp=False) == lanes_bp_inline(64)
    # the segment decoder starts mid-payload: not with a masking key
    assert plan(BP, n, key=True) == wave_only()


@pytest.mark.parametrize("n", [1, 2048, 32768, Q + 1])
@pytest.mark.parametrize("key", [False, True])
def test_forced_wave(plan, n, key):
    assert plan(WAVE, n, key=key) == wave_only()


@pytest.mark.parametrize("key", [False, True])
def test_forced_lane(plan, key):
    for n in (1, 2047, 2048, 32768, Q):
        assert plan(LANE, n, key=key) == lanes_plain()
    assert plan(LANE, Q + 1, key=key) == lanes_queue()


@pytest.mark.parametrize("mode", [AUTO, LANE, WAVE, BP])
def test_takeover_window_always_lanes(plan, mode):
    # only the lane kernel reads a window
    for n in (1, 2047, 2048, 32767, 32768, Q):
        assert plan(mode, n, hist=True) == lanes_plain()
    assert plan(mode, Q + 1, hist=True) == lanes_queue()
    assert plan(mode, Q + 1, hist=True, ordered=False) == lanes_queue(order=False)


@pytest.mark.parametrize("key", [False, True])
@pytest.mark.parametrize("bp", [False, True])
def test_auto_small_batches_use_waves(plan, key, bp):
    assert plan(AUTO, 1, key=key, bp=bp) == wave_only()
    assert plan(AUTO, 2047, key=key, bp=bp) == wave_only()
    assert plan(AUTO, 2048, key=key, bp=bp) != wave_only()


@pytest.mark.parametrize("n", [2048, 32767])
def test_auto_mid_batches_split(plan, n):
    assert plan(AUTO, n) == lanes_bp_inline(4096)
    assert plan(AUTO, n, key=True) == lanes_wave_split(4096)
    assert plan(AUTO, n, bp=False) == lanes_wave_split(4096)
    # BPMD_INFLATE_SPLIT moves the split; 0 leaves everything to the lanes
    assert plan(AUTO, n, split=1024) == lanes_bp_inline(1024)
    assert plan(AUTO, n, key=True, split=1024) == lanes_wave_split(1024)
    assert plan(AUTO, n, split=0) == lanes_plain()
    # the queue knobs do not reach these rows
    assert plan(AUTO, n, ordered=False, long_split=False) == lanes_bp_inline(4096)


@pytest.mark.parametrize("key", [False, True])
@pytest.mark.parametrize("bp", [False, True])
def test_auto_large_batches_that_fit_the_lanes(plan, key, bp):
    assert plan(AUTO, 32768, key=key, bp=bp) == lanes_plain()
    assert plan(AUTO, Q, key=key, bp=bp) == lanes_plain()


def test_auto_work_queue(plan):
    n = Q + 1
    assert plan(AUTO, n) == lanes_queue(long=G_BP_SIDE, args=(Q, 2048, 125))
    assert plan(AUTO, n, share=150) == lanes_queue(long=G_BP_SIDE, args=(Q, 2048, 150))
    wave_ordered = lanes_queue(long=G_WAVE_ORDERED, args=(Q, 4096, 200))
    assert plan(AUTO, n, key=True) == wave_ordered
    assert plan(AUTO, n, bp=False) == wave_ordered
    assert plan(AUTO, n, key=True, share=150) == wave_ordered
    # the split plays no part from 32 Ki messages on
    assert plan(AUTO, n, split=1024) == lanes_queue(long=G_BP_SIDE, args=(Q, 2048, 125))


@pytest.mark.parametrize("key", [False, True])
def test_auto_work_queue_knobs(plan, key):
    n = Q + 1
    # BPMD_INFLATE_ORDER=0: the queue alone, in batch order
    assert plan(AUTO, n, key=key, ordered=False) == lanes_queue(order=False)
    assert plan(AUTO, n, key=key, ordered=False, long_split=False) == lanes_queue(order=False)
    # BPMD_INFLATE_LONG=0: longest first, the long payloads stay on lanes
    assert plan(AUTO, n, key=key, long_split=False) == lanes_queue()


def test_small_grid(plan):
    # BPMD_QUEUE_WGS=8: the lanes hold 512 messages
    w, q = 8, 512
    assert plan(LANE, q, wgs=w) == lanes_plain()
    assert plan(LANE, q + 1, wgs=w) == lanes_queue()
    assert plan(AUTO, q + 1, wgs=w) == wave_only()
    # a split keeps batches below 32 Ki messages off the queue
    for n in (2048, 32767):
        assert plan(AUTO, n, wgs=w) == lanes_bp_inline(4096)
        assert plan(AUTO, n, wgs=w, key=True) == lanes_wave_split(4096)
        assert plan(AUTO, n, wgs=w, split=0) == lanes_queue(long=G_BP_SIDE, args=(q, 2048, 125))
    assert plan(AUTO, 32768, wgs=w) == lanes_queue(long=G_BP_SIDE, args=(q, 2048, 125))
    assert plan(AUTO, 32768, wgs=w, key=True) == lanes_queue(long=G_WAVE_ORDERED, args=(q, 4096, 200))
    assert plan(AUTO, 32768, wgs=w, bp=False) == lanes_queue(long=G_WAVE_ORDERED, args=(q, 4096, 200))
