"""Exact-mode deflate's rules (beast_amd/csrc/exact_plan.h) on the CPU: the
tiers, the queue's early exit against the order's keys, where each tier's
arrays lie in LDS and in the per-wave workspace, and the deflater itself
(deflate_exact_core.h, through tests/cpp/exact_host_backend.cpp) in heap blocks
of exactly each tier's sizes against the oracle, at both tier edges and in the
queue's 64-byte band.  tests/cpp/exact_plan_main.cpp runs a wider grid of the
same under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import pytest

from beast_amd import synth
from oracle import oracle as O
from tests.model import exact_host as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beast_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
NONE = 0xFFFFFFFF
T0_MAX, T1_MAX, LDS_HBITS, SHIFT, T2_LDS_HEAD = 4096, 7930, 12, 6, 2048
WBITS, MEMS = range(9, 16), range(1, 10)


@pytest.fixture(scope="module")
def plan():
    L = X.lib()
    u32, u64, ci = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    u8p, u32p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(u32), ctypes.POINTER(u64)
    L.xp_tier_of.argtypes, L.xp_tier_of.restype = [u32, u32], ci
    L.xp_tables.argtypes, L.xp_tables.restype = [u32, u32, u8p, u8p], None
    L.xp_constants.argtypes, L.xp_constants.restype = [u32p], None
    L.xp_cfg.argtypes, L.xp_cfg.restype = [ci, ci, ci, ci, u32p], None
    L.xp_lds.argtypes, L.xp_lds.restype = [u32, ci, u32, u32, u32, u32p], None
    L.xp_ws.argtypes, L.xp_ws.restype = [u64, u32, u32, u32, u64p], None
    L.xp_t2_grid.argtypes, L.xp_t2_grid.restype = [u32, u32], u32
    L.xp_t2_waves.argtypes, L.xp_t2_waves.restype = [u32], u32
    return L


def _constants(plan):
    o = (ctypes.c_uint32 * 12)()
    plan.xp_constants(o)
    return list(o)


def _tier_of(n, hbits):
    """the rule, restated"""
    return 2 if hbits > LDS_HBITS else 0 if n <= T0_MAX else 1 if n <= T1_MAX else 2


def test_header_needs_no_hip():
    """exact_plan.h compiles with plain g++, warnings on, and includes nothing of HIP or of the library."""
    header = os.path.join(CSRC, "exact_plan.h")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include",
                        header, os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    deps = subprocess.run(["g++", "-std=c++17", "-MM", "-x", "c++", header], capture_output=True, text=True, check=True)
    names = {os.path.basename(p) for p in deps.stdout.replace("\\\n", " ").split()}
    assert "pmd_internal.h" not in names and "pmd_common.h" not in names, names
    assert not [n for n in names if n.startswith("hip")], names


def test_constants_and_cfg(plan):
    c = _constants(plan)
    assert c[:6] == [T0_MAX, 4096 + 512, 4096, T1_MAX, 8192 + 512, 8192]
    assert c[6:11] == [SHIFT, T2_LDS_HEAD, 4, 16, LDS_HBITS]
    for t in (0, 1):
        mx, win, prv = c[3 * t:3 * t + 3]
        assert win >= mx + 258 and prv >= mx and win % 16 == 0 and (2 * prv) % 16 == 0
    o = (ctypes.c_uint32 * 5)()
    for mem in MEMS:
        plan.xp_cfg(6, 12, mem, 3, o)
        assert list(o) == [mem + 7, 1 << (mem + 6), 12, 6, 3]
    for cus, n in [(256, 1), (256, 4095), (256, 4096), (256, 4097), (1, 0), (304, 1 << 20)]:
        assert plan.xp_t2_waves(cus) == 16 * cus and plan.xp_t2_grid(cus, n) == min(16 * cus, n)


def test_tier_of(plan):
    for hbits in range(8, 17):
        for n in range(9001):
            assert plan.xp_tier_of(n, hbits) == _tier_of(n, hbits), (n, hbits)


def test_queue_rule(plan):
    """The workspace tier's waves draw messages in the order of the keys len >> 6, longest first.  Where a
    drawn length ends the queue, no length of its key or a smaller one is a workspace message; and a
    workspace message never ends it."""
    N = 70001
    top = N + (1 << SHIFT)
    tiers, done = (ctypes.c_uint8 * top)(), (ctypes.c_uint8 * top)()
    for hbits in range(8, 17):
        plan.xp_tables(hbits, top, tiers, done)
        tier = bytes(tiers)
        assert all(tier[n] == _tier_of(n, hbits) for n in (0, T0_MAX, T0_MAX + 1, T1_MAX, T1_MAX + 1, N))
        longest2 = [0] * (top >> SHIFT)   # per key: is any length of a key up to this one tier 2?
        seen = False
        for k in range(top >> SHIFT):
            seen = seen or 2 in tier[k << SHIFT:(k + 1) << SHIFT]
            longest2[k] = seen
        ends = 0
        for n in range(N):
            if done[n]:
                assert not longest2[n >> SHIFT], (n, hbits)
                assert tier[n] != 2
                ends += 1
            # the exit is not lost either: a key whose lengths are all below the band ends the queue
            elif hbits <= LDS_HBITS:
                assert n + (1 << SHIFT) > T1_MAX
        assert ends == (T1_MAX - (1 << SHIFT) + 1 if hbits <= LDS_HBITS else 0)


def _ordered(regions, end):
    at = 0
    for off, size in regions:
        assert off % 16 == 0 and off >= at, (regions, end)
        at = off + size
    assert end >= at, (regions, end)


def test_layouts(plan):
    trees = _constants(plan)[11]
    assert 4000 < trees < 5000
    lds, ws = (ctypes.c_uint32 * 6)(), (ctypes.c_uint64 * 6)()
    n = 0
    for wbits in WBITS:
        for mem in MEMS:
            hbits, lit, w, h = mem + 7, 1 << (mem + 6), 1 << wbits, 1 << (mem + 7)
            for t in (0, 1, 2):
                if t < 2 and hbits > LDS_HBITS:
                    continue   # no message reaches an LDS tier
                plan.xp_lds(trees, t, wbits, hbits, lit, lds)
                win, prv, hd, syms, size, prv_n = lds
                assert size <= 65536, (t, wbits, mem)
                if t < 2:
                    mx, wn, pv = _constants(plan)[3 * t:3 * t + 3]
                    assert prv_n == min(w, pv)
                    _ordered([(0, trees), (win, wn), (prv, 2 * pv), (hd, 2 * h), (syms, 3 * lit)], size)
                    # what the deflater touches fits: the physical window and its slack, or the longest
                    # message and the zeroed bytes behind it when no slide can begin
                    assert prv - win == wn
                    if 2 * w + 258 + 64 <= wn:
                        assert prv_n == w
                    else:
                        assert mx + 262 < 2 * w and wn >= mx + 258 and prv_n >= mx
                else:
                    assert (win, prv, syms) == (NONE, NONE, NONE) and prv_n == w
                    if h <= T2_LDS_HEAD:
                        assert hd == (trees + 15) // 16 * 16 and size == hd + 2 * h
                    else:
                        assert hd == NONE and size == (trees + 15) // 16 * 16
                    for base in (0, 1 << 40):
                        plan.xp_ws(base, wbits, hbits, lit, ws)
                        wwin, wprv, whd, wsyms, wend, per = ws
                        assert wwin == base
                        _ordered([(wwin - base, 2 * w + 258 + 64), (wprv - base, 2 * w), (whd - base, 2 * h),
                                  (wsyms - base, 3 * lit)], wend - base)
                        assert per >= wend - base and per % 16 == 0
                n += 1
    assert n == 7 * (5 * 3 + 4)


def _msgs(sizes):
    out = []
    for k in ("json", "binary"):
        for s in sizes:
            d, _, _ = synth.make_batch(k, [s], seed=0xE7AC7 + 7 * s)
            out.append(bytes(d[:s]))
    return out


EDGES = (4095, 4096, 4097, 7866, 7867, 7929, 7930, 7931, 7994)


@pytest.fixture(scope="module")
def edge_msgs():
    return _msgs(EDGES)


@pytest.mark.parametrize("wbits", [9, 11, 12, 13, 15])   # 11 and 12 slide inside an LDS tier, 13 and up cannot
@pytest.mark.parametrize("mem", [1, 4, 5])
def test_tier_sized_runs_match_the_oracle(edge_msgs, plan, wbits, mem):
    tiers = set()
    for level in (0, 1, 6, 9):
        for m in edge_msgs:
            want = O.pmd_deflate(m, level, wbits, mem, 0)
            t = plan.xp_tier_of(len(m), mem + 7)
            tiers.add(t)
            assert X.deflate(m, level, wbits, mem, tier=t) == (0, want), (len(m), level, wbits, mem, t)
            assert X.deflate(m, level, wbits, mem, tier=2) == (0, want), (len(m), level, wbits, mem)
    assert tiers == {0, 1, 2}


def test_sanitized_run_at_tier_sizes():
    """tests/cpp/exact_plan_main.cpp under -fsanitize=address,undefined, with clang++ (the core uses
    __builtin_bitreverse32)"""
    build = os.path.join(CPP, "_build")
    os.makedirs(build, exist_ok=True)
    src, out = os.path.join(CPP, "exact_plan_main.cpp"), os.path.join(build, "exact_plan_main")
    deps = [src] + X.DEPS
    if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, deps)):
        subprocess.run([X.CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "3024 cases" in r.stdout and " 0 failures" in r.stdout
