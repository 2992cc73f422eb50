"""The per-stream deflater's call protocol (beast_amd/csrc/deflate_writer.h)
on the CPU: tests/cpp/deflate_writer_backend.cpp exports the
bpmd_deflate_stream_* ABI over that header alone, built with plain g++, with a
stand-in for the device step that emits stored blocks and an empty static
block (so every flush ends inside a byte) and records what each compress call
was given.  The scripts and checks of tests/deflate_scripts.py run against it
beside the oracle backend: A (call parity), B (decodability), C (framing), D
(restart after full) and E (small rooms, strict).  What the checks that
measure the compressor would show on a device -- the history in use, tune()
in force -- is asserted from the stand-in's record instead."""
import collections
import ctypes
import functools
import os
import subprocess

import pytest

from tests import deflate_scripts as S
from tests.test_facade import BUILD, CPP, ROOT

CSRC = os.path.join(ROOT, "beast_amd", "csrc")
LEVELS, WBITS = (0, 1, 6, 9), (9, 15)
LOW = S.LEVEL_ROWS[1]

Call = collections.namedtuple("Call", "level strategy tune hist n")


@functools.lru_cache(maxsize=None)
def _library():
    os.makedirs(BUILD, exist_ok=True)
    lib = os.path.join(BUILD, "libbpmd_writer_backend.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-shared", "-fPIC", "-o", lib,
                    os.path.join(CPP, "deflate_writer_backend.cpp")], check=True)
    L = S.bind(ctypes.CDLL(lib))
    L.dwb_calls.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.c_size_t]
    L.dwb_calls.restype = ctypes.c_size_t
    L.dwb_hist_keep.restype = ctypes.c_size_t
    return L


class Backend:
    """The backend library as S.run() drives it; `calls` is the record of
    the last run's compress calls, read as run() destroys the stream."""

    def __init__(self):
        self._L = _library()
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._L, name)

    def bpmd_stream_destroy(self, h):
        n = self._L.dwb_calls(h, None, 0)
        rec = (ctypes.c_longlong * (9 * n))()
        assert self._L.dwb_calls(h, rec, n) == n
        rows = [rec[9 * i:9 * i + 9] for i in range(n)]
        self.calls = [Call(r[0], r[1], tuple(r[3:7]) if r[2] else None, r[7], r[8]) for r in rows]
        self._L.bpmd_stream_destroy(h)


@pytest.fixture
def lib():
    return Backend()


@functools.lru_cache(maxsize=None)
def _ref_cached(script, cfg, room):
    return S.run(S.oracle_backend(), list(script), room=room, **dict(cfg))


def _ref(script, cfg, room=None):
    """The oracle backend's run, computed once per script and configuration."""
    return _ref_cached(tuple(script), tuple(sorted(cfg.items())), room)


def _abc(L, script, cfg):
    steps = S.run(L, script, **cfg)
    ref = _ref(script, cfg)
    S.check_call_parity(steps, ref)
    S.check_decodable(steps, script, cfg["wbits"])
    S.check_framing(steps, ref)
    return steps


def test_header_needs_no_hip():
    """deflate_writer.h compiles with plain g++, warnings on, and includes nothing of HIP."""
    header = os.path.join(CSRC, "deflate_writer.h")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include",
                        header, os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    deps = subprocess.run(["g++", "-std=c++17", "-MM", "-x", "c++", header], capture_output=True, text=True, check=True)
    names = {os.path.basename(p) for p in deps.stdout.replace("\\\n", " ").split()}
    assert "lz_core.h" in names and "pmd_internal.h" not in names, names
    assert not [n for n in names if n.startswith("hip")], names


@pytest.mark.parametrize("wbits", WBITS)
@pytest.mark.parametrize("level", LEVELS)
def test_flush_matrix(lib, level, wbits):
    """A, B, C on each flush kind repeated and on the mixed script, D wherever a Flush::full occurs; every strategy."""
    for strategy in range(5):
        seed = level * 5 + strategy + wbits
        for n, flush in enumerate(("partial", "sync", "full", "trees", "block")):
            _abc(lib, S.repeating(flush, seed + n), S.config(level, wbits, strategy, n))
        S.check_restart(lib, S.repeating("full", seed + 2), S.config(level, wbits, strategy, 2))
        _abc(lib, S.mixed(seed), S.config(level, wbits, strategy, 5))
        _abc(lib, S.full_restart(seed), S.config(level, wbits, strategy))
        S.check_restart(lib, S.full_restart(seed), S.config(level, wbits, strategy))
        S.check_restart(lib, S.mixed(seed), S.config(level, wbits, strategy))


@pytest.mark.parametrize("wbits", WBITS)
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("buffered", (False, True))
def test_params_mid_stream(lib, buffered, level, wbits):
    for seed in range(3):
        script = S.params_script(seed, buffered)
        steps = _abc(lib, script, S.config(level, wbits, 0, seed))
        bad = [s.rc for st, s in zip(script, steps) if st[0] == "params" and not 0 <= st[1] <= 9]
        assert bad == [S.STREAM_ERROR] * 2
        cost = S.level0_cost(steps, script)
        assert cost and all(out >= n for out, n in cost), cost


@pytest.mark.parametrize("wbits", WBITS)
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("kind", sorted(S.PRIMES))
def test_prime(lib, kind, level, wbits):
    for between in (False, True):
        _abc(lib, S.prime_script(kind, level, between), S.config(level, wbits, 0))


def test_prime_only_pending(lib):
    steps = S.run(lib, S.prime_only())
    S.check_call_parity(steps, _ref(S.prime_only(), dict(level=6, wbits=15, mem=8, strategy=0)))
    assert [s.pend for s in steps] == [(0, 5), (2, 2), (4, 2), (4, 2)]


def test_split_pattern(lib):
    cfg = dict(level=6, wbits=15, mem=8, strategy=0)
    for i in range(len(S.HELLO) + 1):
        script = S.split_pattern(S.HELLO, i)
        for j in (1, 2, 3, 5, 8, 13):
            steps = S.run(lib, script, room=("split", j))
            S.check_call_parity(steps, _ref(script, cfg, ("split", j)))
            S.check_decodable(steps, script, 15)
            assert [s.rc for s in steps] == [S.OK if i else S.NEED_BUFFERS, S.OK, S.END_OF_STREAM], (i, j)


@pytest.mark.parametrize("k", (1, 2, 5, 7, 64))
def test_tight_output(lib, k):
    """E, strict.  Two configurations, not the oracle test's four: the writer never reads windowBits and
    reads the level only in params(), which these scripts do not call, and the stand-in's stored blocks
    come out k bytes a call (thousands of calls a script at k = 1)."""
    for level, wbits in ((6, 15), (0, 9)):
        for n, script in enumerate(S.tight_scripts(level + wbits)):
            cfg = S.config(level, wbits, 0, n)
            S.check_tight(S.run(lib, script, room=("tight", k), **cfg), script, wbits, k, strict=True)


# ------------------------------------------------- what the compress calls saw

A, B, C = S.segment("json", 3000, 1), S.segment("corpus1", 700, 2), S.segment("json", 2500, 3)
CFG = dict(level=6, wbits=15, mem=8, strategy=0)


def _calls(lib, script, **cfg):
    steps = S.run(lib, script, **{**CFG, **cfg})
    return steps, lib.calls


@pytest.mark.parametrize("flush", ("sync", "trees", "partial", "block"))
def test_history_kept_across_a_flush(lib, flush):
    """The next compress call sees the last min(total written, keep) bytes."""
    keep = lib.dwb_hist_keep()
    assert len(A) < keep < len(A) + len(B) + len(C)
    _, calls = _calls(lib, [("write", A, flush), ("write", B, flush), ("write", C, flush), ("write", A, "finish")])
    assert [c.hist for c in calls] == [0, len(A), len(A) + len(B), keep]
    assert [c.n for c in calls] == [len(A), len(B), len(C), len(A)]
    big = S.segment("json", 20000, 4)
    _, calls = _calls(lib, [("write", big, flush), ("write", B, "finish")])
    assert [c.hist for c in calls] == [0, keep]


def test_history_dropped_by_full_and_reset(lib):
    _, calls = _calls(lib, [("write", A, "full"), ("write", B, "sync"), ("write", C, "full"), ("write", A, "sync"),
                            ("reset",), ("write", B, "sync"), ("write", C, "finish")])
    assert [c.hist for c in calls] == [0, 0, len(B), 0, 0, len(B)]


def test_tune_before_the_first_write_is_not_seen(lib):
    _, calls = _calls(lib, [("tune",) + LOW, ("write", A, "sync"), ("write", B, "finish")])
    assert [c.tune for c in calls] == [None, None]


def test_tune_on_an_initialised_stream_is_seen(lib):
    _, calls = _calls(lib, [("write", A, "sync"), ("tune",) + LOW, ("write", B, "sync"), ("write", C, "finish")])
    assert [c.tune for c in calls] == [None, LOW, LOW]
    # prime() initialises a fresh stream, an empty flush too
    primes = [("prime", bits, value) for bits, value in S.PRIMES["stored"]]
    for first in (primes, [("write", b"", "sync")]):
        _, calls = _calls(lib, first + [("tune",) + LOW, ("write", A, "finish")])
        assert [c.tune for c in calls] == [LOW]


def test_tune_dropped_by_a_level_change_and_by_reset(lib):
    _, calls = _calls(lib, [("write", A, "sync"), ("tune",) + LOW, ("params", 4, 0), ("write", B, "finish")])
    assert [(c.level, c.tune) for c in calls] == [(6, None), (4, None)]
    _, calls = _calls(lib, [("write", A, "sync"), ("tune",) + LOW, ("reset",), ("write", B, "finish")])
    assert [c.tune for c in calls] == [None, None]


def test_tune_survives_a_change_of_strategy_alone(lib):
    """params() with the level unchanged keeps the tune() values (doParams reloads the table row only
    when the level changes)."""
    _, calls = _calls(lib, [("write", A, "sync"), ("tune",) + LOW, ("params", 6, 3), ("write", B, "finish")])
    assert [(c.level, c.strategy, c.tune) for c in calls] == [(6, 0, None), (6, 3, LOW)]


def test_params_compresses_buffered_input_with_the_old_level(lib):
    steps, calls = _calls(lib, [("write", A, "none"), ("params", 1, 2), ("write", B, "finish")])
    assert [s.rc for s in steps] == [S.OK, S.OK, S.END_OF_STREAM] and steps[1].out
    assert [(c.level, c.strategy, c.n) for c in calls] == [(6, 0, len(A)), (1, 2, len(B))]


def test_params_without_room_leaves_the_input_for_the_new_level(lib):
    steps, calls = _calls(lib, [("write", A, "none"), ("params", 1, 2, 0), ("write", B, "finish")])
    assert [s.rc for s in steps] == [S.OK, S.OK, S.END_OF_STREAM] and not steps[1].out
    assert [(c.level, c.strategy, c.n, c.hist) for c in calls] == [(1, 2, len(A) + len(B), 0)]


def test_a_flush_without_buffered_input_makes_no_compress_call(lib):
    steps, calls = _calls(lib, [("write", b"", "sync"), ("write", A, "sync"), ("write", b"", "full"),
                                ("write", b"", "finish")])
    assert [s.rc for s in steps] == [S.OK, S.OK, S.OK, S.END_OF_STREAM]
    assert len(calls) == 1 and calls[0].n == len(A)
