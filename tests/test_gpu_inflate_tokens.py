"""The data step of every inflate decoder on hand-built tokens
(tests/token_cases.py; tests/test_token_cases.py pins the payloads on the CPU).

Encoders almost never emit distance 2-7 with length 258, a match whose source
ends one byte before its destination, a chain of matches inside one 64-byte
chunk, a distance a few bytes from the wave kernel's 4 KiB ring, a distance
beyond 2^windowBits or a 48-bit token, so the suite's other inflate tests do
not reach the code that handles them.  Here:

* every family in every batch decoder (lane, wave, wave with walk rounds and
  with speculative rounds only, block-parallel, automatic): status, length and
  bytes equal to the oracle's;
* families A, D and E again into canary-filled output of the caller's, slots
  at every residue mod 16, half of them touching the next one: no byte outside
  a slot is written and no neighbour's spare bytes land inside one;
* the per-stream inflater (bpmd_inflate_stream_*) on families A, C, D and F,
  call by call against the oracle's inflate_stream, in one roomy call and in
  rooms of 258, 257 and 7 bytes, with the serial and the wave-parallel fast
  loop, at windowBits 15 and 9;
* context takeover: matches that reach exactly to the start of the history
  and one byte before it."""
import ctypes
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import token_cases as T
from tests import zstream_cases as Z

pytestmark = pytest.mark.gpu

MODES = ["lane", "wave", "wave_walk", "wave_spec", "bp", "auto"]
CANARY, GUARD = 0xA5, 64


def _pmd():
    import torch  # noqa: F401
    from beast_amd import pmd
    return pmd


@pytest.fixture(params=MODES)
def inflate_kernel(request):
    """The modes of tests/test_gpu_inflate.py's fixture, and the automatic choice."""
    pmd = _pmd()
    mode = {"lane": 1, "wave": 2, "wave_walk": 2, "wave_spec": 2, "bp": 3, "auto": 0}[request.param]
    walk = {"wave_walk": 1, "wave_spec": 2}.get(request.param, 0)
    assert pmd.lib().bpmd_set_inflate_kernel(mode) == 0
    assert pmd.lib().bpmd_diag_set_wave_walk(walk) == 0
    yield request.param
    pmd.lib().bpmd_set_inflate_kernel(0)
    pmd.lib().bpmd_diag_set_wave_walk(0)


class Job:
    """One case at one (cap, raw, window_bits), with the oracle's answer."""
    __slots__ = ("case", "cap", "raw", "wbits", "st", "out")


_JOBS = {}


def jobs_of(fam):
    """Computed once and shared by every mode and test; never changed."""
    if fam not in _JOBS:
        jobs = []
        for c in T.family(fam):
            for cap, raw, wbits in c.runs:
                j = Job()
                j.case, j.cap, j.raw, j.wbits = c, cap, raw, wbits
                j.st, j.out = O.pmd_inflate(c.payload, cap=cap, raw=raw, wbits=wbits)
                if c.expect == "ok" and cap >= len(c.out):   # the builder's own bytes
                    assert j.out == c.out, c.name
                jobs.append(j)
        _JOBS[fam] = jobs
    return _JOBS[fam]


def _first_diff(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], dtype=np.uint8) != np.frombuffer(b[:n], dtype=np.uint8))
    return int(d[0]) if len(d) else (n if len(a) != len(b) else None)


def _mismatch(j, st, got, mode):
    """None, or what differs: family, token at the first differing byte with
    its (len, dist), output position and mode."""
    at = _first_diff(got, j.out)
    if st == j.st and at is None:
        return None
    return ("%s: status %s want %s, out_len %d want %d, first byte differing %s (cap %d, raw %d, window_bits %d, "
            "payload %d bytes): %s" % (mode, O.ERRORS.get(st, st), O.ERRORS[j.st], len(got), len(j.out), at, j.cap,
                                      j.raw, j.wbits, len(j.case.payload),
                                      j.case.describe(at if at is not None else len(j.out))))


def _inflate(jobs, raw, wbits, out=None, out_off=None):
    """One batch.  Returns (status list, the outputs as bytes, the whole output array)."""
    import torch
    pmd = _pmd()
    src = pmd.Batch.from_host([j.case.payload for j in jobs])
    cap = torch.tensor([j.cap for j in jobs], dtype=torch.int32)
    res = pmd.inflate_batch(src, cap, window_bits=wbits, raw=raw, out=out, out_off=out_off)
    torch.cuda.synchronize()
    st, ln = res.status.cpu().tolist(), res.out.len.cpu().tolist()
    off, data = res.out.off.cpu().tolist(), res.out.data.cpu().numpy()
    bad = [(i, n) for i, n in enumerate(ln) if not 0 <= n <= jobs[i].cap]
    assert not bad, ("out_len outside [0, cap]", bad[:4])
    return st, [data[o:o + n].tobytes() for o, n in zip(off, ln)], data


def _groups(jobs, by_renderer):
    g = {}
    for j in jobs:
        g.setdefault((j.case.mode if by_renderer else "", j.raw, j.wbits), []).append(j)
    return sorted(g.items())


def _report(fails, count):
    assert not fails, "%d of %d differ:\n%s" % (len(fails), count, "\n".join(fails[:6]))


@pytest.mark.parametrize("fam", sorted(T.FAMILIES))
def test_family_matches_the_oracle(inflate_kernel, fam):
    pmd = _pmd()
    mode = inflate_kernel
    jobs = jobs_of(fam)
    fails = []
    for (renderer, raw, wbits), js in _groups(jobs, by_renderer=mode == "bp"):
        if mode == "bp":
            pmd.bp_counters()
        st, outs, _ = _inflate(js, raw, wbits)
        if mode == "bp":
            c = pmd.bp_counters()
            print("family %s [%s] raw %d window_bits %d: %d messages, bp_counters %s, fell back %.1f%%"
                  % (fam, renderer, raw, wbits, len(js), c[:4], 100.0 * (c[2] + c[3]) / max(1, c[0] + c[3])))
            if fam == "A" and renderer == "dyn":
                assert c[0] > 0, c[:4]
        for i, j in enumerate(js):
            m = _mismatch(j, st[i], outs[i], mode)
            if m:
                fails.append(m)
    _report(fails, len(jobs))


def _guarded_layout(jobs, seed):
    """Slots in a shuffled order: every other one touches the one before it,
    the rest follow GUARD canary bytes and a few more that put their offsets,
    in turn, at every residue mod 16.  The buffer ends with the 16 spare bytes
    that pmd.inflate_batch allocates, and nothing else."""
    order = list(range(len(jobs)))
    random.Random(seed).shuffle(order)
    off = [0] * len(jobs)
    cur = GUARD
    for k, i in enumerate(order):
        if k % 2 == 0:
            cur += GUARD
            cur += (k // 2 - cur) % 16
        off[i] = cur
        cur += jobs[i].cap
    return off, cur + 16


@pytest.mark.parametrize("fam", ["A", "D", "E"])
def test_nothing_is_written_outside_a_slot(inflate_kernel, fam):
    import torch
    mode = inflate_kernel
    fails, count = [], 0
    for (_, raw, wbits), js in _groups(jobs_of(fam), by_renderer=False):
        off, size = _guarded_layout(js, len(js))
        assert {o % 16 for o in off} == set(range(16))
        out = torch.full((size,), CANARY, dtype=torch.uint8, device="cuda")
        st, outs, data = _inflate(js, raw, wbits, out=out, out_off=torch.tensor(off, dtype=torch.int64, device="cuda"))
        outside = np.ones(size, dtype=bool)
        for i, j in enumerate(js):
            outside[off[i]:off[i] + j.cap] = False
            m = _mismatch(j, st[i], outs[i], mode)   # after every slot is written: a neighbour's spare bytes too
            if m:
                fails.append("slot at %d (%d mod 16): %s" % (off[i], off[i] % 16, m))
        hit = np.flatnonzero(outside & (data != CANARY))
        if len(hit):
            ends = sorted((off[i] + j.cap, i) for i, j in enumerate(js))
            for h in hit[:4].tolist():
                e, i = max((e, i) for e, i in ends if e <= h) if h >= ends[0][0] else (0, 0)
                fails.append("%s: byte %d outside every slot overwritten, %d past the slot of %s" % (
                    mode, h, h - e, js[i].case.describe(js[i].cap)))
        count += len(js)
    _report(fails, count)


# ------------------------------------------------------------ per-stream inflater
ROOMS = (None, 258, 257, 7)   # None: one call with room for everything
MAX_CALLS = 1000


def _stream_cases(fam):
    """(case, rooms): family A's distances up to 72 and 4095 .. 4097, and all
    of C, D and F.  Every case has its roomy call.  Family A's small rooms
    thin lead-ins (0 and 3, in one renderer each), never distances: at 45 us
    a call that keeps each test near two seconds."""
    picked = []
    for c in T.family(fam):
        rooms = ROOMS
        if fam == "A":
            d, lead = c.key
            if not (d <= 72 or 4095 <= d <= 4097):
                continue
            small = (lead == 0 and c.mode == ("fixed", "dyn")[d % 2]) or (lead == 3 and c.mode == ("dyn", "fixed")[d % 2])
            rooms = ROOMS if small else ROOMS[:1]
        picked.append((c, rooms))
    return picked


@pytest.mark.parametrize("wbits", [15, 9])
@pytest.mark.parametrize("par", [0, -1], ids=["serial", "default"])
@pytest.mark.parametrize("fam", ["A", "C", "D", "F"])
def test_per_stream_inflater(fam, par, wbits):
    from tests.test_gpu_zstream import GpuInflater, _lib
    L = _lib()
    L.bpmd_diag_set_zstream_parallel.argtypes = [ctypes.c_int]
    L.bpmd_diag_set_zstream_parallel(par)
    n_calls = n_cases = 0
    skipped = []
    try:
        for c, rooms in _stream_cases(fam):
            stream = c.payload + Z.EB
            total = len(c.out) + 300
            for room in rooms:
                n = 1 if room is None else -(-total // room)
                if n > MAX_CALLS:
                    skipped.append((c, room))
                    continue
                calls = [(len(stream), room or total, Z.SYNC)] * (n + 2)
                recs = Z.compare(GpuInflater, stream, calls, wbits,
                                 label="room %s, fast loop %s: %s" % (room, par, c.describe(0)))
                n_calls += len(recs)
            n_cases += 1
    finally:
        L.bpmd_diag_set_zstream_parallel(-1)
    print("family %s: %d cases, %d calls, %d (case, room) pairs of over %d calls left out%s" % (
        fam, n_cases, n_calls, len(skipped), MAX_CALLS,
        "".join("; room %d of %s [%s]" % (r, c.name, c.mode) for c, r in skipped)))
    assert n_cases > 0
    # only room 7 on the 40 258 bytes of F's 40000-literal messages is left out
    assert all(fam == "F" and room == 7 and c.key == ("window", c.key[1]) and len(c.out) > 40000 for c, room in skipped)
    assert len(skipped) == (4 if fam == "F" else 0)


# ---------------------------------------------------------------- history
def test_matches_reach_the_start_of_the_history():
    import torch
    pmd = _pmd()
    conns = T.history_connections()
    fails = []
    for wbits in (15, 9):
        cs = [c for c in conns if c[1] == wbits]
        expect = [O.pmd_inflate_stream(pls, cap=1024, wbits=wbits) for _, _, pls in cs]
        tk = pmd.TakeoverInflater(len(cs), window_bits=wbits, max_msg=1024)
        for r in range(2):
            res = tk.inflate(pmd.Batch.from_host([pls[r] for _, _, pls in cs]), 1024)
            torch.cuda.synchronize()
            st, outs = res.status.cpu().tolist(), res.out.to_host()
            for i, (name, _, _) in enumerate(cs):
                est, eout = expect[i][r]
                if st[i] != est or outs[i] != eout:
                    fails.append("window_bits %d, %s, message %d: status %s want %s, out_len %d want %d, first byte "
                                 "differing %s" % (wbits, name, r, O.ERRORS.get(st[i], st[i]), O.ERRORS[est],
                                                   len(outs[i]), len(eout), _first_diff(outs[i], eout)))
    _report(fails, 2 * len(conns))
