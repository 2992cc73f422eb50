"""The lane kernel's decoder / expander protocol on hand-built tokens
(tests/token_cases.py writes the streams; the oracle decides every answer).

The expander takes tokens in stream order, keeps loaded match chunks over an
iteration and applies the output checks of every data token itself
(pmd_inflate_lane3.hip, "Output checks"): when a token does not fit, or its
distance reaches before the window, the expander writes the message's result,
raises the stop bit of its tail word and drops the tokens the decoder had
already sent.  The families here are the ones that protocol can get wrong:

* chains of matches whose source ends 0 .. 40 bytes before its destination,
  with 0 .. 4 literals between them: a source made by the previous token, by
  the one before it and by the one before that;
* distances 1 .. 7 (the pattern path) followed at once by another pattern
  distance, by distance 8 and by distance 16, and a 258-byte pattern match
  followed by a far match into its middle;
* capacities around every edge of the overflowing token -- a literal among
  four, a lone literal, a match cut in its first and in a later chunk, a
  pattern match -- in pmd and in raw framing; distances one past the start of
  the output, and of a connection's history;
* which of two failing tokens decides: the first in stream order;
* a batch larger than the grid's lanes, so lanes take a new message from the
  work queue right after a stopped one; and, with one resident workgroup in a
  process of its own, an expander that trails the decoder by a whole ring when
  the stopped message's lane is handed its next message.

Every batch goes into canary-filled memory with guards between the slots, and
lanes of one wave run different families (the jobs are shuffled).  The CPU
test asserts that the oracle alone gives each case the status it is built
for, so every family reaches the branch it names."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import token_cases as T

CANARY, GUARD = 0xA5, 64
BATCH = 192   # three workgroups
OK, NEED, DIST, LITLEN = 0, 1, 13, 11
assert (O.ERRORS[NEED], O.ERRORS[DIST], O.ERRORS[LITLEN]) == ("need_buffers", "invalid_distance", "invalid_literal_length")


class Job:
    __slots__ = ("name", "payload", "cap", "raw", "want", "st", "out")

    def __init__(self, name, payload, cap, raw, want):
        """want: the status the case is built for (a tuple: any of them), or None where only the oracle says."""
        self.name, self.payload, self.cap, self.raw = name, payload, cap, raw
        self.want = want if want is None or isinstance(want, tuple) else (want,)
        self.st, self.out = O.pmd_inflate(payload, cap=cap, raw=raw)


def _lits(seed, n):
    return T._lits(random.Random(seed), n)


def _mode(k):
    return ("fixed", "dyn")[k % 2]


def _full(raw):
    return OK if raw else NEED   # the status of a full output (pmd_inflate.hip)


# ------------------------------------------------------------------ families
CHAIN_LENS = [3, 4, 15, 16, 17, 32, 33, 258]


def chain_jobs():
    """Every match's source ends `gap` bytes before its destination
    (distance = length + gap), `nlit` literals between the matches."""
    jobs = []
    for gap in range(41):
        for nlit in range(5):
            toks = _lits(1000 + gap, 300)
            for i, n in enumerate(CHAIN_LENS):
                toks += _lits(10 * gap + i, nlit) + [(n, n + gap)]
            r = T.render(toks, _mode(gap + nlit))
            assert r.good
            jobs.append(Job("chain gap %d, %d literals between" % (gap, nlit), r.payload, len(r.out), False, OK))
    return jobs


def pattern_jobs():
    jobs = []
    for p in range(1, 8):
        for n in (3, 9, 258):
            for q in (p % 7 + 1, 8, 16):
                for n2 in (3, 40):
                    r = T.render(_lits(p, 16) + [(n, p), (n2, q)] + _lits(q, 3), _mode(p + n))
                    assert r.good
                    jobs.append(Job("pattern (%d, %d) then (%d, %d)" % (n, p, n2, q), r.payload, len(r.out), False, OK))
        for far in (100, 129, 250):   # into the middle of the 258 pattern bytes
            r = T.render(_lits(p, 20) + [(258, p), (40, far), (5, 3)], _mode(p))
            assert r.good
            jobs.append(Job("pattern (258, %d) then (40, %d)" % (p, far), r.payload, len(r.out), False, OK))
    return jobs


def _overflow_tokens(kind, n):
    """Tokens whose output is n bytes and whose last token is of `kind`, or
    None where n bytes cannot end that way (a match is at least 3 bytes after
    at least one byte; a chunked match needs a distance of 8 or more)."""
    if kind == "lit4":
        return _lits(n, n)
    if kind == "lone":   # a literal after a match is the only symbol of its token's literal part
        return _lits(n, n) if n < 5 else _lits(n, n - 4) + [(3, 1), 7]
    if kind == "pattern":
        return None if n < 5 else _lits(n, 2) + [(min(258, n - 2), 2)] + _lits(n + 1, max(0, n - 260))
    if kind == "match16":   # 16-byte chunks: cut in the first or in a later one
        return None if n < 64 else _lits(n, n - min(258, n - 20)) + [(min(258, n - 20), 20)]
    if kind == "match8":    # 8-byte chunks
        return None if n < 64 else _lits(n, n - min(258, n - 9)) + [(min(258, n - 9), 9)]
    raise AssertionError(kind)


def overflow_jobs():
    jobs = []
    for n in (1, 5, 64, 300):
        caps = sorted({c for c in (0, 1, n - 259, n - 258, n - 17, n - 16, n - 5, n - 4, n - 1, n, n + 1, n + 15) if c >= 0})
        for kind in ("lit4", "lone", "match16", "match8", "pattern"):
            toks = _overflow_tokens(kind, n)
            if toks is None:
                continue
            for mode in ("fixed", "dyn"):
                r = T.render(toks, mode)
                assert r.good and len(r.out) == n
                for raw in (False, True):
                    for cap in caps:
                        jobs.append(Job("overflow %s n %d cap %d" % (kind, n, cap), r.payload, cap, raw,
                                        OK if cap >= n else _full(raw)))
    return jobs


def too_far_jobs():
    """dist == pos + 1; at cap == pos the reference's order between "full" and
    "too far" decides: raw framing reports the full output first."""
    jobs = []
    for pos in (0, 1, 7, 8, 300):
        for mode in ("fixed", "dyn"):
            r = T.render(_lits(pos, pos) + [(5, pos + 1)] + _lits(pos + 1, 6), mode)
            assert not r.good and len(r.out) == pos
            for raw in (False, True):
                jobs.append(Job("too far at %d, roomy" % pos, r.payload, pos + 20, raw, DIST))
                jobs.append(Job("too far at %d, one byte of room" % pos, r.payload, pos + 1, raw, DIST))
                jobs.append(Job("too far at %d, full" % pos, r.payload, pos, raw, OK if raw else DIST))
    return jobs


def precedence_jobs():
    jobs = []
    # (only the fixed code has code words no symbol may use: 286 and 287)
    for gap in (1, 2, 31):
        fill = _lits(gap, gap - 1)
        for lead in (10, 11, 12, 13):   # the failing token as every symbol of its iteration
            r = T.render(_lits(1, lead) + [(5, 400)] + fill + [("L", 286)] + _lits(2, 5), "fixed")
            jobs.append(Job("too far, invalid code %d tokens later" % gap, r.payload, 200, False, DIST))
            r = T.render(_lits(1, lead) + [("L", 286)] + fill + [(5, 400)] + _lits(2, 5), "fixed")
            jobs.append(Job("invalid code, too far %d tokens later" % gap, r.payload, 200, False, LITLEN))
    for mode in ("fixed", "dyn"):
        for raw in (False, True):
            if mode == "fixed":
                r = T.render(_lits(3, 20) + [(30, 10), ("L", 286)] + _lits(4, 5), mode)
                jobs.append(Job("overflow, then an invalid code", r.payload, 25, raw, _full(raw)))
                jobs.append(Job("invalid code after a token that fits", r.payload, 50, raw, LITLEN))
            r = T.render(_lits(3, 20) + [(30, 10)] + _lits(5, 40), mode)
            cut = r.bit[22 + 20] // 8   # the payload ends among the trailing literals
            jobs.append(Job("overflow, then truncated input", r.payload[:cut], 25, raw, _full(raw)))
            jobs.append(Job("truncated input, roomy", r.payload[:cut], 200, raw, None))
    return jobs


FAMILIES = {"chain": chain_jobs, "pattern": pattern_jobs, "overflow": overflow_jobs, "too_far": too_far_jobs,
            "precedence": precedence_jobs}
_BUILT = {}


def family(name):
    """Built once, oracle's answers included, and never changed."""
    if name not in _BUILT:
        _BUILT[name] = FAMILIES[name]()
    return _BUILT[name]


HIST = (1, 7, 8, 300)


def history_connections():
    """(name, [first payload, second payload], status wanted of the second):
    the second message's match reaches exactly the history's first byte, or
    one byte before it."""
    conns = []
    for h in HIST:
        first = T.render(_lits(h, h)).payload
        for k in (0, 1, 3, 9):
            for extra in (0, 1):
                toks = _lits(100 * h + k, k) + [(5, k + h + extra)] + _lits(k, 4)
                conns.append(("history %d, %d literals, distance %d" % (h, k, k + h + extra),
                              [first, T.render(toks, _mode(k)).payload], DIST if extra else OK))
    return conns


# ---------------------------------------------------------------------- CPU
def test_the_oracle_gives_every_case_the_status_it_is_built_for():
    count = 0
    for fam in sorted(FAMILIES):
        for j in family(fam):
            if j.want is not None:
                assert j.st in j.want, (fam, j.name, j.cap, j.raw, O.ERRORS.get(j.st, j.st))
            if j.st in (OK, NEED) and j.want is not None and j.name.startswith("overflow "):
                assert len(j.out) == min(j.cap, len(O.pmd_inflate(j.payload, cap=1 << 12, raw=j.raw)[1])), j.name
            count += 1
    assert count > 900
    truncated = [j for j in family("precedence") if j.name == "truncated input, roomy"]
    # (the input runs out after the overflowing token and before the message's 90 bytes are made)
    assert truncated and all(25 < len(j.out) < 90 for j in truncated)
    for name, pls, want in history_connections():
        sts = [st for st, _ in O.pmd_inflate_stream(pls, cap=1024)]
        assert sts == [OK, want], (name, sts)


# ---------------------------------------------------------------------- GPU
def _pmd():
    import torch  # noqa: F401
    from beast_amd import pmd
    return pmd


@pytest.fixture
def lane_kernel():
    pmd = _pmd()
    assert pmd.lib().bpmd_set_inflate_kernel(1) == 0
    yield pmd
    pmd.lib().bpmd_set_inflate_kernel(0)


def _layout(caps, seed):
    """Slots in a shuffled order, GUARD canary bytes or more before each, their
    offsets at every residue mod 16; 16 spare bytes end the buffer."""
    order = list(range(len(caps)))
    random.Random(seed).shuffle(order)
    off, cur = [0] * len(caps), 0
    for k, i in enumerate(order):
        cur += GUARD
        cur += (k - cur) % 16
        off[i] = cur
        cur += caps[i]
    return off, cur + GUARD + 16


def _run(pmd, jobs, raw, label):
    """One batch into canary-filled memory; the list of what differs from the oracle."""
    import torch
    caps = [j.cap for j in jobs]
    off, size = _layout(caps, len(jobs))
    out = torch.full((size,), CANARY, dtype=torch.uint8, device="cuda")
    res = pmd.inflate_batch(pmd.Batch.from_host([j.payload for j in jobs]), torch.tensor(caps, dtype=torch.int32),
                            raw=raw, out=out, out_off=torch.tensor(off, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    st, ln, data = res.status.cpu().tolist(), res.out.len.cpu().tolist(), out.cpu().numpy()
    fails = []
    outside = np.ones(size, dtype=bool)
    for i, j in enumerate(jobs):
        outside[off[i]:off[i] + j.cap] = False
        got = data[off[i]:off[i] + max(0, min(ln[i], j.cap))].tobytes()
        if st[i] != j.st or ln[i] != len(j.out) or got != j.out:
            d = next((k for k, (a, b) in enumerate(zip(got, j.out)) if a != b), None)
            fails.append("%s: %s (cap %d, raw %d): status %s want %s, out_len %d want %d, first byte differing %s" % (
                label, j.name, j.cap, j.raw, O.ERRORS.get(st[i], st[i]), O.ERRORS[j.st], ln[i], len(j.out), d))
    hit = np.flatnonzero(outside & (data != CANARY))
    if len(hit):
        fails.append("%s: %d bytes outside every slot overwritten, the first at %d" % (label, len(hit), int(hit[0])))
    return fails


def _run_all(pmd, jobs, label, seed=7):
    fails, count = [], 0
    for raw in (False, True):
        js = [j for j in jobs if j.raw == raw]
        random.Random(seed).shuffle(js)   # lanes of one wave run different cases
        for b in range(0, len(js), BATCH):
            part = js[b:b + BATCH]
            if len(part) < 64 and b:      # no batch under one workgroup: top it up from the start
                part = part + js[:64 - len(part)]
            fails += _run(pmd, part, raw, label)
            count += len(part)
    assert not fails, "%d of %d differ:\n%s" % (len(fails), count, "\n".join(fails[:8]))


@pytest.mark.gpu
@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_family_matches_the_oracle(lane_kernel, fam):
    _run_all(lane_kernel, family(fam), fam)


@pytest.mark.gpu
def test_lanes_of_one_wave_run_different_families(lane_kernel):
    """Chains, pattern matches and stopped messages side by side in every
    wave: the lanes' pieces in flight differ in number and kind."""
    rng = random.Random(11)
    jobs = []
    for fam in sorted(FAMILIES):
        js = [j for j in family(fam) if not j.raw]
        jobs += rng.sample(js, min(len(js), 77))
    for raw_job in rng.sample([j for j in family("overflow") if j.raw], 64):
        jobs.append(raw_job)
    _run_all(lane_kernel, jobs, "mixed", seed=3)


@pytest.mark.gpu
def test_history_edges(lane_kernel):
    """pmd framing only: context takeover (pmd.TakeoverInflater,
    bpmd_inflate_takeover_batch) has no raw framing, and the oracle's
    pmd_inflate_stream neither; raw framing's order between "full" and "too
    far" is family too_far's."""
    import torch
    pmd = lane_kernel
    conns = history_connections()
    tk = pmd.TakeoverInflater(len(conns), window_bits=15, max_msg=1024)
    expect = [O.pmd_inflate_stream(pls, cap=1024) for _, pls, _ in conns]
    fails = []
    for r in range(2):
        res = tk.inflate(pmd.Batch.from_host([pls[r] for _, pls, _ in conns]), 1024)
        torch.cuda.synchronize()
        st, outs = res.status.cpu().tolist(), res.out.to_host()
        for i, (name, _, _) in enumerate(conns):
            est, eout = expect[i][r]
            if st[i] != est or outs[i] != eout:
                fails.append("%s, message %d: status %s want %s, out_len %d want %d" % (
                    name, r, O.ERRORS.get(st[i], st[i]), O.ERRORS[est], len(outs[i]), len(eout)))
    assert not fails, "\n".join(fails[:8])


@pytest.mark.gpu
def test_a_lane_takes_a_new_message_after_a_stopped_one(lane_kernel):
    """More messages than the resident grid has lanes (four workgroups per
    compute unit, 64 lanes each, some 69 Ki messages in all: the only way to
    the work queue from pmd.py in this process; the case below reaches it
    with a small grid in a process of its own).  The forced lane kernel then
    runs from its queue, longest payload first, so the lanes do not take the
    messages in the batch's order; stopped and good messages of every length
    class are mixed, and lanes take a NEW message after a stopped one."""
    import torch
    pmd = lane_kernel
    lanes = 4 * torch.cuda.get_device_properties(0).multi_processor_count * 64
    rng = random.Random(5)
    stopped = [j for f in ("overflow", "too_far", "precedence") for j in family(f) if not j.raw and j.st != OK]
    good = [j for f in ("chain", "pattern") for j in family(f)]
    base = []
    for a, b in zip(rng.sample(stopped, 48), rng.sample(good, 48)):
        base += [a, b]
    n = lanes + 4096
    jobs = (base * (n // len(base) + 1))[:n]
    assert len(jobs) > lanes
    fails = _run(pmd, jobs, False, "queue")
    assert not fails, "%d of %d differ:\n%s" % (len(fails), n, "\n".join(fails[:8]))


# ------------------------------------------------- NEW waits for the drained ring
def trailing_expander_jobs():
    """64 messages whose 40 matches of 258 bytes keep the expander a ring's
    length behind the decoder, with a literal that does not fit two tokens
    before the end: the decoder has sent the END and waits for its next
    message while the failing token is still in the ring.  Then 192 messages
    of 40 four-literal tokens in one fixed block (no header waits for the
    ring), which the lanes take from the queue."""
    toks = _lits(9, 300) + [(258, 300)] * 40 + _lits(10, 8)
    r = T.render(toks, "fixed")
    first = [Job("long matches, then a literal that does not fit", r.payload, 300 + 40 * 258 + 4, False, NEED)
             for _ in range(64)]
    nxt = [Job("160 literals, message %d" % i, T.render(_lits(20 + i, 160), "fixed").payload, 160, False, OK)
           for i in range(192)]
    assert len(first[0].payload) >= len(nxt[0].payload) + 64   # the queue's order: longest payload first
    return first + nxt


def test_the_oracle_on_the_trailing_expander_jobs():
    jobs = trailing_expander_jobs()
    assert all(j.st in j.want for j in jobs)
    assert len(jobs[0].out) == jobs[0].cap and all(len(j.out) == 160 for j in jobs[64:])


def _small_grid_main():
    """Child process: one resident workgroup (BPMD_QUEUE_WGS is read once per process)."""
    pmd = _pmd()
    assert pmd.lib().bpmd_set_inflate_kernel(1) == 0
    fails = _run(pmd, trailing_expander_jobs(), False, "one workgroup")
    print("\n".join(fails[:8]))
    raise SystemExit(1 if fails else 0)


@pytest.mark.gpu
def test_new_is_not_published_before_the_stopped_message_is_taken():
    """This test is about a second process: the queue's grid comes from the
    environment when the library first plans a batch."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BPMD_QUEUE_WGS="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", "from tests import test_gpu_lane3_pipeline as t; t._small_grid_main()"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
