"""Context-takeover streams on the GPU.

Without no_context_takeover, every connection's messages continue one deflate
stream: Beast's deflater is not reset between messages (impl_base.hpp:156-166)
and its inflater keeps its window (impl_base.hpp:192-202), so a message may
copy from earlier messages.  Each batch holds one message per connection; the
GPU must produce the oracle's bytes and statuses decoding the same stream
message by message."""
import random

import numpy as np
import pytest

from beast_amd import synth
from oracle import oracle as O
from tests import takeover_cases as TC

pytestmark = pytest.mark.gpu


def _streams(rng, n_conn, rounds, level=6, wbits=15):
    msgs, pls = [], []
    for c in range(n_conn):
        kind = rng.choice(["json", "corpus1", "json"])
        ms = []
        for r in range(rounds):
            d, _, _ = synth.make_batch(kind, [rng.choice([0, 50, 700, 4096, 9000])], seed=c * 131 + r)
            ms.append(bytes(d))
        msgs.append(ms)
        pls.append(O.pmd_deflate_stream(ms, level, wbits, 4))
    return msgs, pls


@pytest.mark.parametrize("wbits", [15, 10])
def test_takeover_streams_match_oracle(wbits):
    import torch
    from beast_amd import pmd
    rng = random.Random(21 + wbits)
    n_conn, rounds = 200, 6
    msgs, pls = _streams(rng, n_conn, rounds, wbits=wbits)
    cap = 9000
    expect = [O.pmd_inflate_stream(p, cap=cap, wbits=wbits) for p in pls]
    tk = pmd.TakeoverInflater(n_conn, window_bits=wbits, max_msg=cap)
    uses_history = 0
    for r in range(rounds):
        batch = pmd.Batch.from_host([pls[c][r] for c in range(n_conn)])
        res = tk.inflate(batch, cap)
        torch.cuda.synchronize()
        st = res.status.cpu().tolist()
        outs = res.out.to_host()
        for c in range(n_conn):
            est, eout = expect[c][r]
            assert st[c] == est, (r, c, st[c], est)
            assert outs[c] == eout == msgs[c][r], (r, c)
        if r:
            fresh = [O.pmd_inflate(pls[c][r], cap=cap)[0] for c in range(n_conn)]
            uses_history += sum(1 for f in fresh if f != 0)
    assert uses_history > 0   # the streams really do reach into earlier messages


def test_distance_past_the_window_is_invalid():
    import torch
    from beast_amd import pmd
    rng = random.Random(5)
    # compressed with a 32 KiB window, decoded with a 512-byte one
    msgs, pls = _streams(rng, 64, 3, wbits=15)
    expect = [O.pmd_inflate_stream(p, cap=9000, wbits=9) for p in pls]
    tk = pmd.TakeoverInflater(64, window_bits=9, max_msg=9000)
    for r in range(3):
        res = tk.inflate(pmd.Batch.from_host([pls[c][r] for c in range(64)]), 9000)
        torch.cuda.synchronize()
        st = res.status.cpu().tolist()
        for c in range(64):
            if r == 0 or all(expect[c][k][0] == 0 for k in range(r)):
                assert st[c] == expect[c][r][0], (r, c, st[c], expect[c][r][0])
    # decoder windows of 512, 1024 and 4096 bytes: the same streams and texts
    # of period W - 1, W and W + 1 (their matches reach exactly that far, into
    # the message before), bytes as well as statuses up to each connection's
    # first failure
    from tests.deflate_scripts import periodic
    for wbits in (9, 10, 12):
        W = 1 << wbits
        texts = [[periodic(p, 3 * n, seed=p % 5)[k * n:(k + 1) * n] for k in range(3)]
                 for p in (W - 1, W, W + 1) for n in (W // 2 + 3, W + 5, 2 * W + 1, 9000)]
        pls_w = pls + [O.pmd_deflate_stream(ms, 9, 15, 8) for ms in texts]
        caps = [[9000] * 3 for _ in pls_w]
        expect = [O.pmd_inflate_stream(p, cap=9000, wbits=wbits) for p in pls_w]
        failed = sum(1 for e in expect if any(s for s, _ in e))
        assert 0 < failed < len(expect), (wbits, failed)   # both outcomes occur
        tk = pmd.TakeoverInflater(len(pls_w), window_bits=wbits, max_msg=9000)
        _run_takeover_inflate(tk, pls_w, expect, [list(range(len(pls_w)))] * 3, caps)


def _periodic_messages(rng, c, rounds):
    """One connection's messages as consecutive pieces of a text of period P
    (tests/deflate_scripts.py periodic): the cheapest match of every byte
    past the first period is exactly P back, in an earlier message for a
    piece shorter than P.  P on both sides of max_dist = 2^wbits - 262 for
    windowBits 9 (250) and 10 (762) and of the 2048- and 4096-byte chunk
    histories."""
    from tests.deflate_scripts import periodic
    period = (100, 250, 251, 300, 700, 762, 763, 2047, 2048, 2049, 4096, 5000)[c % 12]
    lens = [rng.choice([1, 300, 2000, 4096, 6000]) for _ in range(rounds)]
    text = periodic(period, sum(lens), seed=c % 5)
    cuts = [sum(lens[:r]) for r in range(rounds + 1)]
    return [text[a:b] for a, b in zip(cuts, cuts[1:])]


@pytest.mark.parametrize("level,wbits", [(6, 15), (1, 10), (9, 9), (0, 15)])
def test_takeover_deflate_round_trips_and_shrinks(level, wbits):
    """GPU deflate with context takeover: every connection's payload stream
    inflates (oracle, window kept, at the deflater's windowBits: a match from
    beyond the window is invalid_distance) back to its messages, and above
    level 0 reaching into earlier messages makes the payloads smaller than
    independent ones."""
    import torch
    from beast_amd import pmd
    rng = random.Random(31)
    n_conn, rounds = 150, 5
    msgs = []
    for c in range(n_conn):
        if wbits == 15:
            msgs.append([bytes(synth.make_batch("json", [rng.choice([1, 300, 2000, 4096, 6000])], seed=c * 7 + r)[0])
                         for r in range(rounds)])
        else:
            msgs.append(_periodic_messages(rng, c, rounds))
    td = pmd.TakeoverDeflater(n_conn, level=level, window_bits=wbits, max_msg=6000)
    pls = [[None] * rounds for _ in range(n_conn)]
    took = plain = 0
    for r in range(rounds):
        src = pmd.Batch.from_host([msgs[c][r] for c in range(n_conn)])
        res = td.deflate(src)
        ind = pmd.deflate_batch(src, level=level, window_bits=wbits)
        torch.cuda.synchronize()
        assert res.status.cpu().tolist() == [0] * n_conn
        outs = res.out.to_host()
        for c in range(n_conn):
            pls[c][r] = outs[c]
        if r:
            took += sum(len(o) for o in outs)
            plain += sum(ind.out.len.cpu().tolist())
    for c in range(n_conn):
        got = O.pmd_inflate_stream(pls[c], cap=6000, wbits=wbits)
        assert [g[0] for g in got] == [0] * rounds, c
        assert [g[1] for g in got] == msgs[c], c
    if level > 0:
        assert took < plain, (took, plain)
    else:   # stored blocks: every payload holds its message's bytes
        assert took >= sum(len(m[r]) for m in msgs for r in range(1, rounds)), took


# ---------------------------------------------------------------------------
# Takeover deflate, byte for byte against the host model with history
# (tests/model: model.encode(..., hist=...); tests/test_model.py shows that
# these message sets tell a wrong history clamp, chain cap or segment floor
# apart from the right one)

@pytest.mark.parametrize("level,wbits", TC.DEFLATE_CASES)
def test_takeover_deflate_equals_model(level, wbits):
    import torch
    from beast_amd import pmd
    from tests.model import model as M
    conns, msgs = TC.deflate_set(wbits)
    n_conn = len(msgs)
    td = pmd.TakeoverDeflater(n_conn, level=level, window_bits=wbits, max_msg=TC.MAX_MSG)
    assert td.HIST == TC.DEFLATE_HIST and td.slot == TC.takeover_slot(td.HIST, TC.MAX_MSG)
    plain = [np.frombuffer(b"".join(ms), dtype=np.uint8) for ms in msgs]   # this test's record of each connection
    sent, pos, total = [0] * n_conn, [0] * n_conn, [0] * n_conn
    pls = [[] for _ in range(n_conn)]
    slid = 0
    for r, cr in enumerate(conns):
        assert len(set(cr)) == len(cr) <= n_conn - n_conn // 3
        batch = [msgs[c][sent[c]] for c in cr]
        res = td.deflate(pmd.Batch.from_host(batch), conn=torch.tensor(cr))
        torch.cuda.synchronize()
        assert res.status.cpu().tolist() == [0] * len(cr), (r, res.status.cpu().tolist())
        outs = res.out.to_host()
        off, lens, hist = [], [], []
        for i, c in enumerate(cr):
            if pos[c] + len(batch[i]) > td.slot:   # the deflater's rule: the window slides to the front
                pos[c] = min(pos[c], td.HIST)
                slid += 1
            off.append(total[c])
            lens.append(len(batch[i]))
            hist.append(min(pos[c], td.HIST))
            assert hist[-1] == min(total[c], td.HIST)
            pos[c] += len(batch[i])
            total[c] += len(batch[i])
            sent[c] += 1
        assert td.pos.cpu().tolist() == pos, r
        for i, c in enumerate(cr):
            (want,) = M.encode(plain[c], [off[i]], [lens[i]], level=level, wbits=wbits, hist=[hist[i]])
            assert outs[i] == want, (r, c, lens[i], hist[i], len(outs[i]), len(want))
            pls[c].append(outs[i])
    assert sent == [len(ms) for ms in msgs]
    assert slid >= 20, slid
    for c in range(n_conn):
        got = O.pmd_inflate_stream(pls[c], cap=TC.MAX_MSG, wbits=wbits)
        assert [g[0] for g in got] == [0] * len(msgs[c]), c
        assert [g[1] for g in got] == msgs[c], c


NEED_BUFFERS = 1
CANARY, GUARD = 0xA5, 64


def _block_ends(payload):
    """Byte offsets just past every block of a payload made of stored blocks
    only (markers included), and the one-byte tail."""
    ends, p = [], 0
    while p < len(payload) - 1:
        assert payload[p] == 0, p   # 000 and padding, on a byte boundary
        ln = payload[p + 1] | payload[p + 2] << 8
        assert ln ^ 0xFFFF == payload[p + 3] | payload[p + 4] << 8
        p += 5 + ln
        ends.append(p)
    assert p == len(payload) - 1 and payload[p] == 0
    return ends


def _capacity_sweep(data, in_off, in_len, hist, caps, want, bits, level=6):
    """Deflate the one message data[in_off : in_off + in_len] once per cap in
    one batch (every entry reads the same input), into canary-filled slots
    with GUARD bytes between them.  hist None: bpmd_deflate_batch, else
    bpmd_deflate_takeover_batch with that much history.  bits: where the
    model's last block ends.  Returns the smallest accepted cap."""
    import ctypes
    import torch
    from beast_amd import pmd
    n, L = len(caps), len(want)
    dev = "cuda"
    d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    off = torch.full((n,), in_off, dtype=torch.int64, device=dev)
    ln = torch.full((n,), in_len, dtype=torch.int32, device=dev)
    cap = torch.tensor(caps, dtype=torch.int32, device=dev)
    out_off_h = np.concatenate([[0], np.cumsum(np.array(caps, dtype=np.int64) + GUARD)[:-1]]) + GUARD
    size = int(out_off_h[-1]) + caps[-1] + GUARD
    out = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
    out_off = torch.from_numpy(out_off_h).to(dev)
    if hist is None:
        res = pmd.deflate_batch(pmd.Batch(d_in, off, ln), level=level, out_cap=cap, out=out, out_off=out_off)
        out_len, status = res.out.len, res.status
    else:
        out_len = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        hl = torch.full((n,), hist, dtype=torch.int32, device=dev)
        cfg = pmd._Cfg(level, 15, 4, 0, 0)
        pmd._check(pmd.lib().bpmd_deflate_takeover_batch(
            ctypes.byref(cfg), pmd._ptr(d_in), pmd._ptr(off), pmd._ptr(ln), pmd._ptr(hl), n, pmd._ptr(out),
            pmd._ptr(out_off), pmd._ptr(cap), pmd._ptr(out_len), pmd._ptr(status), pmd._stream_handle(None)),
            "bpmd_deflate_takeover_batch")
    torch.cuda.synchronize()
    st, ol, got = status.cpu().tolist(), out_len.cpu().tolist(), out.cpu().numpy()
    outside = np.ones(size, dtype=bool)
    accepted = []
    for i, c in enumerate(caps):
        o = int(out_off_h[i])
        outside[o:o + c] = False
        assert st[i] in (0, NEED_BUFFERS), (c, st[i])
        if st[i] == 0:
            assert ol[i] <= c and got[o:o + ol[i]].tobytes() == want, (c, ol[i], L)
            accepted.append(c)
        else:
            assert ol[i] == 0, (c, ol[i])
    assert (got[outside] == CANARY).all(), np.flatnonzero(outside & (got != CANARY))[:8]
    first = min(accepted)
    print("%s: payload %d bytes, last block ends %d bits into a byte, smallest accepted cap %d"
          % ("plain" if hist is None else "takeover", L, bits % 8, first))
    assert accepted == [c for c in caps if c >= first], "statuses are not monotone in cap"
    assert first in (L, L + 1), (first, L)
    # DESIGN.md 4.2b, the smallest accepted capacity: the stitch (every takeover message, every
    # message over one chunk) asks for the byte after a Huffman block's last
    # one, which the tail does not need when the block ends 1-5 bits into a
    # byte; the single-chunk kernel asks for the payload's bytes
    stitched = hist is not None or in_len > 4096
    assert first == L + (1 if stitched and 1 <= bits % 8 <= 5 else 0), (first, L, bits % 8)
    return first


def test_takeover_deflate_capacity_sweep():
    """need_buffers exactly below the payload's size (or one above it when
    the last block ends 1-5 bits into a byte: stitch_kernel asks for the byte
    after a Huffman block's last), never a byte written outside the slot."""
    from tests.model import model as M
    text = TC.json_message(8000, 3)
    bits = []
    (want,) = M.encode(np.frombuffer(text, dtype=np.uint8), [3000], [5000], level=6, hist=[3000], bits=bits)
    L = len(want)
    _capacity_sweep(text, 3000, 5000, 3000, list(range(L + 3)), want, bits[0])
    # stored chunks (random bytes): the stored and marker exits of the stitch
    rnd = TC.random_message(12000, 4)
    (want,) = M.encode(np.frombuffer(rnd, dtype=np.uint8), [3000], [9000], level=6, hist=[3000], bits=bits)
    L = len(want)
    ends = _block_ends(want)
    assert len(ends) == 4   # three stored chunks and chunk 1's marker
    caps = set(range(65)) | set(range(L - 16, L + 3))
    for e in ends:
        caps |= set(range(e - 8, e + 9))
    assert bits[0] % 8 == 0   # a stored block ends on a byte
    _capacity_sweep(rnd, 3000, 9000, 3000, sorted(caps), want, bits[0])
    # without history: the single-chunk kernel's own check, and the stitch
    for n in (3000, 9000):
        text = TC.json_message(n, 6)
        (want,) = M.encode(np.frombuffer(text, dtype=np.uint8), [0], [n], level=6, bits=bits)
        _capacity_sweep(text, 0, n, None, list(range(len(want) + 3)), want, bits[0])


# ---------------------------------------------------------------------------
# Takeover inflate at its edges, against the oracle's inflater kept across
# each connection's messages

def _run_takeover_inflate(tk, pls, expect, conns, caps):
    """Connection c's payloads pls[c] through tk, one per round it takes part
    in (conns[r]: the connections of round r, in submission order), with the
    per-message caps caps[c][k]; expect[c] is the oracle's [(status, bytes)]
    for that stream and those caps.  Up to and including a connection's first
    non-zero status (after it the caller drops the connection): status,
    length and bytes equal the oracle's.  After every round the whole device
    buffer equals this function's own record -- every connection's window
    [base, base + pos), moved to the front when it slid -- except inside the
    called slots [out_off, out_off + cap): idle and failed connections are
    byte-identical to before, and nothing is written past a slot.  Returns
    how often each connection slid."""
    import torch
    from beast_amd import pmd
    n_conn = len(pls)
    sent, dead, slid = [0] * n_conn, [False] * n_conn, [0] * n_conn
    content = [b""] * n_conn
    for r, cr in enumerate(conns):
        cr = [c for c in cr if not dead[c] and sent[c] < len(pls[c])]
        if not cr:
            continue
        want = tk.buf.cpu().numpy().copy()
        cap = [caps[c][sent[c]] for c in cr]
        res = tk.inflate(pmd.Batch.from_host([pls[c][sent[c]] for c in cr]), torch.tensor(cap, dtype=torch.int32),
                         conn=torch.tensor(cr))
        torch.cuda.synchronize()
        got = tk.buf.cpu().numpy()
        st, ln, off = res.status.cpu().tolist(), res.out.len.cpu().tolist(), res.out.off.cpu().tolist()
        called = np.zeros(len(got), dtype=bool)
        for i, c in enumerate(cr):
            base, pos = c * tk.slot, len(content[c])
            if pos + cap[i] > tk.slot:   # the inflater's rule: the window slides to the front
                keep = min(pos, tk.W)
                content[c] = content[c][pos - keep:]
                want[base:base + keep] = np.frombuffer(content[c], dtype=np.uint8)
                slid[c] += 1
                pos = keep
            assert off[i] == base + pos, (r, c, off[i], base, pos)
            called[off[i]:off[i] + cap[i]] = True
            est, eout = expect[c][sent[c]]
            assert st[i] == est, (r, c, sent[c], O.ERRORS.get(st[i], st[i]), O.ERRORS[est])
            assert ln[i] == len(eout), (r, c, sent[c], ln[i], len(eout))
            assert got[off[i]:off[i] + ln[i]].tobytes() == eout, (r, c, sent[c])
            if est == 0:
                content[c] += eout
            else:
                dead[c] = True
            sent[c] += 1
        diff = np.flatnonzero(~called & (got != want))
        assert diff.size == 0, (r, diff[:8].tolist(), tk.slot)
        for c in cr:
            n = len(content[c])
            assert got[c * tk.slot:c * tk.slot + n].tobytes() == content[c], (r, c)
        assert tk.pos.cpu().tolist() == [len(x) for x in content], r
    return slid


def _needs_history(pls, wbits=15, first=1):
    """Messages from `first` on that fail when inflated without what came before."""
    return sum(1 for p in pls[first:] if O.pmd_inflate(p, cap=1 << 16, wbits=wbits)[0] != 0)


def test_takeover_inflate_foreign_encoder():
    """CPython zlib streams (every strategy, level, memLevel, windowBits 9-15,
    messages from empty to max_msg), decoded at the encoder's windowBits."""
    from beast_amd import pmd
    streams = TC.foreign_set()
    rng = random.Random(17)
    uses_history = 0
    for wbits in range(9, 16):
        group = [s for s in streams if s[0] == wbits]
        if not group:
            continue
        pls = [s[2] for s in group]
        caps = [[max(len(m), 1) for m in s[1]] for s in group]
        expect = [O.pmd_inflate_stream(p, cap=k, wbits=wbits) for p, k in zip(pls, caps)]
        for s, e in zip(group, expect):
            assert [x[0] for x in e] == [0] * len(e) and [x[1] for x in e] == s[1]
        uses_history += sum(_needs_history(p, wbits) for p in pls)
        tk = pmd.TakeoverInflater(len(group), window_bits=wbits, max_msg=1 << 16)
        _run_takeover_inflate(tk, pls, expect, TC.schedule(rng, [len(p) for p in pls]), caps)
    assert uses_history > 0


def test_takeover_inflate_tiny_history():
    """Matches into a history of fewer than 8 bytes: the expander's 8-byte
    look-back must stop at the connection's first byte."""
    from beast_amd import pmd
    streams = TC.tiny_history_set()
    pls = [s[1] for s in streams]
    caps = [[16] * len(p) for p in pls]
    expect = [O.pmd_inflate_stream(p, cap=16, wbits=15) for p in pls]
    short = 0   # pieces that start within 8 bytes of the connection's start and need what lies there
    for (msgs, p), e in zip(streams, expect):
        assert [x[1] for x in e] == msgs and not any(x[0] for x in e)
        k = sum(1 for i in range(1, len(msgs)) if sum(map(len, msgs[:i])) <= 8)
        short += _needs_history(p[:k + 1])
    assert short >= 20, short
    tk = pmd.TakeoverInflater(len(pls), window_bits=15, max_msg=16)
    _run_takeover_inflate(tk, pls, expect, [list(range(len(pls)))] * 16, caps)


def test_takeover_inflate_slides_at_window_bits_15():
    """96 KiB per connection through a buffer of 2 * 32768 + 4096 bytes; in
    half of the connections message r repeats message r - 7, so that matches
    reach 28 KiB back, across the slide."""
    from beast_amd import pmd
    n_conn, rounds = 8, 24
    msgs = []
    for c in range(n_conn):
        ms = [TC.json_message(4096, 900 + c * rounds + r) for r in range(rounds)]
        if c % 2:
            for r in range(7, rounds):
                ms[r] = ms[r - 7]
        msgs.append(ms)
    pls = [O.pmd_deflate_stream(ms, 9, 15, 8) for ms in msgs]
    far = [sum(len(p) < 400 for p in pl) for pl in pls]   # a repeated message is a handful of long matches
    assert all(far[c] >= rounds - 8 for c in range(1, n_conn, 2)), far
    caps = [[4096] * rounds for _ in range(n_conn)]
    expect = [O.pmd_inflate_stream(p, cap=4096, wbits=15) for p in pls]
    assert all([x[1] for x in e] == ms for e, ms in zip(expect, msgs))
    tk = pmd.TakeoverInflater(n_conn, window_bits=15, max_msg=4096)
    rng = random.Random(3)
    slid = _run_takeover_inflate(tk, pls, expect, TC.schedule(rng, [rounds] * n_conn), caps)
    assert min(slid) >= 1, slid


def test_takeover_inflate_per_message_caps():
    """Caps of len, len + 77, len // 2 + 1 and 1 mixed in every batch."""
    from beast_amd import pmd
    rng = random.Random(41)
    msgs, pls = _streams(rng, 80, 5)
    caps = [[max(1, min(9000, (len(m), len(m) + 77, len(m) // 2 + 1, 1)[(c + 3 * k) % 4 if k else c % 2]))
             for k, m in enumerate(ms)] for c, ms in enumerate(msgs)]
    expect = [O.pmd_inflate_stream(p, cap=k, wbits=15) for p, k in zip(pls, caps)]
    firsts = [next((x[0] for x in e if x[0]), 0) for e in expect]
    assert firsts.count(NEED_BUFFERS) >= 20 and firsts.count(0) >= 5, firsts
    tk = pmd.TakeoverInflater(len(pls), window_bits=15, max_msg=9000)
    _run_takeover_inflate(tk, pls, expect, TC.schedule(rng, [5] * len(pls)), caps)


def test_takeover_inflate_errors_stay_local():
    """A corrupted or truncated payload in round 3 of 6: that connection
    reports the oracle's status, keeps its position and its window, and every
    other connection of the batch matches the oracle through round 6."""
    from beast_amd import pmd
    rng = random.Random(23)
    n_conn, rounds = 60, 6
    msgs, pls = _streams(rng, n_conn, rounds)
    hit = 0
    for c in range(0, n_conn, 5):
        if len(msgs[c][2]) < 700:   # enough payload to damage
            msgs[c][2] = TC.json_message(700, 300 + c)
            pls[c] = O.pmd_deflate_stream(msgs[c], 6, 15, 4)
        good = pls[c][2]
        for _ in range(200):   # a damage that the oracle notices
            if (c // 5) % 2 and len(good) > 1:
                bad = good[:rng.randrange(len(good))]
            else:
                q = bytearray(good)
                q[rng.randrange(len(q))] ^= 1 << rng.randrange(8)
                bad = bytes(q)
            if O.pmd_inflate_stream(pls[c][:2] + [bad], cap=9000)[2][0] != 0:
                pls[c][2] = bad
                hit += 1
                break
    assert hit == n_conn // 5
    caps = [[9000] * rounds for _ in range(n_conn)]
    expect = [O.pmd_inflate_stream(p, cap=9000, wbits=15) for p in pls]
    assert all(expect[c][2][0] != 0 for c in range(0, n_conn, 5))
    assert all(not any(x[0] for x in expect[c]) for c in range(n_conn) if c % 5)
    tk = pmd.TakeoverInflater(n_conn, window_bits=15, max_msg=9000)
    # everyone in every round, so that round 3 holds the damaged payloads
    # beside sound ones; the order differs from round to round
    conns = [rng.sample(range(n_conn), n_conn) for _ in range(rounds)]
    _run_takeover_inflate(tk, pls, expect, conns, caps)
    done = tk.pos.cpu().tolist()
    for c in range(n_conn):
        k = 2 if c % 5 == 0 else rounds   # a damaged connection stays where round 2 left it
        assert done[c] == sum(len(m) for m in msgs[c][:k]), c


def test_takeover_inflate_writes_nothing_outside_its_slots():
    """bpmd_inflate_takeover_batch itself, on a canary-filled buffer: the
    second message of each connection decoded right after the first one's
    bytes, with caps of len, len + 77, len // 2 + 1 and 1; some slots end
    where the next connection's history begins, the others have 64 guard
    bytes.  Not a byte outside [out_off, out_off + cap) changes."""
    import ctypes
    import torch
    from beast_amd import pmd
    from tests.deflate_scripts import periodic
    rng = random.Random(57)
    pairs = []
    for c in range(96):
        if c % 3 == 0:     # short periods: pattern stores at the slot's end
            p = 1 + c % 13
            text = periodic(64, 64, seed=c)[:p] * 400
            a, b = text[:rng.choice([1, 3, 7, 8, 9, 200])], text[200:200 + rng.choice([5, 16, 17, 300, 2000])]
        else:
            a = TC.json_message(rng.choice([1, 5, 300, 4096]), 70 + c)
            b = a[:len(a) // 2] + TC.json_message(rng.choice([1, 15, 16, 17, 33, 700, 4097]), 170 + c)
        pairs.append((a, b))
    pls = [TC.zlib_stream([a, b], 9, 15) for a, b in pairs]
    caps = [max(1, (len(b), len(b) + 77, len(b) // 2 + 1, 1)[c % 4]) for c, (a, b) in enumerate(pairs)]
    expect = [O.pmd_inflate_stream(p, cap=[max(len(a), 1), k], wbits=15)[1] for p, (a, b), k in zip(pls, pairs, caps)]
    assert _needs_history([x for p in pls for x in p], first=0) > 0
    out_off, hist = [], []
    size = GUARD
    for c, ((a, b), k) in enumerate(zip(pairs, caps)):
        hist.append(len(a))
        out_off.append(size + len(a))
        size += len(a) + k + (0 if c % 2 else GUARD)   # odd: the next connection's history starts at this slot's end
    size += GUARD
    before = np.full(size, CANARY, dtype=np.uint8)
    for (a, b), o in zip(pairs, out_off):
        before[o - len(a):o] = np.frombuffer(a, dtype=np.uint8)
    dev = "cuda"
    buf = torch.from_numpy(before.copy()).to(dev)
    src = pmd.Batch.from_host([p[1] for p in pls])
    n = len(pls)
    d_off = torch.tensor(out_off, dtype=torch.int64, device=dev)
    d_cap = torch.tensor(caps, dtype=torch.int32, device=dev)
    d_hist = torch.tensor(hist, dtype=torch.int32, device=dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    cfg = pmd._Cfg(0, 15, 8, 0, 0)
    pmd._check(pmd.lib().bpmd_inflate_takeover_batch(
        ctypes.byref(cfg), pmd._ptr(src.data), pmd._ptr(src.off), pmd._ptr(src.len), pmd._ptr(d_hist), n,
        pmd._ptr(buf), pmd._ptr(d_off), pmd._ptr(d_cap), pmd._ptr(out_len), pmd._ptr(status),
        pmd._stream_handle(None)), "bpmd_inflate_takeover_batch")
    torch.cuda.synchronize()
    got, st, ln = buf.cpu().numpy(), status.cpu().tolist(), out_len.cpu().tolist()
    outside = np.ones(size, dtype=bool)
    for c, (o, k) in enumerate(zip(out_off, caps)):
        outside[o:o + k] = False
        est, eout = expect[c]
        assert st[c] == est and ln[c] == len(eout), (c, st[c], est, ln[c], len(eout))
        assert got[o:o + ln[c]].tobytes() == eout, c
    diff = np.flatnonzero(outside & (got != before))
    assert diff.size == 0, diff[:8].tolist()


# ---------------------------------------------------------------------------
# bpmd_slide_batch against numpy

def test_slide_batch_moves_exactly_the_window():
    import torch
    from beast_amd import pmd
    rng = random.Random(8)
    keeps = (0, 1, 15, 16, 17, 63, 64, 1023, 1024, 1025, 4096, 32768)
    base, pos, keep = [], [], []
    size = 5
    for i in rng.sample(range(300), 300):
        k = keeps[i % 12]
        p = (2 * k, 2 * k + 1, 2 * k + 13, 3 * k + 5)[(i // 12) % 4]
        size += 1 + i % 7            # unaligned starts, a few bytes between the buffers
        base.append(size)
        pos.append(p)
        keep.append(k)
        size += p + i % 3            # and now and then bytes past pos
    size += 64
    old = np.random.default_rng(8).integers(0, 256, size, dtype=np.uint8)
    want = old.copy()
    for b, p, k in zip(base, pos, keep):
        want[b:b + k] = old[b + p - k:b + p]
    order = rng.sample(range(300), 300)   # the batch order is not the memory order
    dev = "cuda"
    buf = torch.from_numpy(old.copy()).to(dev)
    d_base = torch.tensor([base[i] for i in order], dtype=torch.int64, device=dev)
    d_pos = torch.tensor([pos[i] for i in order], dtype=torch.int32, device=dev)
    d_keep = torch.tensor([keep[i] for i in order], dtype=torch.int32, device=dev)
    pmd._check(pmd.lib().bpmd_slide_batch(pmd._ptr(buf), pmd._ptr(d_base), pmd._ptr(d_pos), pmd._ptr(d_keep), 300,
                                          pmd._stream_handle(None)), "bpmd_slide_batch")
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, diff[:8].tolist()
    assert (want != old).sum() > 100000   # the windows did move


# ---------------------------------------------------------------------------
# Both classes end to end

@pytest.mark.parametrize("wbits", [15, 10])
def test_takeover_deflater_feeds_takeover_inflater(wbits):
    import torch
    from beast_amd import pmd
    conns, msgs = TC.deflate_set(wbits, n_conn=64, rounds=12, seed=91)
    td = pmd.TakeoverDeflater(64, level=6, window_bits=wbits, max_msg=TC.MAX_MSG)
    ti = pmd.TakeoverInflater(64, window_bits=wbits, max_msg=TC.MAX_MSG)
    sent = [0] * 64
    for r, cr in enumerate(conns):
        batch = [msgs[c][sent[c]] for c in cr]
        conn = torch.tensor(cr)
        sent_r = td.deflate(pmd.Batch.from_host(batch), conn=conn)
        assert sent_r.status.cpu().tolist() == [0] * len(cr), r
        caps = torch.tensor([max(len(m), 1) for m in batch], dtype=torch.int32)
        back = ti.inflate(sent_r.out, caps, conn=conn)
        torch.cuda.synchronize()
        assert back.status.cpu().tolist() == [0] * len(cr), (r, back.status.cpu().tolist())
        assert back.out.to_host() == batch, r
        for c in cr:
            sent[c] += 1
    assert sent == [len(ms) for ms in msgs] and max(sent) > min(sent)
