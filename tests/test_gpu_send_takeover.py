"""bpmd_send_takeover_batch and pmd.TakeoverSender on the GPU: decide, place,
slide, deflate with the connection's history and frame in one chained call,
against tests/send_takeover_model.py connection by connection.

The connections' buffers, the staging slots and the wire are filled with a
canary, carry guard bytes and stay on the device from call to call; after
every call every output array, d_pos, the whole d_buf and the whole wire
buffer equal what the model gives, and no staging byte outside a slot is
touched."""
import ctypes
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import send_model as SM
from tests import send_takeover_model as TM
from tests import takeover_cases as TC

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 64
K = TM.K
SERVER, CLIENT = 0, 1


def _pmd():
    import torch
    from beast_amd import pmd
    return torch, pmd


class Rig:
    """n connections' device state and this test's own record of it"""

    def __init__(self, n, slot, z_max, wire_max, role, level=6, wbits=15, max_len=1 << 16, threshold=0, frag=True,
                 frame_max=4096, seed=1):
        torch, pmd = _pmd()
        self.n, self.slot, self.role, self.level, self.wbits = n, slot, role, level, wbits
        self.max_len, self.threshold, self.frag, self.frame_max = max_len, threshold, frag, frame_max
        self.L = pmd._send_tk_lib()
        self.cfg = pmd._Cfg(level, wbits, 4, 0, 0)
        dev = "cuda"
        self.h_base = GUARD + slot * np.arange(n, dtype=np.int64)           # packed end to start
        self.h_buf = np.full(2 * GUARD + n * slot, CANARY, dtype=np.uint8)
        self.h_pos = [0] * n
        self.z_max = z_max
        self.h_z_off = GUARD + (z_max + GUARD) * np.arange(n, dtype=np.int64)
        self.z_bytes = GUARD + n * (z_max + GUARD)
        self.wire_max = wire_max
        self.h_wire = np.full(wire_max + GUARD, CANARY, dtype=np.uint8)
        self.d_buf = torch.from_numpy(self.h_buf.copy()).to(dev)
        self.d_base = torch.from_numpy(self.h_base).to(dev)
        self.d_pos = torch.zeros(n, dtype=torch.int32, device=dev)
        self.d_z = torch.full((self.z_bytes,), CANARY, dtype=torch.uint8, device=dev)
        self.d_z_off = torch.from_numpy(self.h_z_off).to(dev)
        self.d_wire = torch.from_numpy(self.h_wire.copy()).to(dev)
        self.d_work = torch.empty(max(int(self.L.bpmd_send_takeover_work_bytes(n)), 1), dtype=torch.uint8, device=dev)
        self.stride = SM.frame_count(SM.upper_bound(20000), frame_max, True, True)   # no test sends a longer message
        rng = random.Random(seed)
        self.keys = [rng.getrandbits(32) for _ in range(n * self.stride)] if role == CLIENT else None
        self.d_keys = pmd._keys(self.keys, n * self.stride, dev) if role == CLIENT else None
        self.d_key_base = (torch.arange(n, dtype=torch.int32, device=dev) * self.stride) if role == CLIENT else None
        self.z_in = np.zeros(self.z_bytes, dtype=bool)
        self.sent = [[] for _ in range(n)]       # per connection: (message, payload) of every compressed message sent
        self.slides = self.plain = self.with_hist = self.entries = 0

    def preset(self, i, content):
        """connection i has compressed `content` before"""
        torch, _ = _pmd()
        assert len(content) <= self.slot
        b = int(self.h_base[i])
        self.h_buf[b:b + len(content)] = np.frombuffer(content, dtype=np.uint8)
        self.h_pos[i] = len(content)
        self.d_buf[b:b + len(content)] = torch.from_numpy(np.frombuffer(content, dtype=np.uint8).copy()).to("cuda")
        self.d_pos[i] = len(content)

    def conn_keys(self, i):
        return None if self.keys is None else self.keys[i * self.stride:(i + 1) * self.stride]

    def call(self, msgs, ops, opts=None, z_caps=None, wire_cap=None, align=16, dry=False):
        """One bpmd_send_takeover_batch call, checked against the model.
        Returns the model's entries and their packing [(off, len, status, pos)]."""
        torch, pmd = _pmd()
        n, dev = self.n, "cuda"
        assert len(msgs) == len(ops) == n
        opts = [1] * n if opts is None else opts
        z_caps = [self.z_max] * n if z_caps is None else z_caps
        wire_cap = self.wire_max if wire_cap is None else wire_cap
        assert max(z_caps) <= self.z_max and wire_cap <= self.wire_max
        # ---- the model, on a copy of this record
        bufs = [bytearray(self.h_buf[int(b):int(b) + self.slot].tobytes()) for b in self.h_base]
        ents = [TM.send(self.h_pos[i], bufs[i], msgs[i], ops[i], opts[i], self.threshold, self.max_len, self.slot,
                        z_caps[i], self.conn_keys(i), self.level, self.wbits, self.frame_max, self.frag)
                for i in range(n)]
        packed, total = TM.pack(ents, wire_cap)
        if dry:
            return ents, packed
        # ---- the call
        src = pmd.Batch.from_host(msgs, align=align)
        t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)  # noqa: E731
        d_op, d_opt, d_z_cap = t(ops, torch.uint8), t(opts, torch.uint8), t(z_caps, torch.int32)
        fill = lambda dt, m=n: torch.full((m,), 0x5A, dtype=dt, device=dev)  # noqa: E731
        z_len, w_off, w_len = fill(torch.int32), fill(torch.int64), fill(torch.int32)
        comp, status, tot = fill(torch.uint8), fill(torch.int32), fill(torch.int64, 1)
        pmd._check(self.L.bpmd_send_takeover_batch(
            ctypes.byref(self.cfg), pmd._ptr(src.data), pmd._ptr(src.off), pmd._ptr(src.len), n, self.role,
            self.threshold, int(self.frag), self.frame_max, self.max_len, pmd._ptr(d_op), pmd._ptr(d_opt),
            pmd._ptr(self.d_buf), pmd._ptr(self.d_base), self.slot, pmd._ptr(self.d_pos), pmd._ptr(self.d_z),
            pmd._ptr(self.d_z_off), pmd._ptr(d_z_cap), pmd._ptr(z_len), pmd._optr(self.d_keys),
            pmd._optr(self.d_key_base), pmd._ptr(self.d_wire), wire_cap, pmd._ptr(w_off), pmd._ptr(w_len),
            pmd._ptr(comp), pmd._ptr(status), pmd._ptr(tot), pmd._ptr(self.d_work), pmd._stream_handle(None)),
            "bpmd_send_takeover_batch")
        torch.cuda.synchronize()
        # ---- this record after the call
        z_in = self.z_in       # bytes inside a staging slot's capacity in this call or an earlier one
        for i, (e, (off, ln, st, pos)) in enumerate(zip(ents, packed)):
            b = int(self.h_base[i])
            self.h_buf[b:b + self.slot] = np.frombuffer(bytes(bufs[i]), dtype=np.uint8)
            self.h_pos[i] = pos
            if ln:
                self.h_wire[off:off + ln] = np.frombuffer(e.wire, dtype=np.uint8)
            z_in[int(self.h_z_off[i]):int(self.h_z_off[i]) + z_caps[i]] = True
            if ops[i] != 0:
                self.entries += 1
                self.slides += e.slid
                self.plain += st == 0 and not e.compressed
                self.with_hist += st == 0 and e.compressed and e.hist > 0
            if st == 0 and e.compressed:
                self.sent[i].append((bytes(msgs[i]), e.payload))
        # ---- every output
        assert comp.cpu().tolist() == [e.compressed for e in ents]
        assert status.cpu().tolist() == [p[2] for p in packed]
        assert w_off.cpu().tolist() == [p[0] for p in packed]
        assert w_len.cpu().tolist() == [p[1] for p in packed]
        assert tot.cpu().tolist() == [total]
        assert self.d_pos.cpu().tolist() == self.h_pos
        got_zl, got_z = z_len.cpu().tolist(), self.d_z.cpu().numpy()
        for i, (e, p) in enumerate(zip(ents, packed)):
            if e.compressed and e.status == 0:       # whatever the wire said afterwards
                o = int(self.h_z_off[i])
                assert got_zl[i] == len(e.payload), (i, got_zl[i], len(e.payload))
                assert got_z[o:o + got_zl[i]].tobytes() == e.payload, i
        assert (got_z[~z_in] == CANARY).all(), np.flatnonzero(~z_in & (got_z != CANARY))[:8]
        got = self.d_buf.cpu().numpy()
        assert np.array_equal(got, self.h_buf), np.flatnonzero(got != self.h_buf)[:8]
        got = self.d_wire.cpu().numpy()
        assert np.array_equal(got, self.h_wire), np.flatnonzero(got != self.h_wire)[:8]
        return ents, packed

    def peer_decodes(self, cap):
        """the oracle's inflater, kept per connection, decodes every compressed message sent so far"""
        for c, s in enumerate(self.sent):
            got = O.pmd_inflate_stream([p for _, p in s], cap=cap, wbits=self.wbits)
            assert got == [(0, m) for m, _ in s], c


@pytest.mark.parametrize("level,wbits,role", [(1, 15, SERVER), (6, 15, CLIENT), (9, 15, SERVER), (1, 9, CLIENT),
                                              (6, 9, SERVER), (9, 9, CLIENT)])
def test_connections_out_of_step(level, wbits, role):
    rng = random.Random(1000 * level + wbits)
    n, rounds = 96, 8
    slot = TC.takeover_slot(K, TC.MAX_MSG)
    rig = Rig(n, slot, SM.upper_bound(TC.MAX_MSG), n * (TC.MAX_MSG + 400), role, level, wbits, max_len=TC.MAX_MSG,
              threshold=301)
    active = TC.round_conns(rng, n, rounds, idle=5)
    count = [sum(c in cr for cr in active) for c in range(n)]
    lens = [[rng.choice(TC.LENS + TC.LONG) for _ in range(count[c])] for c in range(n)]
    msgs = [TC.connection_messages(c, lens[c], wbits, seed=21) for c in range(n)]
    turn = [0] * n
    for r, cr in enumerate(active):
        assert 0 < len(set(cr)) < n
        batch, ops, opts = [], [], []
        for c in range(n):
            if c in cr:
                batch.append(msgs[c][turn[c]])
                turn[c] += 1
                ops.append(1 + (c + r) % 2)
                opts.append(0 if rng.randrange(6) == 0 else 1)
            else:   # idle, whatever its entry holds
                batch.append(b"idle" * rng.randrange(3))
                ops.append(0)
                opts.append(rng.randrange(2))
        rig.call(batch, ops, opts, align=(16, 1)[r % 2])
    assert turn == count
    assert rig.slides >= 20, rig.slides
    assert 4 * rig.plain >= rig.entries and 4 * rig.with_hist >= rig.entries, (rig.plain, rig.with_hist, rig.entries)
    rig.peer_decodes(TC.MAX_MSG)


@pytest.mark.parametrize("level", [6, 9])
def test_chunk_and_history_edges(level):
    """every message length on both sides of one and two chunks behind every
    history length on both sides of 32 bytes and of the 2 KiB and 4 KiB chunk
    histories; then the same connections once more"""
    lens = (0, 1, 4095, 4096, 4097, 8193)
    hists = (0, 1, 31, 32, 2047, 2048, 2049, 4095, 4096)
    n = len(lens) * len(hists)
    slot = 2 * K + 8193 + 4100 + 7
    rig = Rig(n, slot, SM.upper_bound(8193), n * 8400, SERVER, level, 15, max_len=8193)
    text = [TC.json_message(4096 + 2 * 8193, 50 + i) for i in range(n)]
    cases = [(h, ln) for h in hists for ln in lens]
    for i, (h, ln) in enumerate(cases):
        rig.preset(i, text[i][:h])
    rig.call([text[i][h:h + ln] for i, (h, ln) in enumerate(cases)], [2] * n, align=1)
    rig.call([text[i][h + ln:h + 2 * ln] for i, (h, ln) in enumerate(cases)], [1] * n)
    assert rig.h_pos == [h + 2 * ln for h, ln in cases]


def test_slide_edges_at_every_alignment():
    """pos + len at slot - 1, slot and slot + 1, the buffers packed end to
    start with an odd slot so that their bases take every residue mod 16, the
    messages packed without padding"""
    slot = 2 * K + 1001
    ln = 1000
    n = 48
    rig = Rig(n, slot, SM.upper_bound(ln), n * 1100, CLIENT, 6, 15, max_len=ln)
    assert {int(b) % 16 for b in rig.h_base[:16]} == set(range(16))
    text = [TC.json_message(slot + ln, 300 + i) for i in range(n)]
    ends = (slot - 1, slot, slot + 1)
    for i in range(n):
        rig.preset(i, text[i][:ends[i // 16] - ln])
    ents, _ = rig.call([text[i][ends[i // 16] - ln:ends[i // 16]] for i in range(n)], [2] * n, align=1)
    assert [e.slid for e in ents] == [0] * 32 + [1] * 16
    assert rig.h_pos == [slot - 1] * 16 + [slot] * 16 + [K + ln] * 16
    # full and nearly full buffers: one more byte slides them all, an empty message none
    ents, _ = rig.call([b"x"] * 16 + [b""] * 16 + [b"y"] * 16, [2] * n, align=1)
    assert [e.slid for e in ents] == [0] * 16 + [0] * 16 + [0] * 16
    ents, _ = rig.call([b"zz"] * n, [1] * n, align=1)
    assert [e.slid for e in ents] == [1] * 32 + [0] * 16


def test_statuses_and_unadvanced_connections():
    """max_len on both sides, a staging slot one byte short, a wire that cuts
    the batch's tail off, both in one batch; then the retry: the failed
    connections alone, with room, and the peer decodes every connection"""
    L = 3000
    slot = 2 * K + L       # max_len is more: the buffer's room sets the limit
    n = 12
    rig = Rig(n, slot, SM.upper_bound(L + 1), n * 3400, SERVER, 6, 15, max_len=L + 50, threshold=0)
    assert TM.room(rig.max_len, slot) == L
    text = [TC.json_message(4 * (L + 1), 700 + i) for i in range(n)]
    head = [L - 1] * n
    head[6] = 200          # a short payload: the bytes past the cap set below are untouched so far
    rig.call([t[:h] for t, h in zip(text, head)], [1] * n)    # some history everywhere
    lens = [L - 1, L, L + 1, L + 1, 100, 100, L, 200, 300, L, L, 50]
    ops = [1, 2, 1, 2, 3, 8, 1, 0, 2, 1, 2, 1]
    opts = [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 1]
    msgs = [text[i][head[i]:head[i] + lens[i]] for i in range(n)]
    ents, packed = rig.call(msgs, ops, opts, dry=True)
    assert [e.status for e in ents] == [0, 0, TM.MESSAGE_TOO_BIG, 0, SM.BAD_OPCODE, SM.BAD_OPCODE, 0, 0, 0, 0, 0, 0]
    # the staging slot of entry 6 one byte short; the wire ends one byte before entry 10's last
    z_caps = [rig.z_max] * n
    z_caps[6] = ents[6].need - 1
    assert ents[6].need in (len(ents[6].payload), len(ents[6].payload) + 1)
    wire_cap = packed[10][0] - len(ents[6].wire) + len(ents[10].wire) - 1   # entry 6's frames are not there
    pos0 = list(rig.h_pos)
    ents, packed = rig.call(msgs, ops, opts, z_caps=z_caps, wire_cap=wire_cap)
    st = [p[2] for p in packed]
    # entry 10 lacks one byte; entry 11 behind it is small and still lies past the wire's end
    assert st == [0, 0, TM.MESSAGE_TOO_BIG, 0, SM.BAD_OPCODE, SM.BAD_OPCODE, SM.NEED_BUFFERS, 0, 0, 0,
                  SM.BUFFER_OVERFLOW, SM.BUFFER_OVERFLOW]
    assert packed[9][1] != 0 and packed[10][1] == 0 and packed[11][1] == 0
    for i in (2, 3, 4, 5, 6, 7, 10, 11):           # refused, uncompressed, idle: where they were
        assert rig.h_pos[i] == pos0[i], i
    for i in (0, 1, 8, 9):
        assert rig.h_pos[i] == pos0[i] + lens[i], i
    # ---- the retry: the ones the peer never saw, with room; everyone else idle
    again = [i for i in range(n) if st[i] in (SM.NEED_BUFFERS, SM.BUFFER_OVERFLOW)]
    assert again == [6, 10, 11]
    ents, packed = rig.call(msgs, [ops[i] if i in again else 0 for i in range(n)], opts)
    assert [p[2] for p in packed] == [0] * n
    assert rig.h_pos[6] == pos0[6] + lens[6]
    rig.call([text[i][-500:] for i in range(n)], [2] * n)     # and the connections go on
    assert all(len(s) >= 2 for s in rig.sent)
    rig.peer_decodes(L)


def test_grid_stride_over_many_tiny_messages():
    """12 000 entries: more than the one-wave-per-entry kernels launch waves"""
    rng = random.Random(12)
    n = 12000
    slot = 2 * K + 48
    rig = Rig(n, slot, 96, n * 64, SERVER, 1, 15, max_len=48, threshold=8)
    words = [b"alpha ", b"beta ", b"gamma ", b"delta ", b"{\"id\": 7}", b"\x00\x01\x02"]
    for r in range(2):
        msgs = [b"".join(rng.choice(words) for _ in range(rng.randrange(7)))[:48] for _ in range(n)]
        rig.call(msgs, [rng.choice((0, 1, 2, 2)) for _ in range(n)], [rng.randrange(4) != 0 for _ in range(n)], align=1)
    assert rig.with_hist >= n // 8 and rig.plain >= n // 4, (rig.with_hist, rig.plain)


@pytest.mark.parametrize("sender_role", [CLIENT, SERVER])
def test_round_trip_through_the_takeover_receiver(sender_role):
    """pmd.TakeoverSender -> pmd.TakeoverReceiver: every message arrives as it
    was sent, across slides on both sides, uncompressed text and binary
    messages in between"""
    torch, pmd = _pmd()
    rng = random.Random(70 + sender_role)
    n, rounds, max_msg, wbits = 24, 14, 6000, 12
    tx = pmd.TakeoverSender(n, sender_role, level=6, window_bits=wbits, max_msg=max_msg, threshold=200, frame_max=1500)
    rx = pmd.TakeoverReceiver(n, CLIENT if sender_role == SERVER else SERVER, window_bits=wbits, max_msg=max_msg)
    keys = None
    if sender_role == CLIENT:
        keys = torch.randint(-2 ** 31, 2 ** 31 - 1, (n * tx.key_stride,), dtype=torch.int32, device="cuda")
    out_cap = SM.upper_bound(max_msg)
    tx_slid = rx_slid = plain = 0
    for r in range(rounds):
        msgs, ops, opts = [], [], []
        for c in range(n):
            ln = rng.choice((0, 1, 150, 900, 4097, max_msg, max_msg))
            text = (c + r) % 3 != 0
            m = TC.json_message(ln, 31 * c + r % 3) if text else TC.random_message(ln, 17 * c + r)
            idle = rng.randrange(7) == 0
            msgs.append(m)
            ops.append(0 if idle else 1 if text else 2)
            opts.append(0 if rng.randrange(5) == 0 else 1)
        tpos, rpos = tx.pos.clone(), rx.pos.clone()
        s = tx.send(pmd.Batch.from_host(msgs), ops, opts, keys=keys)
        got = rx.recv(s.wire, out_cap)
        torch.cuda.synchronize()
        assert s.status.cpu().tolist() == [0] * n and got.status.cpu().tolist() == [0] * n
        comp = s.compressed.cpu().tolist()
        assert comp == [int(ops[c] != 0 and opts[c] and len(msgs[c]) >= 200) for c in range(n)]
        assert got.to_host() == [None if ops[c] == 0 else msgs[c] for c in range(n)], r
        plain += sum(1 for c in range(n) if ops[c] and not comp[c])
        tx_slid += int((tx.pos < tpos).sum())
        rx_slid += int((rx.pos < rpos).sum())
    assert tx_slid >= 10 and rx_slid >= 10 and plain >= n, (tx_slid, rx_slid, plain)


def test_equals_the_host_chain():
    """what TakeoverDeflater.deflate and then frame_batch produce for
    messages that are all compressed, round by round through slides"""
    torch, pmd = _pmd()
    rng = random.Random(8)
    n, max_msg = 40, TC.MAX_MSG
    tx = pmd.TakeoverSender(n, SERVER, level=6, max_msg=max_msg)
    td = pmd.TakeoverDeflater(n, level=6, max_msg=max_msg)
    assert tx.slot == td.slot and tx.HIST == td.HIST
    slid = 0
    for r in range(7):
        msgs = [TC.json_message(rng.choice(TC.LENS + TC.LONG), 13 * c + r) for c in range(n)]
        src = pmd.Batch.from_host(msgs)
        before = td.pos.clone()
        z = td.deflate(src)
        want = pmd.frame_batch(z.out, 4096, op=1, compressed=True)
        s = tx.send(src, 1)
        torch.cuda.synchronize()
        assert s.status.cpu().tolist() == [0] * n and z.status.cpu().tolist() == [0] * n
        assert s.wire.to_host() == want.to_host(), r
        assert s.deflated.out.to_host() == z.out.to_host(), r
        assert tx.pos.cpu().tolist() == td.pos.cpu().tolist()
        assert torch.equal(tx.buf, td.buf)
        slid += int((td.pos < before).sum())
    assert slid >= 10, slid


def test_the_call_does_not_wait():
    """With every buffer given the chained call returns while device copies
    queued before it are still running, also with messages over 4 KiB in the
    batch; bpmd_deflate_takeover_batch on the same inputs waits for its chunk
    count (the event method of tests/test_gpu_async.py)."""
    from tests.test_gpu_async import _call_behind_copies, _setup
    torch, pmd, dev, big, big2 = _setup()
    n, max_msg = 2048, 16384
    some = [TC.json_message((1024, 16384, 5000)[c % 3], c) for c in range(48)]
    src = pmd.Batch.from_host([some[c % 48] for c in range(n)])
    op = torch.full((n,), 2, dtype=torch.uint8, device=dev)   # on the device already: no copy that waits
    tx = pmd.TakeoverSender(n, SERVER, level=6, max_msg=max_msg)
    wire = torch.empty(n * tx.wire_bound + 16, dtype=torch.uint8, device=dev)
    for _ in range(2):   # the stream's pools reach this batch's size
        s = tx.send(src, op, wire=wire)
    torch.cuda.synchronize()
    assert int((s.status != 0).sum()) == 0
    last = []
    assert not _call_behind_copies(torch, lambda: last.append(tx.send(src, op, wire=wire)), big, big2), \
        "the call waited for the queued copies"
    assert int((last[0].status != 0).sum()) == 0 and int((last[0].wire.len == 0).sum()) == 0
    # the host chain's deflate step on the same messages, every buffer given
    cfg = pmd._Cfg(6, 15, 4, 0, 0)
    ln = src.len
    hist = torch.zeros(n, dtype=torch.int32, device=dev)
    cap = torch.full((n,), SM.upper_bound(max_msg), dtype=torch.int32, device=dev)
    off = pmd.slot_offsets(cap)
    out = torch.empty(n * (SM.upper_bound(max_msg) + 16), dtype=torch.uint8, device=dev)
    out_len, status = torch.empty_like(ln), torch.empty_like(ln)

    def chain():
        pmd._check(pmd.lib().bpmd_deflate_takeover_batch(
            ctypes.byref(cfg), pmd._ptr(src.data), pmd._ptr(src.off), pmd._ptr(ln), pmd._ptr(hist), n, pmd._ptr(out),
            pmd._ptr(off), pmd._ptr(cap), pmd._ptr(out_len), pmd._ptr(status), pmd._stream_handle(None)),
            "bpmd_deflate_takeover_batch")

    chain()
    torch.cuda.synchronize()
    assert _call_behind_copies(torch, chain, big, big2), "the takeover deflater returned before the queued copies ran"
