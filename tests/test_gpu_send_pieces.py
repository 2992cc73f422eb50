"""bpmd_send_pieces_batch and pmd.PieceSender on the GPU: messages handed over
in write_some pieces, one piece per connection per call, against
tests/send_pieces_model.py connection by connection.

The connections' buffers, the staging slots and the wire are filled with a
canary, carry guard bytes and stay on the device from call to call; after
every call every output array, d_pos, d_state, the whole d_buf and the whole
wire buffer equal what the model gives, a staging slot holds the model's
payload (the marker behind a non-final piece's) and no staging byte outside a
slot's capacity is touched."""
import ctypes
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import send_model as SM
from tests import send_pieces_model as PM
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
                 frame_max=4096, no_takeover=None, seed=1):
        torch, pmd = _pmd()
        self.n, self.slot, self.role, self.level, self.wbits = n, slot, role, level, wbits
        self.max_len, self.threshold, self.frag, self.frame_max = max_len, threshold, frag, frame_max
        self.L = pmd._send_pc_lib()
        self.cfg = pmd._Cfg(level, wbits, 4, 0, 0)
        dev = "cuda"
        self.h_base = GUARD + slot * np.arange(n, dtype=np.int64)           # packed end to start
        self.h_buf = np.full(2 * GUARD + n * slot, CANARY, dtype=np.uint8)
        self.h_pos = [0] * n
        self.h_state = [PM.ZERO] * n
        self.nt = [0] * n if no_takeover is None else list(no_takeover)
        self.z_max = z_max
        self.h_z_off = GUARD + (z_max + GUARD) * np.arange(n, dtype=np.int64)
        self.z_bytes = GUARD + n * (z_max + GUARD)
        self.wire_max = wire_max
        self.h_wire = np.full(wire_max + GUARD, CANARY, dtype=np.uint8)
        self.d_buf = torch.from_numpy(self.h_buf.copy()).to(dev)
        self.d_base = torch.from_numpy(self.h_base).to(dev)
        self.d_pos = torch.zeros(n, dtype=torch.int32, device=dev)
        self.d_state = pmd.wr_state(n, dev)
        self.d_nt = None if no_takeover is None else torch.tensor(self.nt, dtype=torch.uint8, device=dev)
        self.d_z = torch.full((self.z_bytes,), CANARY, dtype=torch.uint8, device=dev)
        self.d_z_off = torch.from_numpy(self.h_z_off).to(dev)
        self.d_wire = torch.from_numpy(self.h_wire.copy()).to(dev)
        self.d_work = torch.empty(max(int(self.L.bpmd_send_pieces_work_bytes(n)), 1), dtype=torch.uint8, device=dev)
        # keys per piece: frame f of connection i's piece takes keys[i * stride + f]
        self.stride = PM.piece_frame_bound(max(z_max, 1), frame_max, True, True, False)
        rng = random.Random(seed)
        self.keys = [rng.getrandbits(32) for _ in range(n * self.stride)] if role == CLIENT else None
        self.d_keys = pmd._keys(self.keys, n * self.stride, dev) if role == CLIENT else None
        self.d_key_base = (torch.arange(n, dtype=torch.int32, device=dev) * self.stride) if role == CLIENT else None
        self.z_in = np.zeros(self.z_bytes, dtype=bool)
        # per connection: the open message's (plaintext, gathered payload, wire), and every message sent:
        # (plaintext, compressed, gathered payload from the device's staging bytes, wire, opcode)
        self.open = [[b"", b"", b""] for _ in range(n)]
        self.msgs = [[] for _ in range(n)]
        self.pieces = [[] for _ in range(n)]     # every piece that went out: its wire bytes
        self.slides = self.mid_slides = self.markers = self.resets = 0
        self.kinds = []                          # per call: the kinds of entry it held

    def conn_keys(self, i):
        return None if self.keys is None else self.keys[i * self.stride:(i + 1) * self.stride]

    def call(self, pieces, ops, fins, opts=None, z_caps=None, wire_cap=None, align=16, dry=False, fin_ptr=True):
        """One bpmd_send_pieces_batch call, checked against the model.  Returns
        the model's entries and their packing [(off, len, status, pos, state)]."""
        torch, pmd = _pmd()
        n, dev = self.n, "cuda"
        assert len(pieces) == len(ops) == len(fins) == n
        opts = [1] * n if opts is None else opts
        z_caps = [self.z_max] * n if z_caps is None else z_caps
        wire_cap = self.wire_max if wire_cap is None else wire_cap
        assert max(z_caps) <= self.z_max and wire_cap <= self.wire_max
        # ---- the model, on a copy of this record
        bufs = [bytearray(self.h_buf[int(b):int(b) + self.slot].tobytes()) for b in self.h_base]
        ents = [PM.send(self.h_pos[i], self.h_state[i], bufs[i], pieces[i], ops[i], opts[i], fins[i], self.nt[i],
                        self.threshold, self.max_len, self.slot, z_caps[i], self.conn_keys(i), self.level, self.wbits,
                        self.frame_max, self.frag) for i in range(n)]
        packed, total = PM.pack(ents, self.h_state, wire_cap)
        if dry:
            return ents, packed
        # ---- the call
        self.prev_z = self.d_z.cpu().numpy()
        src = pmd.Batch.from_host(pieces, align=align)
        t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)  # noqa: E731
        d_op, d_opt, d_z_cap = t(ops, torch.uint8), t(opts, torch.uint8), t(z_caps, torch.int32)
        d_fin = t([int(bool(f)) for f in fins], torch.uint8) if fin_ptr else None
        assert fin_ptr or all(fins)
        fill = lambda dt, m=n: torch.full((m,), 0x5A, dtype=dt, device=dev)  # noqa: E731
        z_len, w_off, w_len = fill(torch.int32), fill(torch.int64), fill(torch.int32)
        comp, status, tot = fill(torch.uint8), fill(torch.int32), fill(torch.int64, 1)
        pmd._check(self.L.bpmd_send_pieces_batch(
            ctypes.byref(self.cfg), pmd._ptr(src.data), pmd._ptr(src.off), pmd._ptr(src.len), n, self.role,
            self.threshold, int(self.frag), self.frame_max, self.max_len, pmd._ptr(d_op), pmd._ptr(d_opt),
            pmd._optr(d_fin), pmd._optr(self.d_nt), pmd._ptr(self.d_state), pmd._ptr(self.d_buf), pmd._ptr(self.d_base),
            self.slot, pmd._ptr(self.d_pos), pmd._ptr(self.d_z), pmd._ptr(self.d_z_off), pmd._ptr(d_z_cap),
            pmd._ptr(z_len), pmd._optr(self.d_keys), pmd._optr(self.d_key_base), pmd._ptr(self.d_wire), wire_cap,
            pmd._ptr(w_off), pmd._ptr(w_len), pmd._ptr(comp), pmd._ptr(status), pmd._ptr(tot), pmd._ptr(self.d_work),
            pmd._stream_handle(None)), "bpmd_send_pieces_batch")
        torch.cuda.synchronize()
        got_zl, got_z = z_len.cpu().tolist(), self.d_z.cpu().numpy()
        self.last_z, self.last_zl = got_z, got_zl
        # ---- this record after the call
        z_in = self.z_in       # bytes inside a staging slot's capacity in this call or an earlier one
        kinds = set()
        for i, (e, (off, ln, st, pos, state)) in enumerate(zip(ents, packed)):
            b = int(self.h_base[i])
            self.h_buf[b:b + self.slot] = np.frombuffer(bytes(bufs[i]), dtype=np.uint8)
            cont = self.h_state[i][0]
            self.h_pos[i], self.h_state[i] = pos, state
            if ln:
                self.h_wire[off:off + ln] = np.frombuffer(e.wire, dtype=np.uint8)
            z_in[int(self.h_z_off[i]):int(self.h_z_off[i]) + z_caps[i]] = True
            self.slides += e.slid
            self.mid_slides += e.slid and cont
            if ops[i] == 0:
                kinds.add("idle")
            if st != 0 or ops[i] == 0:
                continue
            kinds.add(("middle", "final", "first", "whole")[2 * (not cont) + bool(fins[i])])
            self.markers += e.marked
            self.resets += bool(fins[i] and e.compressed and self.nt[i])
            o = int(self.h_z_off[i])
            m = self.open[i]
            m[0] += bytes(pieces[i])
            m[1] += got_z[o:o + got_zl[i]].tobytes() if e.compressed else b""
            m[2] += e.wire
            self.pieces[i].append(e.wire)
            if fins[i]:
                self.msgs[i].append((m[0], e.compressed, m[1], m[2], state[2]))
                self.open[i] = [b"", b"", b""]
        self.kinds.append(kinds)
        # ---- every output
        assert comp.cpu().tolist() == [e.compressed for e in ents]
        assert status.cpu().tolist() == [p[2] for p in packed]
        assert w_off.cpu().tolist() == [p[0] for p in packed]
        assert w_len.cpu().tolist() == [p[1] for p in packed]
        assert tot.cpu().tolist() == [total]
        assert self.d_pos.cpu().tolist() == self.h_pos
        assert [tuple(s[:3]) for s in self.d_state.cpu().tolist()] == self.h_state
        assert int(self.d_state[:, 3].sum()) == 0
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
        """Beast's receiving end on the gathered payloads (the device's staging
        bytes, piece after piece): one inflater kept per takeover connection,
        a fresh one per message under no_context_takeover"""
        for c, sent in enumerate(self.msgs):
            z = [(m, p) for m, comp, p, _, _ in sent if comp]
            if self.nt[c]:
                got = [O.pmd_inflate(p, cap=cap, wbits=self.wbits) for _, p in z]
            else:
                got = O.pmd_inflate_stream([p for _, p in z], cap=cap, wbits=self.wbits)
            assert got == [(0, m) for m, _ in z], c


def _script(rng, c, n_msgs, lens, max_pieces=4):
    """One connection's pieces in sending order: [(piece, op, opt, fin)], the
    continuation pieces with the other data opcode and a random opt, which the
    call must ignore"""
    out = []
    for k in range(n_msgs):
        np_ = rng.randrange(1, max_pieces + 1)
        op, opt = 1 + (c + k) % 2, 0 if rng.randrange(5) == 0 else 1
        size = max(lens) * max_pieces + 1
        text = TC.json_message(size, 97 * c + k) if (c + k) % 3 else TC.random_message(size, 97 * c + k)
        at = 0
        for j in range(np_):
            ln = rng.choice(lens)
            if j == np_ - 1 and j > 0 and rng.randrange(3) == 0:
                ln = 0     # write_some(true, {}) after the data
            out.append((text[at:at + ln], op if j == 0 else 3 - op, opt if j == 0 else rng.randrange(2), j == np_ - 1))
            at += ln
    return out


@pytest.mark.parametrize("role,frame_max,frag,level", [(SERVER, 7, True, 6), (CLIENT, 125, False, 1),
                                                       (SERVER, 126, True, 9), (CLIENT, 4096, True, 6)])
def test_connections_out_of_step(role, frame_max, frag, level):
    """idle, first, middle and final pieces in one call; the marker across a
    frame cut and the 2/4-byte header-length edge; a slot of 2K + 4097, so
    buffers slide in the middle of messages; a third of the connections under
    no_context_takeover"""
    rng = random.Random(frame_max + role)
    n, thr = 24, 301
    slot = 2 * K + 4097
    L = TM.room(1 << 16, slot)
    assert L == 4097
    lens = (0, 1, thr - 1, thr, 4095, 4097)
    nt = [int(c % 3 == 2) for c in range(n)]
    rig = Rig(n, slot, SM.upper_bound(L) + 4, n * (SM.upper_bound(L) + 4 + 6 * 700), role, level, 15, max_len=1 << 16,
              threshold=thr, frag=frag, frame_max=frame_max, no_takeover=nt)
    scripts = [_script(rng, c, 3, lens) for c in range(n)]
    for c in (0, 1, 3, 4):    # takeover connections: 3 * L > slot - L, so the third piece of four slides
        text = TC.json_message(4 * L, 7 + c)
        scripts[c][0:0] = [(text[j * L:(j + 1) * L], 2, 1, j == 3) for j in range(4)]
    turn = [0] * n
    r = 0
    while any(turn[c] < len(scripts[c]) for c in range(n)):
        batch, ops, opts, fins = [], [], [], []
        for c in range(n):
            if turn[c] < len(scripts[c]) and rng.randrange(5):
                p, op, opt, fin = scripts[c][turn[c]]
                turn[c] += 1
            else:   # idle, whatever its entry holds
                p, op, opt, fin = b"idle" * rng.randrange(3), 0, rng.randrange(2), rng.randrange(2)
            batch.append(p), ops.append(op), opts.append(opt), fins.append(fin)
        rig.call(batch, ops, fins, opts, align=(16, 1)[r % 2])
        r += 1
    assert [len(m) for m in rig.msgs] == [4 if c in (0, 1, 3, 4) else 3 for c in range(n)]
    assert any(k >= {"idle", "first", "middle", "final"} for k in rig.kinds), rig.kinds
    assert rig.markers >= n and rig.mid_slides >= 3 and rig.resets >= 4, (rig.markers, rig.mid_slides, rig.resets)
    plain = sum(1 for s in rig.msgs for m in s if not m[1])
    assert plain >= n // 4, plain
    rig.peer_decodes(4 * L)


def test_marker_room_wire_cut_and_resend():
    """A middle piece whose staging slot has exactly 3 bytes beyond the
    deflater's length is refused and none of the marker's bytes is written,
    one with exactly 4 goes out; a wire that cuts a middle piece off; a piece
    longer than L; a bad opcode.  Every refused connection keeps its state and
    position, sends the same piece again with room (a shorter one after
    message_too_big) and ends up where the uncut run does, wire byte for wire
    byte."""
    n = 8
    slot = 2 * K + 4097
    L = 4097
    text = [TC.json_message(3 * L, 500 + i) for i in range(n)]
    first = [t[:1500] for t in text]
    mid = [t[1500:3500] for t in text]
    last = [t[3500:3900] for t in text]
    zmax = SM.upper_bound(L + 1) + 4

    def rig():
        return Rig(n, slot, zmax, n * 5000, SERVER, 6, 15, max_len=1 << 16, threshold=0, frame_max=125)

    a = rig()      # the uncut run
    a.call(first, [1] * n, [0] * n)
    a.call(mid, [1] * n, [0] * n)
    a.call(last, [1] * n, [1] * n)
    b = rig()
    b.call(first, [1] * n, [0] * n)
    ents, packed = b.call(mid, [2] * n, [0] * n, dry=True)
    assert [e.status for e in ents] == [0] * n and all(e.marked for e in ents)
    zl = [len(e.payload) - 4 for e in ents]           # the deflater's lengths
    assert all(e.need <= z + 1 for e, z in zip(ents, zl))
    pieces, ops = list(mid), [2] * n
    pieces[1], ops[4] = text[1][1500:1500 + L + 1], 3
    z_caps = [zmax] * n
    z_caps[2], z_caps[3] = zl[2] + 3, zl[3] + 4
    # the wire ends one byte before entry 6's last (entries 1, 2 and 4 take no room)
    ents, packed = b.call(pieces, ops, [0] * n, z_caps=z_caps, dry=True)
    wire_cap = packed[6][0] + len(ents[6].wire) - 1
    pos0, state0 = list(b.h_pos), list(b.h_state)
    ents, packed = b.call(pieces, ops, [0] * n, z_caps=z_caps, wire_cap=wire_cap)
    st = [p[2] for p in packed]
    assert st == [0, TM.MESSAGE_TOO_BIG, SM.NEED_BUFFERS, 0, SM.BAD_OPCODE, 0, SM.BUFFER_OVERFLOW, SM.BUFFER_OVERFLOW]
    # entry 2: the deflater's length and bytes, and behind what it asked for nothing has changed
    o = int(b.h_z_off[2])
    assert b.last_zl[2] == zl[2] and b.last_z[o:o + zl[2]].tobytes() == ents[2].payload
    assert np.array_equal(b.last_z[o + ents[2].need:o + zmax], b.prev_z[o + ents[2].need:o + zmax])
    o = int(b.h_z_off[3])
    assert b.last_zl[3] == zl[3] + 4 and b.last_z[o + zl[3]:o + zl[3] + 4].tobytes() == PM.MARKER
    assert np.array_equal(b.last_z[o + zl[3] + 4:o + zmax], b.prev_z[o + zl[3] + 4:o + zmax])
    again = [i for i in range(n) if st[i]]
    assert again == [1, 2, 4, 6, 7]
    for i in again:           # no slide in this call, so not even that
        assert b.h_pos[i] == pos0[i] and b.h_state[i] == state0[i] == (1, 1, 1), i
    for i in (0, 3, 5):
        assert b.h_pos[i] == pos0[i] + 2000 and b.h_state[i] == (1, 1, 1)
    # ---- the same pieces again, with room; the others idle
    b.call(mid, [1 if i in again else 0 for i in range(n)], [0] * n)
    b.call(last, [1] * n, [1] * n)
    assert b.h_pos == a.h_pos and b.h_state == a.h_state == [(0, 1, 1)] * n
    assert b.pieces == a.pieces and [m[:4] for s in b.msgs for m in s] == [m[:4] for s in a.msgs for m in s]
    b.peer_decodes(3 * L)


def test_threshold_is_decided_at_the_first_piece_only():
    """a short first piece followed by long ones stays uncompressed: RSV1
    never set, the history and d_pos untouched (the rig compares the whole
    d_buf); a long first piece followed by short ones stays compressed"""
    n, thr = 8, 400
    slot = 2 * K + 4097
    rig = Rig(n, slot, SM.upper_bound(4097) + 4, n * 4400, CLIENT, 6, 15, threshold=thr, frame_max=4096)
    short = [c % 2 == 0 for c in range(n)]
    text = [TC.json_message(9000, 40 + c) for c in range(n)]
    plan = [((10, 4000, 4097, 0) if s else (thr, 3, thr - 1, 1)) for s in short]
    at = [0] * n
    for j in range(4):
        batch = []
        for c in range(n):
            batch.append(text[c][at[c]:at[c] + plan[c][j]])
            at[c] += plan[c][j]
        ents, packed = rig.call(batch, [1] * n, [j == 3] * n)
        assert [e.compressed for e in ents] == [int(not s) for s in short]
        for c, e in enumerate(ents):
            assert bool(e.wire[0] & 0x40) == (j == 0 and not short[c]) and e.wire[0] & 15 == (1 if j == 0 else 0)
    assert rig.h_pos == [0 if s else sum(plan[c]) for c, s in enumerate(short)]
    rig.peer_decodes(9000)


def test_no_takeover_resets_after_the_final_piece_and_not_before():
    n = 6
    slot = 2 * K + 4097
    nt = [1, 0, 1, 0, 1, 1]
    rig = Rig(n, slot, SM.upper_bound(4097) + 4, n * 4400, SERVER, 6, 15, no_takeover=nt)
    text = [TC.json_message(6000, 80 + c) for c in range(n)]
    for k in range(2):     # two messages each: the second starts without history where the first was reset
        rig.call([t[:1000] for t in text], [1] * n, [0] * n)
        assert rig.h_pos == [1000 if f else 2200 * k + 1000 for f in nt]
        rig.call([t[1000:2000] for t in text], [1] * n, [0] * n, opts=[0] * n)
        assert rig.h_pos == [2000 if f else 2200 * k + 2000 for f in nt]
        # entry 4's final piece does not reach the wire: no reset yet
        ents, packed = rig.call([t[2000:2200] for t in text], [1] * n, [1] * n, dry=True)
        rig.call([t[2000:2200] for t in text], [1] * n, [1] * n, wire_cap=packed[4][0] + 1)
        assert rig.h_pos == [0, 2200 * (k + 1), 0, 2200 * (k + 1), 2000, 2000]
        assert rig.h_state[4] == rig.h_state[5] == (1, 1, 1)
        rig.call([t[2000:2200] for t in text], [0, 0, 0, 0, 1, 1], [1] * n)
        assert rig.h_pos == [0 if f else 2200 * (k + 1) for f in nt] and rig.h_state == [(0, 1, 1)] * n
    assert rig.resets == 8
    rig.peer_decodes(6000)


def test_grid_stride_over_many_tiny_pieces():
    """9 000 entries: more than the one-wave-per-entry kernels launch waves"""
    rng = random.Random(12)
    n = 9000
    slot = 2 * K + 48
    rig = Rig(n, slot, 96 + 4, n * 72, SERVER, 1, 15, max_len=48, threshold=8, no_takeover=[c % 2 for c in range(n)])
    words = [b"alpha ", b"beta ", b"gamma ", b"delta ", b"{\"id\": 7}", b"\x00\x01\x02"]
    fins = [rng.randrange(2) for _ in range(n)]
    for r in range(2):
        pieces = [b"".join(rng.choice(words) for _ in range(rng.randrange(7)))[:48] for _ in range(n)]
        rig.call(pieces, [rng.choice((0, 1, 2, 2)) for _ in range(n)], fins if r == 0 else [1] * n,
                 [rng.randrange(4) != 0 for _ in range(n)], align=1)
    assert rig.markers >= n // 8 and rig.resets >= n // 8, (rig.markers, rig.resets)


def test_whole_messages_equal_the_takeover_call():
    """every piece final, zeroed state, no resets: wire, staging, statuses and
    d_pos equal bpmd_send_takeover_batch's byte for byte, call after call
    through slides, with refused and idle entries among them; d_fin and
    d_no_takeover NULL"""
    torch, pmd = _pmd()
    rng = random.Random(8)
    n, max_msg = 40, TC.MAX_MSG
    tk = pmd.TakeoverSender(n, CLIENT, level=6, max_msg=max_msg, threshold=301, frame_max=1500)
    pc = pmd.PieceSender(n, CLIENT, level=6, max_piece=max_msg, threshold=301, frame_max=1500)
    assert tk.slot == pc.slot and tk.key_stride <= pc.key_stride
    keys = torch.randint(-2 ** 31, 2 ** 31 - 1, (n * pc.key_stride,), dtype=torch.int32, device="cuda")
    pc.key_base = tk.key_base     # the same keys for the same frames
    slid = 0
    for r in range(7):
        lens = [rng.choice(TC.LENS + TC.LONG + (max_msg + 1,)) for _ in range(n)]
        msgs = [TC.json_message(ln, 13 * c + r) for c, ln in enumerate(lens)]
        ops = [rng.choice((0, 1, 2, 2, 2, 3)) for _ in range(n)]
        opts = [rng.randrange(5) != 0 for _ in range(n)]
        src = pmd.Batch.from_host(msgs)
        wire = torch.full((2, n * tk.wire_bound + 16), CANARY, dtype=torch.uint8, device="cuda")
        before = tk.pos.clone()
        a = tk.send(src, ops, opts, keys=keys, wire=wire[0])
        b = pc.send(src, ops, None, opts, keys=keys, wire=wire[1])
        torch.cuda.synchronize()
        st = a.status.cpu().tolist()
        assert b.status.cpu().tolist() == st and {0, TM.MESSAGE_TOO_BIG, SM.BAD_OPCODE} >= set(st)
        assert torch.equal(a.compressed, b.compressed) and torch.equal(a.total, b.total)
        assert torch.equal(a.wire.off, b.wire.off) and torch.equal(a.wire.len, b.wire.len)
        assert torch.equal(wire[0], wire[1]), r
        assert torch.equal(tk.pos, pc.pos) and torch.equal(tk.buf, pc.buf)
        ok = (a.status == 0) & (a.compressed != 0)
        assert torch.equal(a.deflated.out.len[ok], b.deflated.out.len[ok])
        za, zb = a.deflated.out.to_host(), b.deflated.out.to_host()
        assert [z for z, k in zip(za, ok.cpu().tolist()) if k] == [z for z, k in zip(zb, ok.cpu().tolist()) if k]
        assert int(pc.state[:, 0].sum()) == 0      # no message left open
        slid += int((tk.pos < before).sum())
    assert slid >= 10, slid


@pytest.mark.parametrize("sender_role", [CLIENT, SERVER])
def test_round_trip_through_the_receivers(sender_role):
    """pmd.PieceSender -> a message's per-call wire gathered -> on takeover
    connections pmd.TakeoverReceiver, under no_context_takeover
    pmd.recv_batch: every message arrives as it was sent, several per
    connection so later ones copy from earlier ones, among them messages of
    3 * L bytes in pieces of at most L and uncompressed ones"""
    torch, pmd = _pmd()
    rng = random.Random(90 + sender_role)
    n, L, wbits, n_msgs = 16, 3000, 12, 4
    nt = [int(c >= n // 2) for c in range(n)]
    tx = pmd.PieceSender(n, sender_role, level=6, window_bits=wbits, max_piece=L, threshold=200, frame_max=1500,
                         no_takeover=nt)
    assert tx.slot - 2 * K < L + 16
    peer = CLIENT if sender_role == SERVER else SERVER
    rx = pmd.TakeoverReceiver(n // 2, peer, window_bits=wbits, max_msg=3 * L)
    keys = None
    if sender_role == CLIENT:
        keys = torch.randint(-2 ** 31, 2 ** 31 - 1, (n * tx.key_stride,), dtype=torch.int32, device="cuda")
    # per connection: messages, each a list of pieces; the first of every connection is 3 * L bytes long
    scripts, want = [], []
    for c in range(n):
        conn, msgs = [], []
        for k in range(n_msgs):
            ln = 3 * L if k == 0 else rng.choice((0, 150, 900, L, 2 * L + 1))
            text = (c + k) % 3 != 0
            m = TC.json_message(ln, 31 * c + k % 2) if text else TC.random_message(ln, 17 * c + k)
            if k == 0 or rng.randrange(2) == 0:
                cuts = [m[a:a + L] for a in range(0, ln, L)] or [m]
            else:   # thirds, an empty piece among them
                t = ln // 3
                cuts = [m[:t], b"", m[t:2 * t], m[2 * t:]]
            assert b"".join(cuts) == m and max(map(len, cuts)) <= L
            if rng.randrange(2):
                cuts.append(b"")
            op, opt = 1 if text else 2, 0 if (c + k) % 4 == 0 else 1
            conn += [(p, op, opt, j + 1 == len(cuts)) for j, p in enumerate(cuts)]
            msgs.append((m, op, int(opt and len(cuts[0]) >= 200)))
        scripts.append(conn)
        want.append(msgs)
    turn, gathered, open_ = [0] * n, [[] for _ in range(n)], [b""] * n
    tx_slid = 0
    while any(turn[c] < len(scripts[c]) for c in range(n)):
        batch, ops, opts, fins = [], [], [], []
        for c in range(n):
            if turn[c] < len(scripts[c]) and rng.randrange(6):
                p, op, opt, fin = scripts[c][turn[c]]
                turn[c] += 1
            else:
                p, op, opt, fin = b"", 0, 1, 1
            batch.append(p), ops.append(op), opts.append(opt), fins.append(fin)
        before = tx.pos.clone()
        s = tx.send(pmd.Batch.from_host(batch), ops, fins, opts, keys=keys)
        torch.cuda.synchronize()
        assert s.status.cpu().tolist() == [0] * n
        tx_slid += int(((tx.pos < before) & (tx.pos != 0)).sum())
        for c, w in enumerate(s.wire.to_host()):
            if ops[c]:
                open_[c] += w
                if fins[c]:
                    gathered[c].append(open_[c])
                    open_[c] = b""
    assert [len(g) for g in gathered] == [n_msgs] * n and tx_slid >= 4, tx_slid
    out_cap = SM.upper_bound(3 * L) + 64
    plain = 0
    for k in range(n_msgs):
        half = n // 2
        got = rx.recv(pmd.Batch.from_host([gathered[c][k] for c in range(half)]), out_cap)
        got_nt = pmd.recv_batch(pmd.Batch.from_host([gathered[c][k] for c in range(half, n)]), out_cap, 3 * L, peer,
                                window_bits=wbits)
        torch.cuda.synchronize()
        assert got.status.cpu().tolist() == [0] * half and got_nt.status.cpu().tolist() == [0] * half
        comp = got.frames.compressed.cpu().tolist() + got_nt.frames.compressed.cpu().tolist()
        assert comp == [want[c][k][2] for c in range(n)]
        assert got.frames.op.cpu().tolist() + got_nt.frames.op.cpu().tolist() == [want[c][k][1] for c in range(n)]
        assert got.to_host() + got_nt.to_host() == [want[c][k][0] for c in range(n)], k
        plain += comp.count(0)
    assert plain >= n // 2, plain


def test_the_call_does_not_wait():
    """With `wire` given PieceSender.send returns while device copies queued
    before it are still running, also with pieces over 4 KiB in the batch (the
    event method of tests/test_gpu_async.py)."""
    from tests.test_gpu_async import _call_behind_copies, _setup
    torch, pmd, dev, big, big2 = _setup()
    n, max_piece = 2048, 16384
    some = [TC.json_message((1024, 16384, 5000)[c % 3], c) for c in range(48)]
    src = pmd.Batch.from_host([some[c % 48] for c in range(n)])
    op = torch.full((n,), 2, dtype=torch.uint8, device=dev)   # on the device already: no copy that waits
    fin = torch.zeros(n, dtype=torch.uint8, device=dev)
    tx = pmd.PieceSender(n, SERVER, level=6, max_piece=max_piece,
                         no_takeover=torch.ones(n, dtype=torch.uint8, device=dev))
    wire = torch.empty(n * tx.wire_bound + 16, dtype=torch.uint8, device=dev)
    for _ in range(2):   # the stream's pools reach this batch's size
        s = tx.send(src, op, fin, wire=wire)
    torch.cuda.synchronize()
    assert int((s.status != 0).sum()) == 0
    last = []
    assert not _call_behind_copies(torch, lambda: last.append(tx.send(src, op, fin, wire=wire)), big, big2), \
        "the call waited for the queued copies"
    assert int((last[0].status != 0).sum()) == 0 and int((last[0].wire.len == 0).sum()) == 0
    assert int(tx.state[:, 0].sum()) == n
