"""bpmd_receive_pieces_batch and pmd.PieceReceiver on the GPU: messages handed
over in pieces, one piece per connection per call, against
tests/receive_pieces_model.py connection by connection -- the walk in Python,
the oracle's inflate_stream with one write(Flush::sync) per piece and the
oracle's streaming utf8_checker, so the expected bytes are Beast's own.

The gathered slots, the message slots and the inflater states stay on the
device from call to call; the slots are filled with a canary and carry guard
bytes.  After every call every output array, the whole d_state, the whole
d_out, d_msg (d_msg_len bytes compared, the rest of the inflater's room free,
everything else unchanged), the control slots and all guards equal the model.

The toy-sized cases are built here; the long ones (16 KiB messages in read
buffer pieces, a window that wraps many times, one piece over the inflater's
staging and ring, UTF-8 across the scan's 1 KiB rounds) come from
tests/receive_pieces_cases.py, which the CPU suite runs through the model
alone (tests/test_receive_pieces_cases.py)."""
import ctypes
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import frame_parse_model as FM
from tests import receive_pieces_cases as C
from tests import receive_pieces_model as M
from tests import takeover_cases as TC
from tests.receive_pieces_cases import drive, events

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 64
SERVER, CLIENT = FM.SERVER, FM.CLIENT


def _pmd():
    import torch
    from beast_amd import pmd
    return torch, pmd


def _layout(caps, residues):
    """slot offsets at the given residues mod 16, GUARD bytes apart at least; (offsets, total bytes)"""
    off, at = [], 0
    for c, r in zip(caps, residues):
        o = (at + GUARD + 15) // 16 * 16 + r
        off.append(o)
        at = o + c
    return np.array(off, dtype=np.int64), at + GUARD + 16


class Rig:
    """n connections' device state and the model's record of it"""

    def __init__(self, n, role, wbits=15, pmd_on=True, msg_max=0, out_cap=64, msg_cap=4096, out_res=None, wire_res=None,
                 msg_res=None):
        torch, pmd = _pmd()
        self.n, self.role, self.pmd_on, self.msg_max = n, role, pmd_on, msg_max
        self.L = pmd._recv_pc_lib()
        self.cfg = pmd._Cfg(0, wbits, 8, 0, 0)
        dev = "cuda"
        lst = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n  # noqa: E731
        self.out_cap, self.msg_cap = lst(out_cap), lst(msg_cap)
        self.wire_res = lst(wire_res or 0)
        self.h_out_off, out_bytes = _layout(self.out_cap, lst(out_res or 0))
        self.h_msg_off, msg_bytes = _layout(self.msg_cap, lst(msg_res or 0))
        self.h_out = np.full(out_bytes, CANARY, dtype=np.uint8)
        self.h_msg = np.full(msg_bytes, CANARY, dtype=np.uint8)
        self.d_out = torch.from_numpy(self.h_out.copy()).to(dev)
        self.d_msg = torch.from_numpy(self.h_msg.copy()).to(dev) if pmd_on else None
        self.d_out_off = torch.from_numpy(self.h_out_off).to(dev)
        self.d_msg_off = torch.from_numpy(self.h_msg_off).to(dev) if pmd_on else None
        self.d_out_cap = torch.tensor(self.out_cap, dtype=torch.int32, device=dev)
        self.d_state = pmd.rd_piece_state(n, dev)
        self.zb = int(self.L.bpmd_receive_pieces_zstate_bytes())
        self.d_z = self.d_work = None
        if pmd_on:
            self.d_z = torch.zeros(n * self.zb + GUARD, dtype=torch.uint8, device=dev)
            self.d_z[n * self.zb:] = CANARY
            self.d_work = torch.empty(max(int(self.L.bpmd_receive_pieces_work_bytes(n)), 1), dtype=torch.uint8, device=dev)
        self.conns = [M.Conn(role, wbits, pmd_on, msg_max) for _ in range(n)]
        self.dead = [False] * n
        self.calls = 0

    def call(self, wires, msg_cap=None):
        """One bpmd_receive_pieces_batch call checked against the model; returns the model's pieces."""
        torch, pmd = _pmd()
        n, dev = self.n, "cuda"
        assert len(wires) == n
        wires = [b"" if self.dead[i] else bytes(w) for i, w in enumerate(wires)]
        msg_cap = self.msg_cap if msg_cap is None else ([msg_cap] * n if isinstance(msg_cap, int) else list(msg_cap))
        assert all(a <= b for a, b in zip(msg_cap, self.msg_cap))
        # ---- the wire of this call, entry i at residue wire_res[i]
        w_off, total = _layout([len(w) for w in wires], self.wire_res)
        h_wire = np.full(total, CANARY, dtype=np.uint8)
        for o, w in zip(w_off, wires):
            h_wire[o:o + len(w)] = np.frombuffer(w, dtype=np.uint8)
        d_wire = torch.from_numpy(h_wire).to(dev)
        d_w_off = torch.from_numpy(w_off).to(dev)
        d_w_len = torch.tensor([len(w) for w in wires], dtype=torch.int32, device=dev)
        # ---- the model
        ps = [None if self.dead[i] else self.conns[i].call(wires[i], self.out_cap[i], msg_cap[i]) for i in range(n)]
        # ---- the call
        fill = lambda dt, *shape: torch.full(shape or (n,), 0x5A, dtype=dt, device=dev)  # noqa: E731
        out_len, msg_len, status, consumed = fill(torch.int32), fill(torch.int32), fill(torch.int32), fill(torch.int32)
        op, comp, event, ctl_len = fill(torch.uint8), fill(torch.uint8), fill(torch.uint8), fill(torch.uint8)
        code, ctl = fill(torch.int16), torch.full((n, 128), CANARY, dtype=torch.uint8, device=dev)
        d_msg_cap = torch.tensor(msg_cap, dtype=torch.int32, device=dev) if self.pmd_on else None
        on = self.pmd_on
        pmd._check(self.L.bpmd_receive_pieces_batch(
            ctypes.byref(self.cfg) if on else None, self.role, int(on), self.msg_max, pmd._ptr(d_wire), pmd._ptr(d_w_off),
            pmd._ptr(d_w_len), n, pmd._ptr(self.d_state), pmd._optr(self.d_z), pmd._ptr(self.d_out),
            pmd._ptr(self.d_out_off), pmd._ptr(self.d_out_cap), pmd._ptr(out_len), pmd._ptr(op), pmd._ptr(comp),
            pmd._ptr(event), pmd._ptr(status), pmd._ptr(consumed), pmd._ptr(ctl), pmd._ptr(ctl_len), pmd._ptr(code),
            pmd._optr(self.d_msg), pmd._optr(self.d_msg_off), pmd._optr(d_msg_cap), pmd._ptr(msg_len),
            pmd._optr(self.d_work), pmd._stream_handle(None)), "bpmd_receive_pieces_batch")
        torch.cuda.synchronize()
        self.calls += 1
        # ---- every output
        g = {k: v.cpu().tolist() for k, v in dict(out_len=out_len, msg_len=msg_len, status=status, consumed=consumed,
                                                   op=op, comp=comp, event=event, ctl_len=ctl_len).items()}
        g_code = (code.to(torch.int32) & 0xFFFF).cpu().tolist()
        g_ctl, g_state = ctl.cpu().numpy(), self.d_state.cpu().numpy()
        g_out = self.d_out.cpu().numpy()
        g_msg = self.d_msg.cpu().numpy() if on else None
        assert np.array_equal(d_wire.cpu().numpy(), h_wire)
        for i, p in enumerate(ps):
            if p is None:
                continue
            s = p.stop
            got = (g["event"][i], g["status"][i], g["consumed"][i], g["out_len"][i], g["op"][i], g["comp"][i],
                   g["ctl_len"][i], g_code[i], g["msg_len"][i])
            want = (s.event, p.status, s.consumed, p.out_len, s.op, s.compressed, len(s.ctl), s.close_code,
                    len(p.delivered))
            assert got == want, (self.calls, i, got, want)
            assert g_ctl[i, :len(s.ctl)].tobytes() == s.ctl and (g_ctl[i, len(s.ctl):] == CANARY).all(), i
            if p.state is not None:
                assert g_state[i].tobytes() == p.state, (self.calls, i, g_state[i].tobytes().hex(), p.state.hex())
            o = int(self.h_out_off[i])
            self.h_out[o:o + len(p.out)] = np.frombuffer(p.out, dtype=np.uint8)
            assert len(p.out) <= self.out_cap[i]
            if p.ran:
                o = int(self.h_msg_off[i])
                assert len(p.delivered) <= p.eff <= msg_cap[i]
                self.h_msg[o:o + p.eff] = g_msg[o:o + p.eff]            # the inflater's room: free beyond d_msg_len
                self.h_msg[o:o + len(p.delivered)] = np.frombuffer(p.delivered, dtype=np.uint8)
            if p.status:
                self.dead[i] = True
        assert np.array_equal(g_out, self.h_out), (self.calls, np.flatnonzero(g_out != self.h_out)[:8])
        if on:
            assert np.array_equal(g_msg, self.h_msg), (self.calls, np.flatnonzero(g_msg != self.h_msg)[:8])
            assert bool((self.d_z[n * self.zb:] == CANARY).all())
        return ps


def keyed(role, rng):
    return (lambda: rng.getrandbits(32)) if role == SERVER else (lambda: None)


TEXT = ("The quick brown fox jumps over the lazy dog; pack my box with five dozen liquor jugs. "
        "Sphinx of black quartz, judge my vow! How vexingly quick daft zebras jump.").encode()


def test_every_cut():
    """70 connections (more than one wave, more than one block) share one wire
    of about 300 bytes -- a compressed text message in three frames with a ping
    between two of them, a plain binary message, a compressed message with a
    126-form length, a close -- connection j fed j + 1 bytes per call"""
    rng = random.Random(3)
    key = keyed(SERVER, rng)
    text, blob, plain = "grüße, 世界! 😀 ".encode() * 3, rng.randbytes(140), bytes(range(40, 70))
    p1, p2 = O.pmd_deflate_stream([text, blob], 6, 15, 4)
    assert len(p2) >= 126
    a, b = len(p1) // 3, 2 * len(p1) // 3
    w = (FM.frame(p1[:a], 1, False, 4, key()) + FM.frame(p1[a:b], 0, False, 0, key()) + FM.frame(b"hi", 9, True, 0, key()) +
         FM.frame(p1[b:], 0, True, 0, key()) + FM.frame(plain, 2, True, 0, key()) + FM.frame(p2, 2, True, 4, key()) +
         FM.frame(b"\x03\xe8bye", 8, True, 0, key()))
    assert 250 <= len(w) <= 350, len(w)
    n = 70
    rig = Rig(n, SERVER, out_cap=64, msg_cap=512)
    log = drive(rig, [w] * n, [j + 1 for j in range(n)])
    want = [("ping", b"hi"), ("message", 1, 1, text), ("message", 2, 0, plain), ("message", 2, 1, blob),
            ("close", b"\x03\xe8bye")]
    for j in range(n):
        assert events(log[j]) == want, j
    assert len(log[0]) == len(w)          # a byte a call: every call took its byte


@pytest.mark.parametrize("role", [SERVER, CLIENT])
def test_mask_and_alignment(role):
    """a frame cut so that the resumed payload starts at every key phase, the
    wire at every residue mod 16, the out slot at every residue mod 16; plain
    and compressed messages alternate, so the inflater's input starts at every
    residue too.  Server role reads masked frames, client role unmasked ones."""
    rng = random.Random(5 + role)
    key = keyed(role, rng)
    n = 256 if role == SERVER else 32
    plain = rng.randbytes(100)
    zp = O.pmd_deflate(TEXT)
    wires, first = [], []
    for e in range(n):
        comp = e & 1
        w = FM.frame(zp if comp else plain, 2, True, 4 if comp else 0, key())
        hdr = len(w) - len(zp if comp else plain)
        wires.append(w)
        first.append(hdr + 17 + (e >> 1) % 4)          # the second call resumes at phase (17 + e / 2) % 4
    rig = Rig(n, role, out_cap=160, msg_cap=256, out_res=[e % 16 for e in range(n)],
              wire_res=[(e // 16 + e) % 16 for e in range(n)])
    a = rig.call([w[:k] for w, k in zip(wires, first)])
    b = rig.call([w[k:] for w, k in zip(wires, first)])
    for e in range(n):
        assert a[e].stop.consumed == first[e] and a[e].stop.event == FM.EV_NEED_MORE
        assert b[e].stop.event == FM.EV_MESSAGE and b[e].status == 0
        assert a[e].delivered + b[e].delivered == (TEXT if e & 1 else plain), e
    if role == SERVER:
        assert {(p.stop.consumed - 6) % 4 for p in a} == {0, 1, 2, 3}


def test_slot_bound():
    """with d_out_cap = 12 one 100-byte frame is taken 8 bytes a call, plain
    and compressed; d_out_cap = 7 is refused, per entry on the device and by
    pmd.PieceReceiver on the host"""
    torch, pmd = _pmd()
    body, noise = bytes(range(100)), random.Random(1).randbytes(90)
    zgood = O.pmd_deflate(noise)
    wires = [FM.frame(body, 2, True, 0, 0x01020304), FM.frame(zgood, 2, True, 4, 0xA1B2C3D4),
             FM.frame(body, 2, True, 0, 7)]
    rig = Rig(3, SERVER, out_cap=[12, 12, 7], msg_cap=256)
    log = drive(rig, wires, 1000)
    assert [len(p.stop.piece) for p in log[0]] == [8] * 12 + [4]
    assert all(len(p.stop.piece) == 8 for p in log[1][:-1]) and len(log[1]) == (len(zgood) + 7) // 8
    assert events(log[0]) == [("message", 2, 0, body)]
    assert events(log[1]) == [("message", 2, 1, noise)]
    assert events(log[2]) == [("error", M.BUFFER_OVERFLOW)] and log[2][0].stop.consumed == 0
    rx = pmd.PieceReceiver(1, SERVER)
    with pytest.raises(pmd.BpmdError):
        rx.recv(pmd.Batch.from_host([wires[0]]), 7, 256)


def test_mid_symbol_cuts():
    """a 124-byte dynamic-block payload: connection c gets it as two fragments
    cut behind byte c + 1, one fragment per call, so a piece ends at every byte
    of the payload -- inside the block header, a code length, a symbol, extra
    bits; the last connection gets it as one frame a byte at a time"""
    zp = O.pmd_deflate(TEXT)
    assert 100 <= len(zp) <= 140 and (zp[0] >> 1) & 3 == 2
    n = len(zp)
    rng = random.Random(9)
    key = keyed(SERVER, rng)
    frames = [(FM.frame(zp[:c + 1], 1, False, 4, key()), FM.frame(zp[c + 1:], 0, True, 0, key())) for c in range(n - 1)]
    rig = Rig(n, SERVER, out_cap=160, msg_cap=256)
    one = FM.frame(zp, 1, True, 4, key())
    got, pend = [b""] * n, b""
    for k in range(len(one)):
        pend += one[k:k + 1]
        ps = rig.call([f[k] if k < 2 else b"" for f in frames] + [pend])
        pend = pend[ps[-1].stop.consumed:]
        for i, p in enumerate(ps):
            assert p.status == 0, (k, i)
            got[i] += p.delivered
            if i < n - 1 and k < 2:
                assert p.stop.event == (FM.EV_MESSAGE if k == 1 else FM.EV_NEED_MORE)
    assert got == [TEXT] * n and pend == b"" and ps[-1].stop.event == FM.EV_MESSAGE


def test_context_takeover():
    """message 2 copies from message 1 at window bits 15; at window bits 9 a
    distance past the window gives invalid_distance in the piece where the
    oracle reports it for the same calls"""
    rng = random.Random(13)
    first = rng.randbytes(600)
    msgs = [first, first[:80] + b"tail"]
    pays = O.pmd_deflate_stream(msgs, 6, 15, 4)
    assert len(pays[1]) < 30                       # a copy from 600 bytes back, not 84 literals
    w = b"".join(FM.frame(p, 2, True, 4) for p in pays)
    for wbits, step in [(15, 7), (15, 1000), (9, 7), (9, 1000)]:
        rig = Rig(2, CLIENT, wbits=wbits, out_cap=64, msg_cap=1024)
        ev = events(drive(rig, [w, w], [step, step + 1])[0])
        if wbits == 15:
            assert ev == [("message", 2, 1, msgs[0]), ("message", 2, 1, msgs[1])]
        else:
            assert ev == [("message", 2, 1, msgs[0]), ("error", O.ERROR_CODES["invalid_distance"])]


def test_room():
    """a 1 000-byte run of one letter: with d_msg_cap = 100 as a single last
    piece buffer_overflow; as a piece inside the message that consumes all its
    input with output pending status 0, and the rest arrives with the next
    piece; d_msg_cap = 0"""
    run = b"a" * 1000
    zp = O.pmd_deflate(run)
    # the cut after which the model's inflater has taken all its input and still owes output
    cut = next(k for k in range(1, len(zp))
               if (lambda p: p.status == 0 and p.in_used == k and len(p.delivered) == 100)(
                   M.Conn(CLIENT).call(FM.frame(zp[:k], 2, False, 4), 64, 100)))
    whole = FM.frame(zp, 2, True, 4)
    split = [FM.frame(zp[:cut], 2, False, 4), FM.frame(zp[cut:], 0, True, 0)]
    empty = FM.frame(O.pmd_deflate(b""), 2, True, 4)
    rig = Rig(5, CLIENT, out_cap=64, msg_cap=2048)
    # entry 4: one input byte more than the room lets the inflater take
    a = rig.call([whole, split[0], whole, empty, FM.frame(zp[:cut + 1], 2, False, 4)], msg_cap=[100, 100, 0, 0, 100])
    assert [p.status for p in a] == [M.BUFFER_OVERFLOW, 0, M.BUFFER_OVERFLOW, 0, M.BUFFER_OVERFLOW]
    assert a[4].in_used == cut and len(a[4].delivered) == 100
    assert a[1].delivered == run[:100] and a[1].in_used == cut and a[3].stop.event == FM.EV_MESSAGE
    b = rig.call([b"", split[1], b"", b"", b""], msg_cap=[100, 2048, 0, 0, 100])
    assert b[1].status == 0 and b[1].stop.event == FM.EV_MESSAGE and a[1].delivered + b[1].delivered == run


def test_msg_max():
    """a message that reaches rd_msg_max exactly in its third piece gives 0,
    one byte more gives message_too_big in that piece and not earlier; a plain
    message is refused at header time; msg_max = 0 is no limit"""
    def wire(chunks):
        segs = M.deflate_chunks(chunks)
        segs[-1] = segs[-1][:-4]
        return [FM.frame(s, 2 if k == 0 else 0, k + 1 == len(segs), 4 if k == 0 else 0) for k, s in enumerate(segs)]
    exact, over = wire([b"x" * 40, b"y" * 40, b"z" * 20]), wire([b"x" * 40, b"y" * 40, b"z" * 21])
    plain = FM.frame(b"p" * 101, 2, True)
    ok = FM.frame(b"p" * 60, 2, False) + FM.frame(b"q" * 40, 0, True)
    late = FM.frame(b"p" * 60, 2, False) + FM.frame(b"q" * 41, 0, True)
    for msg_max in (100, 0):
        rig = Rig(5, CLIENT, msg_max=msg_max, out_cap=128, msg_cap=512)
        st = []
        for k in range(3):
            ps = rig.call([exact[k], over[k], plain if k == 0 else b"", ok if k == 0 else b"", late if k == 0 else b""])
            st.append([p.status if p else 0 for p in ps])
            assert [p.eff for p in ps[:2]] == [min(512, 100 - 40 * k + 1) if msg_max else 512] * 2
        big = M.MESSAGE_TOO_BIG if msg_max else 0
        assert st == [[0, 0, big, 0, big], [0, 0, 0, 0, 0], [0, big, 0, 0, 0]]
        assert ps[0].stop.event == FM.EV_MESSAGE and len(ps[1].delivered) == 21 and ps[1].stop.event == FM.EV_MESSAGE


def _split_wires(text, c, comp, op=1):
    """text as two frames whose pieces deliver text[:c] and text[c:]"""
    if comp:
        a, b = M.deflate_chunks([text[:c], text[c:]])
        return FM.frame(a, op, False, 4), FM.frame(b[:-4], 0, True, 0)
    return FM.frame(text[:c], op, False, 0), FM.frame(text[c:], 0, True, 0)


@pytest.mark.parametrize("comp", [0, 1])
def test_utf8(comp):
    """2-, 3- and 4-byte code points split across pieces at every position; an
    invalid prefix fails in the piece that holds it; a message that ends inside
    a code point fails at its last piece, also when that piece is empty"""
    text = "aé€😀z-ö".encode()
    bad_prefix = [b"ok\xe0\x80", b"ok\xf4\x90", b"\x80", b"ab\xc0", b"\xf0\x9f\x28"]
    cut_end = [b"ok\xe2\x82", b"\xf0\x9f\x98", b"z\xc3"]
    first, second, want = [], [], []
    for c in range(len(text) + 1):
        a, b = _split_wires(text, c, comp)
        first.append(a), second.append(b), want.append((0, 0))
    for t in bad_prefix:                      # fails in the first piece; the second is never looked at
        a, b = _split_wires(t + b"rest", len(t), comp)
        first.append(a), second.append(b), want.append((M.BAD_FRAME_PAYLOAD, None))
    for t in cut_end:                         # a valid prefix: fine inside the message, not at its end
        a, b = _split_wires(t + b"", len(t), comp)     # an empty last piece after a carry
        first.append(a), second.append(b), want.append((0, M.BAD_FRAME_PAYLOAD))
        a, b = _split_wires(t, 1, comp)
        first.append(a), second.append(b), want.append((0, M.BAD_FRAME_PAYLOAD))
    # the same bytes in a binary message are nobody's business
    a, b = _split_wires(bad_prefix[0] + b"x", 3, comp, op=2)
    first.append(a), second.append(b), want.append((0, 0))
    n = len(first)
    rig = Rig(n, CLIENT, out_cap=64, msg_cap=64, out_res=[(3 * i) % 16 for i in range(n)])
    pa = rig.call(first)
    pb = rig.call(second)
    assert [p.status for p in pa] == [w[0] for w in want]
    assert [None if p is None else p.status for p in pb] == [w[1] for w in want]
    for c in range(len(text) + 1):
        assert pa[c].delivered == text[:c] and pb[c].delivered == text[c:] and pb[c].stop.event == FM.EV_MESSAGE
    carries = {len(rig.conns[c].st.utf8) for c in range(len(text) + 1)}
    assert carries == {0}
    assert {p.state[24] for p in pa if p.state is not None} == {0, 1, 2, 3}      # utf8_n after the first piece


def test_errors():
    """a flipped payload bit gives the oracle's zlib::error in the piece that
    holds it; a refused header behind a good partial piece: the piece is
    delivered and the frame error reported"""
    zp = O.pmd_deflate(TEXT)
    rng = random.Random(17)
    wires = []
    for bit in rng.sample(range(8 * len(zp)), 60):
        bad = bytearray(zp)
        bad[bit >> 3] ^= 1 << (bit & 7)
        wires.append(FM.frame(bytes(bad), 2, True, 4))
    part = FM.frame(zp[:50], 2, False, 4)
    wires += [part + FM.frame(b"x", 0, True, 2),            # RSV2 on the continuation
              part + FM.frame(b"x", 2, True, 0),            # a data frame inside the message
              FM.frame(b"plain", 2, False) + FM.frame(b"x", 0, True, 4),   # RSV1 on a continuation
              FM.frame(b"plain", 2, False) + FM.frame(b"x" * 3, 11, True)]  # a reserved opcode
    n = len(wires)
    rig = Rig(n, CLIENT, out_cap=64, msg_cap=512)
    log = drive(rig, wires, 23)
    zerr = [ev[-1][1] for ev in map(events, log[:60]) if ev[-1][0] == "error"]
    assert len(zerr) >= 10 and all(2 <= e < 256 for e in zerr), zerr
    for i, want in zip(range(60, n), ["bad_reserved_bits", "bad_data_frame", "bad_reserved_bits", "bad_opcode"]):
        last, got = log[i][-1], b"".join(p.delivered for p in log[i])
        assert last.status == FM.ERR[want] and last.state is None
        assert len(got) > 0 and got == (TEXT[:len(got)] if i < 62 else b"plain")


def test_idle_and_mixed():
    """one call mixes idle entries, connections between messages, connections
    in the middle of a frame and of a message; the same without the extension,
    with NULL inflater arguments, where RSV1 is refused"""
    zp = O.pmd_deflate(TEXT)
    for pmd_on in (True, False):
        rng = random.Random(21)
        key = keyed(SERVER, rng)
        whole = FM.frame(zp, 1, True, 4, key()) if pmd_on else FM.frame(TEXT, 1, True, 0, key())
        frag = FM.frame(b"abc", 2, False, 0, key()) + FM.frame(b"defgh", 0, True, 0, key())
        rig = Rig(6, SERVER, pmd_on=pmd_on, out_cap=200, msg_cap=256)
        # call 1: 0 idle, 1 a whole message, 2 half a frame, 3 a fragment, 4 a cut header, 5 RSV1
        a = rig.call([b"", whole, whole[:40], frag[:9], whole[:3], FM.frame(zp, 2, True, 4, key())])
        assert a[0].state == M.ZERO and a[0].stop.consumed == 0 and a[4].stop.consumed == 0
        assert a[1].delivered == TEXT and a[1].stop.event == FM.EV_MESSAGE
        assert a[5].status == (0 if pmd_on else FM.ERR["bad_reserved_bits"])
        # call 2: 0 starts, 1 idle between messages, 2 idle inside its frame, 3 goes on, 4 still cut, 5 idle
        b = rig.call([frag, b"", b"", frag[9:], whole[:5], b""])
        assert b[2].state == a[2].state != M.ZERO and b[1].state == M.ZERO
        assert b[0].delivered == b"abcdefgh" and a[3].delivered + b[3].delivered == b"abcdefgh"
        c = rig.call([b"", b"", whole[40:], b"", whole, b""])
        assert a[2].delivered + c[2].delivered == TEXT and c[4].delivered == TEXT


def test_agreement_with_the_takeover_call():
    """whole-frame wire, a message per call: message bytes, statuses and events
    equal bpmd_receive_takeover_batch's"""
    torch, pmd = _pmd()
    rng = random.Random(23)
    n, k_msgs = 24, 4
    conns = []
    for c in range(n):
        msgs = [TC.json_message(rng.choice((0, 30, 700, 3000)), 7 * c + k) if (c + k) % 3 else
                TC.random_message(rng.choice((1, 200, 1500)), 5 * c + k) for k in range(k_msgs)]
        sent_comp = [k for k in range(k_msgs) if (c + k) % 4 != 0]
        # one deflate history per connection over the messages that are sent compressed
        pays = dict(zip(sent_comp, O.pmd_deflate_stream([msgs[k] for k in sent_comp], 6, 12, 4)))
        frames = []
        for k, m in enumerate(msgs):
            body, op = pays.get(k, m), 1 if (c + k) % 3 else 2
            if c == 5 and k == 2:
                body = bytes([body[0] | 0x06]) + body[1:]              # a damaged message: block type 3
            cut = len(body) // 2
            frames.append(FM.frame(body[:cut], op, False, 4 if k in pays else 0, rng.getrandbits(32)) +
                          FM.frame(body[cut:], 0, True, 0, rng.getrandbits(32)))
        conns.append((msgs, frames))
    tk = pmd.TakeoverReceiver(n, SERVER, window_bits=12, max_msg=4096, msg_max=1 << 20)
    pc = pmd.PieceReceiver(n, SERVER, window_bits=12, msg_max=1 << 20)
    dead = [False] * n
    for k in range(k_msgs):
        wire = pmd.Batch.from_host([b"" if dead[c] else conns[c][1][k] for c in range(n)])
        a = tk.recv(wire, 4096)
        b = pc.recv(wire, 4096 + 4, 4096)
        torch.cuda.synchronize()
        st = a.status.cpu().tolist()
        assert b.status.cpu().tolist() == st and b.event.cpu().tolist() == a.event.cpu().tolist()
        assert b.frames.consumed.cpu().tolist() == a.frames.consumed.cpu().tolist()
        assert b.frames.op.cpu().tolist() == a.frames.op.cpu().tolist()
        ma, mb = a.to_host(), b.to_host()
        for c in range(n):
            if dead[c]:
                continue
            if st[c] == 0:
                assert ma[c] == mb[c] == conns[c][0][k], (c, k)
            else:
                dead[c] = True
    assert sum(dead) == 1


@pytest.mark.parametrize("sender_role", [CLIENT, SERVER])
def test_round_trip_from_the_piece_sender(sender_role):
    """pmd.PieceSender -> pmd.PieceReceiver: messages sent in pieces of 1, 7
    and 4 096 bytes, the wire handed on in chunks unrelated to frame edges;
    every message arrives byte for byte"""
    torch, pmd = _pmd()
    rng = random.Random(31 + sender_role)
    n = 8
    tx = pmd.PieceSender(n, sender_role, level=6, max_piece=4096, threshold=0, frame_max=1000)
    peer = CLIENT if sender_role == SERVER else SERVER
    rx = pmd.PieceReceiver(n, peer)
    keys = None
    if sender_role == CLIENT:
        keys = torch.randint(-2 ** 31, 2 ** 31 - 1, (n * tx.key_stride,), dtype=torch.int32, device="cuda")
    want, scripts = [], []
    for c in range(n):
        msgs = [(TC.json_message(20, c), 1, 1), (TC.random_message(100, c), 2, 7), (TC.json_message(10000, 3 * c), 1, 4096),
                (TC.json_message(20, c), 1, 7)]
        want.append([(m, op) for m, op, _ in msgs])
        scripts.append([(m[a:a + sz], op, a + sz >= len(m)) for m, op, sz in msgs for a in range(0, len(m), sz)])
    stream = [b""] * n
    for t in range(max(map(len, scripts))):
        row = [s[t] if t < len(s) else (b"", 0, 1) for s in scripts]
        s = tx.send(pmd.Batch.from_host([r[0] for r in row]), [r[1] for r in row], [int(r[2]) for r in row], keys=keys)
        torch.cuda.synchronize()
        assert s.status.cpu().tolist() == [0] * n
        for c, w in enumerate(s.wire.to_host()):
            if row[c][1]:
                stream[c] += w
    got, cur, used, fed = [[] for _ in range(n)], [b""] * n, [0] * n, [0] * n
    steps = [rng.choice((333, 1000, 77)) for _ in range(n)]
    while any(used[c] < len(stream[c]) for c in range(n)):
        for c in range(n):
            fed[c] = min(len(stream[c]), fed[c] + steps[c])
        r = rx.recv(pmd.Batch.from_host([stream[c][used[c]:fed[c]] for c in range(n)]), 512, 1 << 15)
        torch.cuda.synchronize()
        assert r.status.cpu().tolist() == [0] * n
        ev, ops = r.event.cpu().tolist(), r.frames.op.cpu().tolist()
        for c, (piece, k) in enumerate(zip(r.to_host(), r.frames.consumed.cpu().tolist())):
            used[c] += k
            cur[c] += piece
            if ev[c] == FM.EV_MESSAGE:
                got[c].append((cur[c], ops[c]))
                cur[c] = b""
    assert got == want


# ---- long messages, pieces over the kernels' thresholds (inputs: tests/receive_pieces_cases.py, whose conditions
# tests/test_receive_pieces_cases.py checks on the CPU)

def run_case(case):
    """the case on a Rig of its own: every call compared with the model, then
    what each connection's pieces amount to"""
    rig = Rig(case.n, case.role, **case.rig)
    log = case.run(rig)
    for c in range(case.n):
        assert events(log[c]) == case.want[c], (c, case.tags[c])
        bad = None if case.fail_piece is None else case.fail_piece[c]
        assert [p.status for p in log[c]] == ([0] * len(log[c]) if bad is None else [0] * bad + [M.BAD_FRAME_PAYLOAD]), c
    return rig, log


def test_long_messages_in_read_buffer_pieces():
    """70 kept-context connections, four 16 KiB messages each of json, binary,
    random, corpus1 or zeros, through a 1 536-byte read buffer into 1 540-byte
    out slots; out slots, wire and message slots at every residue mod 16.  The
    pieces take the copy's and the scan's second round, every connection
    inflates 64 KiB through its 32 KiB window in calls that load the saved
    window and write it back, random's stored blocks span pieces, and a zeros
    piece delivers FLUSH_AT bytes from a few"""
    rig, log = run_case(C.long_messages())
    assert rig.calls >= 4 * 16384 // 1536 and max(p.out_len for ps in log for p in ps) == 1536


@pytest.mark.parametrize("wbits", [9, 10])
def test_small_window_wraps_many_times(wbits):
    """the same with 3 000-byte json messages in 100-byte pieces at window
    bits 9 and 10: the saved window wraps between calls about twenty times"""
    run_case(C.small_window(wbits))


def test_one_piece_over_staging_and_ring():
    """one call per message: 70 000 stored bytes (input far over the 4 KiB
    staging, from a misaligned slot; output that wraps the 64 KiB ring) or
    100 000 zeros from under 200 wire bytes, then a json message and an echo
    whose matches reach 32 000 bytes back into the window that call left"""
    rig, log = run_case(C.over_staging_ring())
    assert rig.calls == 3 and {len(ps[0].delivered) for ps in log} == {70000, 100000}


@pytest.mark.parametrize("comp", [0, 1])
def test_utf8_over_scan_rounds(comp):
    """2 600-byte text pieces in the out slot (comp 0) or the message slot
    (comp 1) at every residue: 2-, 3- and 4-byte code points at every split
    across the boundaries between the scan's rounds of 1 024 bytes, where lane
    63 fetches its own look-ahead; the same texts cut inside such a code point,
    so that a piece over 1 KiB leaves a carry or meets one; and continuation
    bytes replaced, lone continuations, E0 80 80, ED A0 80 and F4 90 80 80
    across the same boundaries, each failing in the piece the model says"""
    rig, log = run_case(C.utf8_rounds(comp))
    assert rig.calls == 2
