"""bpmd_receive_takeover_batch and pmd.TakeoverReceiver on the GPU: unframe,
inflate with context takeover and check in one chained call, connection by
connection against tests/receive_takeover_model.py (the frame model's walk,
the oracle's inflater given the connection's window, the oracle's UTF-8 check,
the merge and connection rules) and against the chain it replaces
(unframe_batch + TakeoverInflater.inflate + utf8_check_batch).

The Rig works through the C ABI on canary-filled wire, out and connection
buffers that stay on the device from call to call.  After every call the wire
must be unchanged, every output array and d_pos equal to the model's, the
whole out buffer equal to the gathered payloads, and the whole d_buf equal to
the host's record of it: the model's slides and inflated bytes applied to the
buffer as it was before the call.  One allowance, from the inflater's own
contract: inside a called slot [msg_off, msg_off + effective capacity) only
the first msg_len bytes are fixed; the rest is the inflater's scratch and is
taken over into the record as found."""
import ctypes
import random
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests import frame_parse_model as FM
from tests import receive_model as M
from tests import receive_takeover_model as TM
from tests import takeover_cases as TC
from tests.deflate_scripts import periodic
from tests.test_gpu_async import _call_behind_copies, _setup
from tests.test_gpu_receive import _utf8_sequences

pytestmark = pytest.mark.gpu

WIRE_FILL, OUT_FILL, BUF_FILL = 0xA5, 0x5A, 0xC3
INVALID_DISTANCE = 13


def _pmd():
    import torch  # noqa: F401
    from beast_amd import pmd
    return pmd


def _u32(v):
    """uint32 values as the int32 tensor the binding passes"""
    import torch
    return torch.from_numpy(np.asarray(v, dtype=np.uint32).view(np.int32).copy()).cuda()


class Got:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def c_call(wire, role, msg_max, wbits, state, out, out_off, out_cap, buf, base, slot, pos, msg_cap, work=None,
           stream=None):
    """bpmd_receive_takeover_batch itself; returns its output tensors"""
    import torch
    pmd = _pmd()
    L = pmd._recv_tk_lib()
    n, dev, p = wire.n, "cuda", pmd._ptr
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)  # noqa: E731
    r = Got(out_len=i32(), op=u8(n), compressed=u8(n), event=u8(n), status=i32(), consumed=i32(), ctl=u8(n, 128),
            ctl_len=u8(n), code=torch.empty(n, dtype=torch.int16, device=dev), msg_off=torch.empty(n, dtype=torch.int64, device=dev),
            msg_len=i32())
    if work is None:
        work = u8(max(int(L.bpmd_receive_takeover_work_bytes(n)), 1))
    cfg = pmd._Cfg(0, wbits, 8, 0, 0)
    pmd._check(L.bpmd_receive_takeover_batch(
        ctypes.byref(cfg), role, msg_max, p(wire.data), p(wire.off), p(wire.len), n, p(state), p(out), p(out_off),
        p(out_cap), p(r.out_len), p(r.op), p(r.compressed), p(r.event), p(r.status), p(r.consumed), p(r.ctl),
        p(r.ctl_len), p(r.code), p(buf), p(base), slot, p(pos), p(msg_cap), p(r.msg_off), p(r.msg_len), p(work),
        pmd._stream_handle(stream)), "bpmd_receive_takeover_batch")
    return r


class Rig:
    """n connections: their buffers of `slot` bytes at `bases` in one device
    buffer, their out slots at ragged offsets in another, positions and
    message states -- and the host's record of all four."""

    def __init__(self, n, wbits, slot, out_cap, rng, bases=None, pos=None, prefill=None):
        import torch
        self.n, self.wbits, self.W, self.slot, self.ocap, self.rng = n, wbits, 1 << wbits, slot, out_cap, rng
        # packed end to start from an odd offset: a store past a slot hits the next connection's window
        self.bases = list(bases) if bases is not None else [5 + i * slot for i in range(n)]
        self.buf = np.full(max(self.bases) + slot + 64, BUF_FILL, np.uint8)
        self.pos = list(pos) if pos is not None else [0] * n
        for i, b in enumerate(prefill or []):   # bytes a connection has received before
            self.buf[self.bases[i]:self.bases[i] + len(b)] = np.frombuffer(b, np.uint8)
        self.offs, pos_ = [], 0
        for _ in range(n):
            pos_ += rng.randrange(1, 20)
            self.offs.append(pos_)
            pos_ += out_cap
        self.out = np.full(pos_ + 64, OUT_FILL, np.uint8)
        self.m_state = [FM.State() for _ in range(n)]
        self.m_slot = [bytearray([OUT_FILL]) * out_cap for _ in range(n)]
        self.slides = 0
        t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
        self.d_buf = torch.from_numpy(self.buf.copy()).cuda()
        self.d_out = torch.from_numpy(self.out.copy()).cuda()
        self.d_base, self.d_off = t64(self.bases), t64(self.offs)
        self.d_pos = torch.tensor(self.pos, dtype=torch.int32, device="cuda")
        self.d_cap = torch.full((n,), out_cap, dtype=torch.int32, device="cuda")
        self.d_state = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")

    def call(self, bufs, role, msg_caps, msg_max=16 << 20):
        """One call over bufs (connection i's wire bytes, b"" for an idle one),
        compared with the model in every output and every buffer; returns
        (device results, model results)."""
        import torch
        pmd = _pmd()
        n = self.n
        assert len(bufs) == n
        msg_caps = [msg_caps] * n if isinstance(msg_caps, int) else list(msg_caps)
        woffs, wpos = [], 0
        for b in bufs:
            wpos += self.rng.randrange(1, 20)
            woffs.append(wpos)
            wpos += len(b)
        wire = np.full(wpos + 64, WIRE_FILL, np.uint8)
        for o, b in zip(woffs, bufs):
            wire[o:o + len(b)] = np.frombuffer(b, np.uint8)
        wb = pmd.Batch(torch.from_numpy(wire.copy()).cuda(), torch.tensor(woffs, dtype=torch.int64, device="cuda"),
                       torch.tensor([len(b) for b in bufs], dtype=torch.int32, device="cuda"))
        r = c_call(wb, role, msg_max, self.wbits, self.d_state, self.d_out, self.d_off, self.d_cap, self.d_buf,
                   self.d_base, self.slot, self.d_pos, _u32(msg_caps))
        torch.cuda.synchronize()
        assert np.array_equal(wb.data.cpu().numpy(), wire), "the wire was modified"
        got_buf, got_out = self.d_buf.cpu().numpy(), self.d_out.cpu().numpy()
        state = self.d_state.cpu().numpy()
        ev, stt, con = r.event.tolist(), r.status.tolist(), r.consumed.tolist()
        ol, op, comp = r.out_len.tolist(), r.op.tolist(), r.compressed.tolist()
        ctl, cl, code = r.ctl.cpu().numpy(), r.ctl_len.tolist(), (r.code.to(torch.int32) & 0xFFFF).tolist()
        ml, mo, dpos = r.msg_len.tolist(), r.msg_off.tolist(), self.d_pos.tolist()
        got, want = [], []
        for i, b in enumerate(bufs):
            base = self.bases[i]
            m_buf = bytearray(self.buf[base:base + self.slot].tobytes())
            e = TM.receive(b, role, msg_max, self.ocap, msg_caps[i], self.m_state[i], self.m_slot[i], self.pos[i], m_buf,
                           self.wbits)
            s = e.stop
            g = Got(event=ev[i], status=stt[i], consumed=con[i], out_len=ol[i], op=op[i], compressed=comp[i],
                    ctl=ctl[i, :cl[i]].tobytes(), close_code=code[i], state=state[i].tobytes(), msg_len=ml[i],
                    msg_off=mo[i] - base, pos=dpos[i])
            assert (g.event, g.status, g.consumed, g.out_len, g.op, g.compressed, g.ctl, g.close_code, g.state,
                    g.msg_len, g.msg_off, g.pos) == \
                (s.event, e.status, s.consumed, s.out_len, s.op, s.compressed, s.ctl, s.close_code, s.state, e.msg_len,
                 e.msg_off, e.pos), (i, b[:40].hex(), g.__dict__, e)
            if e.inflated is not None:   # the inflater's scratch inside its capacity (see the module's docstring)
                a, z = e.msg_off + len(e.inflated), e.msg_off + e.eff_cap
                m_buf[a:z] = got_buf[base + a:base + z].tobytes()
            self.buf[base:base + self.slot] = np.frombuffer(bytes(m_buf), np.uint8)
            self.pos[i] = e.pos
            self.slides += e.slid
            g.message = None
            if g.event == FM.EV_MESSAGE and g.status in (0, M.BAD_FRAME_PAYLOAD):
                src, o = (got_buf, mo[i]) if g.compressed else (got_out, self.offs[i])
                g.message = src[o:o + g.msg_len].tobytes()
            assert g.message == e.message, i
            got.append(g)
            want.append(e)
        for o, s in zip(self.offs, self.m_slot):
            self.out[o:o + self.ocap] = np.frombuffer(bytes(s[:self.ocap]), np.uint8)
        diff = np.flatnonzero(got_out != self.out)
        assert diff.size == 0, ("out buffer differs from the gathered payloads", diff[:8].tolist())
        diff = np.flatnonzero(got_buf != self.buf)
        assert diff.size == 0, ("d_buf differs from the record", diff[:8].tolist(), self.bases[:3], self.slot)
        return got, want


# ---------------------------------------------------------------------------
# Traffic of many connections that get out of step

class Traffic:
    """Per round, each connection of TC.schedule's subset gets one of: the next
    message of its kept deflate stream (text or binary), the same in two
    fragments with a ping between, the same with its last byte held back for a
    round, an uncompressed message, a close.  What a call does not consume
    stays in front of the connection's next bytes."""

    KINDS = ("z", "z", "z", "frag", "cut", "plain", "plain", "close")

    def __init__(self, rng, n, wbits, lens, masked, rounds=8):
        self.rng, self.n, self.masked = rng, n, masked
        self.plan = [{c: rng.choice(self.KINDS) for c in cr} for cr in TC.schedule(rng, [rounds] * n)[:rounds]]
        count = [sum(p.get(c) in ("z", "frag", "cut") for p in self.plan) for c in range(n)]
        self.msgs = [TC.connection_messages(c, [rng.choice(lens) for _ in range(count[c])], wbits, seed=17)
                     for c in range(n)]
        # CPython's deflater and the oracle's, kept across each connection's messages
        self.pls = [TC.zlib_stream(ms, (6, 9)[c % 4 // 2], wbits) if c % 2 else O.pmd_deflate_stream(ms, 6, wbits, 4)
                    for c, ms in enumerate(self.msgs)]
        self.next = [0] * n
        self.pending = [b""] * n
        self.sent = [[] for _ in range(n)]   # (op, message) in the order they must arrive

    def needs_history(self, wbits):
        """(later messages that fail when inflated without what came before, later messages)"""
        later = [p for pl in self.pls for p in pl[1:]]
        return sum(1 for p in later if O.pmd_inflate(p, cap=1 << 16, wbits=wbits)[0] != 0), len(later)

    def _key(self):
        return self.rng.getrandbits(32) if self.masked else None

    def round(self, r):
        hold = [0] * self.n
        for c, kind in (self.plan[r] if r < len(self.plan) else {}).items():
            if kind == "close":
                w = FM.frame((1000).to_bytes(2, "big") + b"bye", 8, key=self._key())
            elif kind == "plain":
                op = self.rng.choice([1, 2])
                m = ("plain text ü %d" % c).encode() * self.rng.randrange(0, 4) + (b"\xff" if c % 5 == 0 else b"")
                w = FM.frame(m, op, key=self._key())
                self.sent[c].append((op, m))
            else:
                k = self.next[c]
                self.next[c] += 1
                op, p = self.rng.choice([1, 2]), self.pls[c][k]
                self.sent[c].append((op, self.msgs[c][k]))
                if kind == "frag":
                    h = len(p) // 2
                    w = FM.frame(p[:h], op, fin=False, rsv=4, key=self._key()) + \
                        FM.frame(b"still there?", 9, key=self._key()) + FM.frame(p[h:], 0, key=self._key())
                else:
                    w = FM.frame(p, op, rsv=4, key=self._key())
                    hold[c] = int(kind == "cut")
            self.pending[c] += w
        return [p[:len(p) - h] for p, h in zip(self.pending, hold)]

    def consumed(self, got):
        for c, g in enumerate(got):
            self.pending[c] = self.pending[c][g.consumed:]


def _mixed(wbits, masked, seed):
    rng = random.Random(seed)
    lens = (0, 1, 300, 300, 700, 700) if wbits == 9 else (0, 300, 4096, 9000, 9000)
    return rng, Traffic(rng, 96, wbits, lens, masked), max(lens)


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("wbits", [9, 15])
def test_mixed_connections_out_of_step(wbits, masked):
    """96 connections, 8 rounds and what it takes to drain them.  Half of the
    connections start with a buffer that is nearly full of earlier bytes, so
    windows slide at window_bits 15 too.  At least half of the later messages
    of the kept streams cannot be inflated without the window."""
    rng, tr, max_msg = _mixed(wbits, masked, 1000 + wbits)
    need, later = tr.needs_history(wbits)
    assert 2 * need >= later > 150, (need, later)
    W = 1 << wbits
    slot = 2 * W + max_msg + 1   # odd: the packed buffers start at every residue mod 16
    pos0 = [0 if c % 2 == 0 else slot - (c * 613) % (2 * max_msg) for c in range(tr.n)]
    before = [rng.randbytes(min(p, W + 40)).rjust(p, b"\x11") for p in pos0]
    rig = Rig(tr.n, wbits, slot, max(len(p) for pl in tr.pls for p in pl) + 8, rng, pos=pos0, prefill=before)
    assert {b % 16 for b in rig.bases} == set(range(16))
    role = FM.SERVER if masked else FM.CLIENT
    arrived = [[] for _ in range(tr.n)]
    events, statuses = set(), set()
    for r in range(40):
        bufs = tr.round(r)
        if r >= 8 and not any(bufs):
            break
        got, want = rig.call(bufs, role, max_msg)
        tr.consumed(got)
        for c, (g, e) in enumerate(zip(got, want)):
            events.add(g.event)
            if g.event == FM.EV_MESSAGE:
                statuses.add(g.status)
                assert e.zst == 0 and g.status in (0, M.BAD_FRAME_PAYLOAD)
                arrived[c].append((g.op, g.message))
    assert r < 39 and not any(tr.pending)
    assert arrived == tr.sent                                  # every message, in order, byte for byte
    assert events == {FM.EV_NEED_MORE, FM.EV_MESSAGE, FM.EV_PING, FM.EV_CLOSE}
    assert statuses == {0, M.BAD_FRAME_PAYLOAD}
    assert rig.slides >= 20, rig.slides


def test_equals_the_chain_it_replaces():
    """pmd.TakeoverReceiver against unframe_batch + a host-side pick +
    TakeoverInflater.inflate + utf8_check_batch on the mixed test's traffic:
    events, statuses, consumed bytes, messages and positions, round by round."""
    import torch
    pmd = _pmd()
    wbits = 9
    rng, tr, max_msg = _mixed(wbits, True, 1000 + wbits)
    out_cap = max(len(p) for pl in tr.pls for p in pl) + 8
    new = pmd.TakeoverReceiver(tr.n, pmd.ROLE_SERVER, window_bits=wbits, max_msg=max_msg)
    old = pmd.TakeoverInflater(tr.n, window_bits=wbits, max_msg=max_msg)
    assert new.slot == old.slot
    st = pmd.rd_state(tr.n)
    stride = (out_cap + 15) // 16 * 16
    out = torch.zeros(tr.n * stride + 16, dtype=torch.uint8, device="cuda")
    off = torch.arange(tr.n, dtype=torch.int64, device="cuda") * stride
    slid = msgs = 0
    for r in range(40):
        bufs = tr.round(r)
        if r >= 8 and not any(bufs):
            break
        wire = pmd.Batch.from_host(bufs)
        rn = new.recv(wire, out_cap)
        u = pmd.unframe_batch(wire, out_cap, pmd.ROLE_SERVER, state=st, out=out, out_off=off)
        status = u.status.clone()
        done = (u.event == pmd.EV_MESSAGE) & (u.status == 0)
        zi = torch.nonzero(done & (u.compressed != 0)).flatten()
        ti = torch.nonzero(done & (u.op == 1)).flatten()
        before = old.pos.clone()
        text = [None] * tr.n
        if zi.numel():
            res = old.inflate(pmd.Batch(u.out.data, u.out.off[zi].contiguous(), u.out.len[zi].contiguous()), max_msg,
                              conn=zi)
            status[zi] = res.status
            for j, c in enumerate(zi.tolist()):
                text[c] = res.out.message(j)
        slid += int((old.pos < before).sum())
        for c in torch.nonzero(done & (u.compressed == 0)).flatten().tolist():
            text[c] = u.out.message(c)
        if ti.numel():   # text, where the message lies
            sub = pmd.Batch.from_host([text[c] for c in ti.tolist()])
            verdict = pmd.utf8_check_batch(sub)
            status[ti] = torch.where((status[ti] == 0) & (verdict != 0), pmd.BAD_FRAME_PAYLOAD, status[ti])
        torch.cuda.synchronize()
        assert rn.event.tolist() == u.event.tolist() and rn.frames.consumed.tolist() == u.consumed.tolist()
        assert rn.status.tolist() == status.tolist()
        assert rn.to_host() == text
        assert new.pos.tolist() == old.pos.tolist()
        msgs += sum(t is not None for t in text)
        tr.consumed([Got(consumed=k) for k in u.consumed.tolist()])
    assert not any(tr.pending) and msgs == sum(map(len, tr.sent)) and slid >= 20


# ---------------------------------------------------------------------------
# The edges

def test_slide_edges():
    """window_bits 9.  Each connection has received p0 bytes of a text of
    period 512 or 513 and gets the text's next bytes, deflated by CPython's
    kept deflater with a 1 KiB window, with a capacity that puts pos + capacity
    at slot - 1, slot and slot + 1: the last slides.  Every match reaches one
    period back: 512 is the window's first byte, 513 lies before it
    (invalid_distance), whether the window slid or not.  A second message
    follows on every connection."""
    W, slot = 512, 2 * 512 + 701
    cases = [(d, period, ln) for d in (-1, 0, 1) for period in (W, W + 1) for ln in (40, 300, 690)]
    prefill, pos0, caps, pls = [], [], [], []
    for d, period, ln in cases:
        cap = ln + 3
        p0 = slot + d - cap
        text = periodic(period, p0 + ln + 100, seed=period % 5)
        z = zlib.compressobj(9, zlib.DEFLATED, -10)
        ps = []
        for m in (text[:p0], text[p0:p0 + ln], text[p0 + ln:]):
            p = z.compress(m) + z.flush(zlib.Z_SYNC_FLUSH)
            ps.append(p[:-4])
        assert p0 > 2 * W and O.pmd_inflate(ps[1], cap=cap, wbits=9)[0] != 0   # it needs the window
        prefill.append(text[:p0])
        pos0.append(p0)
        caps.append(cap)
        pls.append(ps[1:])
    rng = random.Random(5)
    rig = Rig(len(cases), 9, slot, 800, rng, pos=pos0, prefill=prefill)
    assert {b % 16 for b in rig.bases} == set(range(16))
    got, want = rig.call([FM.frame(p[0], 2, rsv=4) for p in pls], FM.CLIENT, caps, msg_max=0)
    for g, e, (d, period, ln), p0, cap in zip(got, want, cases, pos0, caps):
        assert e.slid == (d == 1) and e.eff_cap == cap
        assert g.msg_off == (W if d == 1 else p0)
        if period == W:
            assert (g.status, g.msg_len, g.pos) == (0, ln, g.msg_off + ln)
        else:
            assert (g.status, g.pos) == (INVALID_DISTANCE, g.msg_off) and g.msg_len < ln
    assert rig.slides == len(cases) // 3
    got, want = rig.call([FM.frame(p[1], 2, rsv=4) for p in pls], FM.CLIENT, 120, msg_max=0)
    assert {g.status for g in got} == {0, INVALID_DISTANCE}
    assert all(g.status == 0 and g.msg_len == 100 for g, c in zip(got, cases) if c[1] == W)


@pytest.mark.parametrize("length", [300])
def test_capacity_and_limit(length):
    """msg_max in {len - 2 .. len + 2, 0} x d_msg_cap in {len - 1, len, len + 1,
    slot - 2W, slot - 2W + 1, 2^32 - 1} (the last two are clamped to the
    first of them), text and binary, on a message that needs the connection's
    first one; the same with its first block header damaged (the zlib error
    precedes any limit and wins) or its middle (the model decides).  d_pos
    advances iff the inflater's own status is 0: with message_too_big after a
    fit of msg_max + 1 bytes it does, after a zlib error or an outgrown
    capacity it does not."""
    rng = random.Random(43)
    W, slot = 512, 2 * 512 + length + 100
    room = slot - 2 * W
    first = TC.json_message(600, 77)
    text = first[-200:-200 + length // 2] + TC.json_message(length - length // 2, 78)
    assert len(text) == length and O.utf8_check(text) == 0
    z = TC.zlib_stream([first, text], 9, 9)[1]
    assert O.pmd_inflate(z, cap=length, wbits=9)[0] != 0          # it needs the window
    head = bytearray(z)
    head[0] |= 6                                                  # block type 3
    mid = bytearray(z)
    mid[len(z) // 2] ^= 0x10
    caps = [length - 1, length, length + 1, room, room + 1, M.U32]
    cases = [(op, cap, p) for op in (1, 2) for cap in caps for p in (z, bytes(head), bytes(mid))]
    bufs = [FM.frame(p, op, rsv=4) for op, _, p in cases]
    seen, advanced_too_big = set(), 0
    for msg_max in [length - 2, length - 1, length, length + 1, length + 2, 0]:
        rig = Rig(len(cases), 9, slot, len(z) + 4, rng, pos=[len(first)] * len(cases), prefill=[first] * len(cases))
        got, want = rig.call(bufs, FM.CLIENT, [c for _, c, _ in cases], msg_max=msg_max)
        for g, e, (op, cap, p) in zip(got, want, cases):
            cap = min(cap, room)                                   # the clamp
            eff = min(cap, msg_max + 1) if msg_max else cap
            assert e.eff_cap == eff and not e.slid
            if p is z:   # the rule, spelled out
                over_max, over_cap = bool(msg_max) and length > msg_max, length > cap
                rule = (FM.ERR["message_too_big"] if msg_max <= cap else FM.ERR["buffer_overflow"]) if over_max else \
                    FM.ERR["buffer_overflow"] if over_cap else 0
                assert g.status == rule, (msg_max, cap, op)
                assert g.msg_len == min(length, eff)
                fits = length <= eff                               # the inflater's own status is 0
                assert g.pos == len(first) + (g.msg_len if fits else 0), (msg_max, cap, op)
                advanced_too_big += fits and rule == FM.ERR["message_too_big"]
                assert g.message == (text if rule == 0 else None)
            elif p == bytes(head):
                assert (g.status, g.msg_len, g.message, g.pos) == (4 + 1, 0, None, len(first)), (msg_max, cap, op)
            seen.add(g.status)
    assert {0, FM.ERR["message_too_big"], FM.ERR["buffer_overflow"], 5} <= seen
    assert advanced_too_big >= 4


@pytest.mark.parametrize("residue", range(16))
def test_utf8_from_the_connection_buffer(residue):
    """Text whose invalid or incomplete code point sits at byte 0, at the unit
    edges 15 / 16 / 17, as the last bytes and before a tail; the message
    starts at `residue` mod 16 of d_buf because a first binary message of
    32 + residue bytes went before it.  Compressed text is checked in the
    connection's buffer, plain text in its gathered slot: among the cases are
    valid texts whose deflated bytes are not UTF-8."""
    rng = random.Random(61 + residue)
    texts = [b"a" * at + seq + tail for seq in _utf8_sequences() for at in (0, 15, 16, 17) for tail in (b"", b"~" * 40)]
    cases = [(t, comp) for t in texts for comp in (True, False)]
    first = rng.randbytes(32 + residue)
    pls = [TC.zlib_stream([first, t], 6, 9) for t, _ in cases]
    slot = 2 * 512 + 128
    rig = Rig(len(cases), 9, slot, 160, rng, bases=[16 * 3 + i * slot for i in range(len(cases))])
    got, _ = rig.call([FM.frame(p[0], 2, rsv=4) for p in pls], FM.CLIENT, 128)
    assert all((g.status, g.pos) == (0, len(first)) for g in got)
    got, _ = rig.call([FM.frame(p[1], 1, rsv=4) if comp else FM.frame(t, 1) for p, (t, comp) in zip(pls, cases)],
                      FM.CLIENT, 128)
    for i, (g, (t, comp)) in enumerate(zip(got, cases)):
        bad = M.BAD_FRAME_PAYLOAD if O.utf8_check(t) else 0
        assert (g.event, g.status, g.compressed, g.message) == (FM.EV_MESSAGE, bad, int(comp), t), i
        if comp:   # it lies at the residue, and the position advances whatever the verdict
            assert (rig.bases[i] + g.msg_off) % 16 == residue and g.pos == len(first) + len(t)
        else:
            assert g.pos == len(first)
    assert {g.status for g in got} == {0, M.BAD_FRAME_PAYLOAD}
    assert any(O.utf8_check(p[1]) and not O.utf8_check(t) for p, (t, c) in zip(pls, cases) if c)


def test_errors_stay_local():
    """Round 2 of 3 carries a damaged payload in every third connection: the
    oracle's status, position unchanged, no byte outside its called slot
    changed (Rig.call compares the whole buffer); its neighbours are exact in
    this round and the next."""
    rng = random.Random(23)
    n, wbits, max_msg = 60, 9, 700
    msgs = [TC.connection_messages(c, [rng.choice((300, 700)) for _ in range(3)], wbits, seed=3) for c in range(n)]
    pls = [TC.zlib_stream(ms, 6, wbits) for ms in msgs]
    rig = Rig(n, wbits, 2 * 512 + max_msg + 1, max(len(p) for pl in pls for p in pl) + 4, rng)
    got, _ = rig.call([FM.frame(p[0], 2, rsv=4) for p in pls], FM.CLIENT, max_msg)
    assert all(g.status == 0 for g in got)
    hit = 0
    for c in range(0, n, 3):
        for _ in range(200):   # a damage that the oracle notices
            q = bytearray(pls[c][1])
            q[rng.randrange(len(q))] ^= 1 << rng.randrange(8)
            if TM.inflate_after(msgs[c][0][-512:], bytes(q), max_msg, wbits)[0] > 1:   # a zlib error, not need_buffers
                pls[c][1] = bytes(q)
                hit += 1
                break
    assert hit == n // 3
    before = list(rig.pos)
    got, want = rig.call([FM.frame(p[1], 2, rsv=4) for p in pls], FM.CLIENT, max_msg)
    for c, (g, e) in enumerate(zip(got, want)):
        if c % 3 == 0:
            assert g.status == e.zst != 0 and g.pos == before[c] and g.message is None
        else:
            assert (g.status, g.message) == (0, msgs[c][1])
    got, _ = rig.call([b"" if c % 3 == 0 else FM.frame(p[2], 2, rsv=4) for c, p in enumerate(pls)], FM.CLIENT, max_msg)
    assert all(g.event == FM.EV_NEED_MORE and g.pos == before[c] for c, g in enumerate(got) if c % 3 == 0)
    assert all((g.status, g.message) == (0, msgs[c][2]) for c, g in enumerate(got) if c % 3)
    assert rig.slides > 0


def test_grid_stride_over_tiny_entries():
    """12 000 connections, more than the kernels' grids hold waves: every third
    completes a compressed message that copies from the 24 bytes its
    connection received before, the others reach the inflater with length 0."""
    import torch
    pmd = _pmd()
    n, wbits, slot = 12000, 9, 2 * 512 + 32
    OUT_CAP, MSG_CAP, WSTRIDE, MSG_MAX = 32, 24, 48, 20
    first = b"hello hello, said the hen"[:24]
    texts = [b"", b"a", b"hello hello hello", b"said the hen, hello hello", b"the hen \xff"]
    pl = [TC.zlib_stream([first, t], 9, wbits)[1] for t in texts]
    assert sum(O.pmd_inflate(p, cap=64, wbits=wbits)[0] != 0 for p in pl) >= 2      # they copy from `first`
    zs = [FM.frame(p, 1, rsv=4) for p in pl]
    others = [FM.frame(b"plain text", 1), FM.frame(b"\xffbinary", 2), FM.frame(b"plain \xc3", 1), FM.frame(b"ping", 9),
              zs[2][:-1], FM.frame(b"abc", 1, rsv=2), b""]
    bufs = [zs[(i // 3) % len(zs)] if i % 3 == 0 else others[(i // 3 * 2 + i % 3) % len(others)] for i in range(n)]
    assert max(map(len, bufs)) <= WSTRIDE
    start = bytearray([BUF_FILL]) * slot
    start[:len(first)] = first
    kinds = {}
    for b in set(bufs):
        o, m_buf = bytearray([OUT_FILL]) * OUT_CAP, bytearray(start)
        kinds[b] = (TM.receive(b, FM.CLIENT, MSG_MAX, OUT_CAP, MSG_CAP, FM.State(), o, len(first), m_buf, wbits), o, m_buf)
    wire = np.full(n * WSTRIDE + 16, WIRE_FILL, np.uint8)
    for i, b in enumerate(bufs):
        wire[i * WSTRIDE:i * WSTRIDE + len(b)] = np.frombuffer(b, np.uint8)
    ar = lambda k: torch.arange(n, dtype=torch.int64, device="cuda") * k  # noqa: E731
    wb = pmd.Batch(torch.from_numpy(wire.copy()).cuda(), ar(WSTRIDE),
                   torch.tensor([len(b) for b in bufs], dtype=torch.int32, device="cuda"))
    buf0 = np.concatenate([np.tile(np.frombuffer(bytes(start), np.uint8), n), np.full(16, BUF_FILL, np.uint8)])
    d_buf = torch.from_numpy(buf0.copy()).cuda()
    d_out = torch.full((n * OUT_CAP + 16,), OUT_FILL, dtype=torch.uint8, device="cuda")
    d_pos = torch.full((n,), len(first), dtype=torch.int32, device="cuda")
    full = lambda v: torch.full((n,), v, dtype=torch.int32, device="cuda")  # noqa: E731
    r = c_call(wb, pmd.ROLE_CLIENT, MSG_MAX, wbits, torch.zeros((n, 16), dtype=torch.uint8, device="cuda"), d_out,
               ar(OUT_CAP), full(OUT_CAP), d_buf, ar(slot), slot, d_pos, full(MSG_CAP))
    torch.cuda.synchronize()
    assert np.array_equal(wb.data.cpu().numpy(), wire)
    exp = [kinds[b][0] for b in bufs]
    assert r.event.tolist() == [e.stop.event for e in exp]
    assert r.status.tolist() == [e.status for e in exp]
    assert r.msg_len.tolist() == [e.msg_len for e in exp]
    assert r.msg_off.tolist() == [i * slot + e.msg_off for i, e in enumerate(exp)]
    assert d_pos.tolist() == [e.pos for e in exp]
    assert r.consumed.tolist() == [e.stop.consumed for e in exp]
    assert {FM.ERR["message_too_big"], M.BAD_FRAME_PAYLOAD, 0, FM.ERR["bad_reserved_bits"]} <= {e.status for e in exp}
    assert sum(e.inflated is not None for e in exp) == n // 3
    tail = d_buf.cpu().numpy()[n * slot:]
    assert np.array_equal(tail, np.full(16, BUF_FILL, np.uint8))
    got_buf = d_buf.cpu().numpy()[:n * slot].reshape(n, slot)
    want_buf = np.stack([np.frombuffer(bytes(kinds[b][2]), np.uint8) for b in bufs])
    for i, e in enumerate(exp):
        if e.inflated is not None:   # the inflater's scratch
            a, z = e.msg_off + len(e.inflated), e.msg_off + e.eff_cap
            want_buf[i, a:z] = got_buf[i, a:z]
    assert np.array_equal(got_buf, want_buf)
    want_out = np.stack([np.frombuffer(bytes(kinds[b][1]), np.uint8) for b in bufs]).reshape(-1)
    assert np.array_equal(d_out.cpu().numpy(), np.concatenate([want_out, np.full(16, OUT_FILL, np.uint8)]))


# ---------------------------------------------------------------------------
# The Python class and the call's edges

def test_argument_errors_and_empty_batches():
    import torch
    pmd = _pmd()
    empty = pmd.Batch(torch.empty(16, dtype=torch.uint8, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"),
                      torch.empty(0, dtype=torch.int32, device="cuda"))
    r = pmd.TakeoverReceiver(0, pmd.ROLE_SERVER, window_bits=9).recv(empty, 16)
    assert r.event.numel() == 0 and r.msg.len.numel() == 0 and r.to_host() == []
    with pytest.raises(pmd.BpmdError):
        pmd.TakeoverReceiver(0, 2, window_bits=9).recv(empty, 16)
    with pytest.raises(pmd.BpmdError):
        pmd.TakeoverReceiver(0, pmd.ROLE_SERVER, window_bits=7).recv(empty, 16)
    rx = pmd.TakeoverReceiver(1, pmd.ROLE_CLIENT, window_bits=9, max_msg=64)
    pls = TC.zlib_stream([b"hello hello", b"hello again, hello"], 9, 9)
    with pytest.raises(pmd.BpmdError):   # one entry per connection
        rx.recv(empty, 32)
    with pytest.raises(pmd.BpmdError):
        rx.recv(pmd.Batch.from_host([FM.frame(pls[0], 1, rsv=4)]), 32, msg_cap=65)
    got = []
    for p in pls:
        r = rx.recv(pmd.Batch.from_host([FM.frame(p, 1, rsv=4)]), 32)
        torch.cuda.synchronize()
        got += r.to_host()
    assert got == [b"hello hello", b"hello again, hello"] and rx.pos.tolist() == [29]
    with pytest.raises(pmd.BpmdError):   # the gathered slots keep fragments from call to call
        rx.recv(pmd.Batch.from_host([b""]), 48)
    # the C call: a slot of exactly two windows is refused, one byte more is served
    one = pmd.Batch.from_host([FM.frame(pls[0], 1, rsv=4)])
    t = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")  # noqa: E731
    args = dict(state=torch.zeros((1, 16), dtype=torch.uint8, device="cuda"),
                out=torch.zeros(64, dtype=torch.uint8, device="cuda"), out_off=t([0], torch.int64),
                out_cap=t([32], torch.int32), buf=torch.zeros(2048, dtype=torch.uint8, device="cuda"),
                base=t([0], torch.int64), pos=t([0], torch.int32), msg_cap=t([64], torch.int32))
    with pytest.raises(pmd.BpmdError):
        c_call(one, pmd.ROLE_CLIENT, 0, 9, slot=1024, **args)
    r = c_call(one, pmd.ROLE_CLIENT, 0, 9, slot=1025, **args)   # room for one byte
    torch.cuda.synchronize()
    assert (r.status.tolist(), r.msg_len.tolist(), args["pos"].tolist()) == ([FM.ERR["buffer_overflow"]], [1], [0])


def test_the_call_reads_nothing_back():
    """As tests/test_gpu_async.py: behind long copies queued on the stream,
    TakeoverReceiver.recv returns while they still run.  4 096 connections with
    1 KiB messages at window_bits 9, so every other call slides windows."""
    torch, pmd, dev, big, big2 = _setup()
    n, rounds = 4096, 5
    msgs = [[TC.json_message(1024, 7 * c + k) for k in range(rounds)] for c in range(16)]
    pls = [TC.zlib_stream(ms, 6, 9) for ms in msgs]
    wires = [pmd.Batch.from_host([FM.frame(pls[c % 16][k], 1, rsv=4) for c in range(n)]) for k in range(rounds)]
    rx = pmd.TakeoverReceiver(n, pmd.ROLE_CLIENT, window_bits=9, max_msg=1024)
    out_cap = max(len(p) for pl in pls for p in pl)
    for k in range(rounds - 1):   # the stream's pools reach this batch's size
        r = rx.recv(wires[k], out_cap)
    torch.cuda.synchronize()
    assert int((r.status != 0).sum()) == 0 and r.to_host()[:16] == [ms[rounds - 2] for ms in msgs]
    last = []
    assert not _call_behind_copies(torch, lambda: last.append(rx.recv(wires[-1], out_cap)), big, big2), \
        "the call waited for the queued copies"
    assert int((last[0].status != 0).sum()) == 0 and last[0].to_host()[-16:] == [ms[-1] for ms in msgs]
    assert int((rx.pos != 1024 + 512).sum()) == 0   # 5 KiB through 2 KiB + 1 KiB: the windows slid
