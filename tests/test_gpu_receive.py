"""bpmd_receive_batch and pmd.recv_batch on the GPU: unframe, inflate and
check in one chained call, entry by entry against tests/receive_model.py (the
frame model's walk, the oracle's inflater at the effective capacity, the
oracle's UTF-8 check and the merge rule) and against pmd.receive_batch, the
chain it replaces.  Entries lie at ragged offsets with guard bytes between
them, out and message slots likewise; wire, out and msg are canary-filled and
after every call the wire must be unchanged and the whole out and msg buffers
equal to what the expected results alone would have written.

One allowance, from bpmd_inflate_batch's own contract: it fixes the first
out_len bytes of a slot and stores nothing at or past the capacity it was
given, and the bytes between the two are its scratch (a decoder's last wide
store may run past the message's end inside the capacity).  So the bytes
[msg_len, effective capacity) of an inflated entry's slot are not compared;
everything else of the buffer is."""
import ctypes
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import frame_parse_model as FM
from tests import receive_model as M
from tests import utf8_cases
from tests.test_gpu_async import _call_behind_copies, _setup
from tests.test_gpu_unframe import _json_messages

pytestmark = pytest.mark.gpu

WIRE_FILL, OUT_FILL, MSG_FILL = 0xA5, 0x5A, 0xC3
MODES = {"auto": 0, "lane": 1, "wave": 2, "bp": 3}


def _pmd():
    import torch  # noqa: F401
    from beast_amd import pmd
    return pmd


@pytest.fixture(params=["auto", "lane", "wave"])
def inflate_kernel(request):
    pmd = _pmd()
    assert pmd.lib().bpmd_set_inflate_kernel(MODES[request.param]) == 0
    yield request.param
    pmd.lib().bpmd_set_inflate_kernel(0)


@pytest.fixture(params=["lane", "wave", "bp"])
def decoder(request):
    pmd = _pmd()
    assert pmd.lib().bpmd_set_inflate_kernel(MODES[request.param]) == 0
    yield request.param
    pmd.lib().bpmd_set_inflate_kernel(0)


def _ragged(caps, rng, residue=None):
    """slot offsets with 1-19 guard bytes before each; residue: every offset = residue mod 16"""
    offs, pos = [], 0
    for c in caps:
        pos += rng.randrange(1, 20)
        if residue is not None:
            pos += (residue - pos) % 16
        offs.append(pos)
        pos += c
    return offs, pos + 64


class Got:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Rig:
    """n connections' out and message slots at ragged offsets in two buffers,
    their message states, and the model's copy of all three."""

    def __init__(self, out_caps, msg_caps, rng, residue=None):
        self.rng = rng
        self.caps, self.mcaps = list(out_caps), list(msg_caps)
        self.offs, total = _ragged(self.caps, rng, residue)
        self.moffs, mtotal = _ragged(self.mcaps, rng, residue)
        self.out = bytearray([OUT_FILL]) * total
        self.msg = bytearray([MSG_FILL]) * mtotal
        self.state = bytearray(16 * len(self.caps))
        self.m_state = [FM.State() for _ in self.caps]
        self.m_slot = [bytearray([OUT_FILL]) * c for c in self.caps]
        self.m_msg = [bytearray([MSG_FILL]) * c for c in self.mcaps]

    def call(self, bufs, role, pmd_on=True, msg_max=16 << 20, stream=None):
        """One bpmd_receive_batch over bufs (one wire buffer per slot), compared
        entry by entry with the model and buffer by buffer with what the
        model's results alone write; returns (device results, model results)."""
        import torch
        pmd = _pmd()
        n = len(bufs)
        assert n == len(self.caps)
        woffs, wtotal = _ragged([len(b) for b in bufs], self.rng)
        wire = bytearray([WIRE_FILL]) * wtotal
        for o, b in zip(woffs, bufs):
            wire[o:o + len(b)] = b
        dev = "cuda"
        t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)  # noqa: E731
        t32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
        wb = pmd.Batch(torch.frombuffer(bytearray(wire), dtype=torch.uint8).to(dev), t64(woffs),
                       t32([len(b) for b in bufs]))
        out = torch.frombuffer(bytearray(self.out), dtype=torch.uint8).to(dev)
        msg = torch.frombuffer(bytearray(self.msg), dtype=torch.uint8).to(dev)
        st = torch.frombuffer(bytearray(self.state), dtype=torch.uint8).to(dev).reshape(n, 16)
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        r = pmd.recv_batch(wb, t32(self.caps), t32(self.mcaps), role, pmd_on, msg_max, state=st, out=out,
                           out_off=t64(self.offs), msg=msg, msg_off=t64(self.moffs), stream=stream)
        torch.cuda.synchronize()
        assert wb.data.cpu().numpy().tobytes() == bytes(wire), "the wire was modified"
        self.out = bytearray(out.cpu().numpy().tobytes())
        got_msg = bytearray(msg.cpu().numpy().tobytes()) if pmd_on else self.msg
        self.state = bytearray(st.cpu().numpy().tobytes())
        u = r.frames
        ev, stt, con = r.event.cpu().tolist(), r.status.cpu().tolist(), u.consumed.cpu().tolist()
        ol, op, comp = u.out.len.cpu().tolist(), u.op.cpu().tolist(), u.compressed.cpu().tolist()
        ctl, cl, code = u.ctl.cpu().numpy(), u.ctl_len.cpu().tolist(), u.close_code.cpu().tolist()
        ml = r.msg.len.cpu().tolist()
        assert r.status is u.status and r.event is u.event
        got, want = [], []
        expect_msg = bytearray([MSG_FILL]) * len(self.msg)
        for i, b in enumerate(bufs):
            e = M.receive(b, role, pmd_on, msg_max, self.caps[i], self.mcaps[i], self.m_state[i], self.m_slot[i])
            g = Got(event=ev[i], status=stt[i], consumed=con[i], out_len=ol[i], op=op[i], compressed=comp[i],
                    ctl=ctl[i, :cl[i]].tobytes(), close_code=code[i], state=bytes(self.state[16 * i:16 * i + 16]),
                    msg_len=ml[i])
            s = e.stop
            assert (g.event, g.status, g.consumed, g.out_len, g.op, g.compressed, g.ctl, g.close_code, g.state,
                    g.msg_len) == (s.event, e.status, s.consumed, s.out_len, s.op, s.compressed, s.ctl, s.close_code,
                                   s.state, e.msg_len), (i, b[:40].hex(), g.__dict__, e)
            mo = self.moffs[i]
            if e.inflated is not None:
                assert len(e.inflated) <= e.eff_cap <= self.mcaps[i]
                self.m_msg[i][:len(e.inflated)] = e.inflated
                # the inflater's scratch inside its capacity (see the module's docstring)
                self.m_msg[i][len(e.inflated):e.eff_cap] = got_msg[mo + len(e.inflated):mo + e.eff_cap]
            expect_msg[mo:mo + self.mcaps[i]] = self.m_msg[i]
            g.message = None
            if g.event == FM.EV_MESSAGE and g.status in (0, M.BAD_FRAME_PAYLOAD):
                g.message = bytes(got_msg[mo:mo + g.msg_len]) if g.compressed else \
                    bytes(self.out[self.offs[i]:self.offs[i] + g.msg_len])
            assert g.message == e.message, i
            got.append(g)
            want.append(e)
        expect_out = bytearray([OUT_FILL]) * len(self.out)
        for o, s in zip(self.offs, self.m_slot):
            expect_out[o:o + len(s)] = s
        assert self.out == expect_out, "out buffer differs from the gathered payloads"
        assert got_msg == expect_msg, "msg buffer differs from the inflated messages"
        self.msg = got_msg
        self.last = r
        return got, want


def _wire(payload, op, comp, masked, rng, frame_max=1000):
    nf = max(1, -(-len(payload) // frame_max))
    keys = [rng.getrandbits(32) for _ in range(nf)] if masked else None
    return O.frame_write(payload, op, comp, keys=keys, frame_max=frame_max)


def _mixed(rng, n, max_len):
    """(plain, op, compressed, payload): JSON messages, 30 % with one byte that is not UTF-8"""
    plain = _json_messages(n, rng, max_len)
    out = []
    for m in plain:
        op, comp, bad = rng.choice([1, 2]), rng.random() < 0.5, rng.random() < 0.3
        if bad and m:
            b = bytearray(m)
            b[rng.randrange(len(b))] = rng.choice([0x80, 0xC0, 0xFF])
            m = bytes(b)
        out.append((m, op, comp, O.pmd_deflate(m, 6, 15, 4) if comp else m))
    return out


@pytest.mark.parametrize("masked", [True, False])
def test_mixed_batch_entry_by_entry(inflate_kernel, masked):
    """240 entries: compressed and plain, text and binary, 30 % not UTF-8,
    lengths 0, 1 and up to 3000 in 1000-byte frames; every 17th cut one byte
    short, every 13th stopped by a ping or a close between its fragments."""
    rng = random.Random(31)
    key = (lambda: rng.getrandbits(32)) if masked else (lambda: None)
    msgs = _mixed(rng, 240, 3000)
    bufs = []
    for i, (m, op, comp, payload) in enumerate(msgs):
        if i % 13 == 7:
            h = len(payload) // 2
            ctl = FM.frame(b"still there?", 9, key=key()) if i % 2 else \
                FM.frame((1001).to_bytes(2, "big") + b"bye", 8, key=key())
            w = FM.frame(payload[:h], op, fin=False, rsv=4 if comp else 0, key=key()) + ctl + \
                FM.frame(payload[h:], 0, key=key())
        else:
            w = _wire(payload, op, comp, masked, rng)
        bufs.append(w[:-1] if i % 17 == 5 else w)
    rig = Rig([3100] * len(msgs), [3000 + (i % 3) for i in range(len(msgs))], rng)
    got, want = rig.call(bufs, FM.SERVER if masked else FM.CLIENT)
    seen = {(g.event, g.status, g.compressed, g.op) for g in got}
    for comp in (0, 1):   # every kind occurred
        assert {(FM.EV_MESSAGE, 0, comp, 1), (FM.EV_MESSAGE, 0, comp, 2), (FM.EV_MESSAGE, M.BAD_FRAME_PAYLOAD, comp, 1)} \
            <= seen
    assert {FM.EV_NEED_MORE, FM.EV_PING, FM.EV_CLOSE} <= {g.event for g in got}
    for i, (g, (m, op, comp, _)) in enumerate(zip(got, msgs)):
        if g.event == FM.EV_MESSAGE:
            assert (g.message, g.op, g.compressed, g.consumed) == (m, op, int(comp), len(bufs[i])), i
        else:   # not inflated: the msg slot still holds the canary (Rig.call compared the whole buffer)
            assert g.msg_len == 0 and rig.m_msg[i] == bytearray([MSG_FILL]) * rig.mcaps[i]
    assert rig.last.to_host() == [e.message for e in want]


def test_equals_the_chain_it_replaces(inflate_kernel):
    """pmd.recv_batch and pmd.receive_batch on the same wires: the all-text
    compressed batch of test_gpu_unframe's end-to-end test, and its mixed
    one."""
    import torch
    pmd = _pmd()
    rng = random.Random(7)
    msgs = _json_messages(512, rng)
    z = pmd.deflate_batch(pmd.Batch.from_host(msgs), level=6)
    nk = int(pmd.frame_counts(z.out.len, 1000).sum().item())
    wire = pmd.frame_batch(z.out, 1000, op=1, compressed=True, keys=[rng.getrandbits(32) for _ in range(nk)])
    cap = int(z.out.len.max().item())
    old = pmd.receive_batch(wire, cap, 6000, pmd.ROLE_SERVER)
    new = pmd.recv_batch(wire, cap, 6000, pmd.ROLE_SERVER)
    torch.cuda.synchronize()
    assert new.event.cpu().tolist() == old.event.cpu().tolist() == [pmd.EV_MESSAGE] * len(msgs)
    assert new.status.cpu().tolist() == old.status.cpu().tolist() == [0] * len(msgs)
    assert new.frames.consumed.cpu().tolist() == wire.len.cpu().tolist()
    assert new.to_host() == old.to_host() == msgs

    rng = random.Random(8)
    mixed = _mixed(rng, 240, 3000)
    src = pmd.Batch.from_host([p for _, _, _, p in mixed])
    nk = int(pmd.frame_counts(src.len, 1000).sum().item())
    wire = pmd.frame_batch(src, 1000, op=torch.tensor([k[1] for k in mixed], dtype=torch.uint8),
                           compressed=torch.tensor([int(k[2]) for k in mixed], dtype=torch.uint8),
                           keys=[rng.getrandbits(32) for _ in range(nk)])
    cut = [i for i in range(len(mixed)) if i % 17 == 5]
    wire.len[cut] -= 1
    old = pmd.receive_batch(wire, 3100, 3000, pmd.ROLE_SERVER)
    new = pmd.recv_batch(wire, 3100, 3000, pmd.ROLE_SERVER)
    torch.cuda.synchronize()
    assert new.event.cpu().tolist() == old.event.cpu().tolist()
    assert new.status.cpu().tolist() == old.status.cpu().tolist()
    assert pmd.BAD_FRAME_PAYLOAD in new.status.cpu().tolist()
    got = new.to_host()
    assert got == old.to_host()
    assert [g for i, g in enumerate(got) if i not in cut] == [m for i, (m, _, _, _) in enumerate(mixed) if i not in cut]


@pytest.mark.parametrize("length", [600, 5000])
def test_msg_max_on_the_inflated_size(decoder, length):
    """rd_msg_max on the inflated size: every msg_max in {len - 2 .. len + 2,
    0} x msg_cap in {len - 1, len, len + 1, len + 8}, text and binary, and the
    same with a payload whose first block header is damaged (the zlib error
    comes before any limit and wins) or whose middle is (the model decides)."""
    rng = random.Random(41)
    text = _json_messages(3, rng, length)[2]
    assert len(text) == length and O.utf8_check(text) == 0
    z = O.pmd_deflate(text, 6, 15, 4)
    head = bytearray(z)
    head[0] |= 6                       # block type 3
    mid = bytearray(z)
    mid[len(z) // 2] ^= 0x10
    bad_head = O.pmd_inflate(bytes(head), length + 8)
    assert 1 < bad_head[0] < 17 and bad_head[1] == b""   # a zlib error before the first output byte
    caps = [length - 1, length, length + 1, length + 8]
    cases = [(op, cap, p) for op in (1, 2) for cap in caps for p in (z, bytes(head), bytes(mid))]
    bufs = [FM.frame(p, op, rsv=4) for op, _, p in cases]
    seen = set()
    for msg_max in [length - 2, length - 1, length, length + 1, length + 2, 0]:
        rig = Rig([len(z)] * len(cases), [c for _, c, _ in cases], rng)
        got, want = rig.call(bufs, FM.CLIENT, msg_max=msg_max)
        for g, e, (op, cap, p) in zip(got, want, cases):
            over_max, over_cap = bool(msg_max) and length > msg_max, length > cap
            if p is z:   # the rule, spelled out
                rule = (FM.ERR["message_too_big"] if msg_max <= cap else FM.ERR["buffer_overflow"]) if over_max else \
                    FM.ERR["buffer_overflow"] if over_cap else 0
                assert g.status == rule, (msg_max, cap, op)
                eff = min(cap, msg_max + 1) if msg_max else cap
                assert g.msg_len == min(length, eff) == len(O.pmd_inflate(z, eff)[1])
                assert g.message == (text if rule == 0 else None)
            elif p == bytes(head):
                assert (g.status, g.msg_len, g.message) == (bad_head[0], 0, None), (msg_max, cap, op)
            seen.add(g.status)
    assert {0, FM.ERR["message_too_big"], FM.ERR["buffer_overflow"], bad_head[0]} <= seen


def test_several_calls_with_state(inflate_kernel):
    """Three short compressed messages in fragments with controls between
    them; entry k of each starts with the k-byte prefix of the wire, drops
    what was consumed and continues with the rest until done.  Every call is
    compared with the model (events, statuses, state, the gathered bytes
    surviving between calls); each entry ends with the whole wire's events."""
    rng = random.Random(51)
    texts = [("grüße aus der ferne " * 8).encode(), b"binary \x00\xff\xfe payload " * 6,
             ("κόσμε" * 20).encode()[:-1]]            # the last stops inside a code point
    for t, op, masked in zip(texts, (1, 2, 1), (True, False, True)):
        key = (lambda: rng.getrandbits(32)) if masked else (lambda: None)
        z = O.pmd_deflate(t, 6, 15, 4)
        a, b = len(z) // 3, 2 * len(z) // 3
        wire = FM.frame(z[:a], op, fin=False, rsv=4, key=key()) + FM.frame(b"are you there", 9, key=key()) + \
            FM.frame(z[a:b], 0, fin=False, key=key()) + FM.frame(b"", 10, key=key()) + FM.frame(z[b:], 0, key=key())
        assert len(wire) <= 260
        role = FM.SERVER if masked else FM.CLIENT
        n = len(wire) + 1
        rig = Rig([len(z)] * n, [len(t)] * n, rng)
        got, _ = rig.call([wire[:j] for j in range(n)], role)
        seq = [[g] for g in got]
        rest = [wire[g.consumed:] for g in got]
        for _ in range(6):
            got, _ = rig.call(rest, role)
            for j, g in enumerate(got):
                if g.consumed:
                    seq[j].append(g)
                rest[j] = rest[j][g.consumed:]
            if all(g.consumed == 0 for g in got):
                break
        final = M.BAD_FRAME_PAYLOAD if op == 1 and O.utf8_check(t) else 0
        for j in range(n):
            stops = [g for g in seq[j] if g.event != FM.EV_NEED_MORE]
            assert [(g.event, g.status) for g in stops] == [(FM.EV_PING, 0), (FM.EV_PONG, 0), (FM.EV_MESSAGE, final)], j
            assert rest[j] == b"" and stops[0].ctl == b"are you there"
            assert (stops[2].message, stops[2].msg_len, stops[2].compressed) == (t, len(t), 1), j


def _utf8_sequences():
    """from the reference's own cases: two that write() rejects, two that only
    finish() rejects, one valid four-byte code point"""
    by = {0: [], 1: [], 2: []}
    for data, verdict in utf8_cases.prefixes():
        if verdict is not None and len(data) <= 4 and data not in by[verdict]:
            by[verdict].append(data)
    inv = [d for d in by[2] if len(d) == 1][:1] + [d for d in by[2] if len(d) == 3][:1]
    inc = [d for d in by[1] if d[0] < 0xE0][:1] + [d for d in by[1] if d[0] >= 0xF0][:1]
    val = [d for d in by[0] if len(d) == 4][:1]
    assert len(inv) == 2 and len(inc) == 2 and len(val) == 1
    return inv + inc + val


@pytest.mark.parametrize("residue", range(16))
def test_utf8_source_and_edges(inflate_kernel, residue):
    """Plain and compressed text whose invalid or incomplete code point sits at
    byte 0, at the unit edges 15 / 16 / 17 and at the wave-step edges 1023 /
    1024 / 1025, as the last bytes and before a tail, the slot at one residue
    mod 16 per case: the check reads the slot that holds the message."""
    rng = random.Random(61 + residue)
    cases = []
    for seq in _utf8_sequences():
        for pos in (0, 15, 16, 17, 1023, 1024, 1025):
            for tail in (b"", b"~" * 40):
                t = b"a" * pos + seq + tail
                for comp in (False, True):
                    cases.append((t, comp))
    bufs = [FM.frame(O.pmd_deflate(t, 6, 15, 4) if comp else t, 1, rsv=4 if comp else 0) for t, comp in cases]
    rig = Rig([len(t) + 16 for t, _ in cases], [len(t) for t, _ in cases], rng, residue=residue)
    assert all(o % 16 == residue for o in rig.offs + rig.moffs)
    got, _ = rig.call(bufs, FM.CLIENT)
    for g, (t, comp) in zip(got, cases):
        want = M.BAD_FRAME_PAYLOAD if O.utf8_check(t) else 0
        assert (g.event, g.status, g.compressed, g.message) == (FM.EV_MESSAGE, want, int(comp), t)
    assert {g.status for g in got} == {0, M.BAD_FRAME_PAYLOAD}
    # the verdict follows the slot that holds the message: a compressed message whose gathered
    # (deflated) bytes are not UTF-8 but whose text is, passes; one byte that is not UTF-8 in
    # the text fails whatever the deflated bytes look like (both kinds are among the cases)
    assert any(O.utf8_check(O.pmd_deflate(t, 6, 15, 4)) and not O.utf8_check(t) for t, c in cases if c)


@pytest.mark.parametrize("n", [2048, 32768])
def test_tiny_entries_on_each_plan(n):
    """Automatic mode at the sizes where the inflate plan changes (lanes from
    2048 messages, no split from 32 Ki): only every 3rd entry completes a
    compressed message, the others reach the inflater with length 0."""
    import torch
    pmd = _pmd()
    assert pmd.lib().bpmd_set_inflate_kernel(0) == 0
    texts = [b"", b"a", b"hello hello hello hello", "zwölf boxkämpfer".encode(), b"not utf-8 \xff"]
    zs = [FM.frame(O.pmd_deflate(t, 6, 15, 4), 1, rsv=4) for t in texts]
    others = [FM.frame(b"plain text", 1), FM.frame(b"\xffbinary", 2), FM.frame(b"plain \xc3", 1), FM.frame(b"ping", 9),
              zs[2][:-1], FM.frame(b"abc", 1, rsv=2), FM.frame(zs[2][2:], 2, fin=False, rsv=4)]
    bufs = [zs[(i // 3) % len(zs)] if i % 3 == 0 else others[(i // 3 * 2 + i % 3) % len(others)] for i in range(n)]
    OUT_CAP, MSG_CAP, W = 32, 24, 48
    kinds = {}
    for b in set(bufs):
        slot = bytearray([OUT_FILL]) * OUT_CAP
        kinds[b] = (M.receive(b, FM.CLIENT, True, 20, OUT_CAP, MSG_CAP, FM.State(), slot), slot)
    wire = np.full(n * W + 16, WIRE_FILL, np.uint8)
    for i, b in enumerate(bufs):
        wire[i * W:i * W + len(b)] = np.frombuffer(b, np.uint8)
    wb = pmd.Batch(torch.from_numpy(wire.copy()).cuda(), torch.arange(n, dtype=torch.int64, device="cuda") * W,
                   torch.tensor([len(b) for b in bufs], dtype=torch.int32, device="cuda"))
    out = torch.full((n * OUT_CAP + 16,), OUT_FILL, dtype=torch.uint8, device="cuda")
    msg = torch.full((n * 32 + 16,), MSG_FILL, dtype=torch.uint8, device="cuda")
    # one capacity for all: recv_batch lays the slots out itself, 16-byte aligned (24 -> stride 32)
    r = pmd.recv_batch(wb, OUT_CAP, MSG_CAP, pmd.ROLE_CLIENT, msg_max=20, out=out, msg=msg)
    torch.cuda.synchronize()
    assert r.msg.off.tolist()[:3] == [0, 32, 64] and r.frames.out.off.tolist()[:3] == [0, 32, 64]
    assert wb.data.cpu().numpy().tobytes() == wire.tobytes()
    exp = [kinds[b][0] for b in bufs]
    assert r.event.cpu().tolist() == [e.stop.event for e in exp]
    assert r.status.cpu().tolist() == [e.status for e in exp]
    assert r.msg.len.cpu().tolist() == [e.msg_len for e in exp]
    assert r.frames.out.len.cpu().tolist() == [e.stop.out_len for e in exp]
    assert r.frames.consumed.cpu().tolist() == [e.stop.consumed for e in exp]
    assert r.frames.compressed.cpu().tolist() == [e.stop.compressed for e in exp]
    # the model saw a limit, an overflow-free fit, text that is not UTF-8, and entries that are not messages
    assert {FM.ERR["message_too_big"], M.BAD_FRAME_PAYLOAD, 0, FM.ERR["bad_reserved_bits"]} <= {e.status for e in exp}
    assert sum(e.inflated is not None for e in exp) == (n + 2) // 3
    got_msg = msg.cpu().numpy()
    want_msg = np.full(n * 32 + 16, MSG_FILL, np.uint8)
    want_out = np.full(n * OUT_CAP + 16, OUT_FILL, np.uint8)
    for i, b in enumerate(bufs):
        e, slot = kinds[b]
        want_out[i * OUT_CAP:(i + 1) * OUT_CAP] = np.frombuffer(bytes(slot), np.uint8)
        if e.inflated is not None:
            k = len(e.inflated)
            want_msg[i * 32:i * 32 + k] = np.frombuffer(e.inflated, np.uint8)
            want_msg[i * 32 + k:i * 32 + e.eff_cap] = got_msg[i * 32 + k:i * 32 + e.eff_cap]   # the inflater's scratch
    assert np.array_equal(out.cpu().numpy(), want_out)
    assert np.array_equal(got_msg, want_msg)


def test_permessage_deflate_off_needs_no_inflater_arguments():
    """pmd_on == 0 with NULL cfg, d_msg, d_msg_off, d_msg_cap and d_work (what
    pmd.recv_batch passes then): plain messages are checked, RSV1 is refused by
    the frame pass."""
    rng = random.Random(71)
    bufs = [FM.frame(b"plain", 1), FM.frame("grüße".encode(), 1), FM.frame(b"caf\xe9", 1), FM.frame(b"caf\xe9", 2),
            FM.frame(O.pmd_deflate(b"hello", 6, 15, 4), 1, rsv=4), FM.frame(b"", 1), FM.frame(b"x" * 300 + b"\xc3", 1),
            FM.frame(b"he", 1, fin=False) + FM.frame(b"llo", 0), FM.frame(b"p", 9)]
    rig = Rig([400] * len(bufs), [0] * len(bufs), rng)
    got, _ = rig.call(bufs, FM.CLIENT, pmd_on=False)
    assert [(g.event, g.status, g.msg_len) for g in got] == \
        [(1, 0, 5), (1, 0, 7), (1, M.BAD_FRAME_PAYLOAD, 4), (1, 0, 4), (0, FM.ERR["bad_reserved_bits"], 0), (1, 0, 0),
         (1, M.BAD_FRAME_PAYLOAD, 301), (1, 0, 5), (FM.EV_PING, 0, 0)]
    assert rig.last.msg.data.numel() == 0 and got[7].message == b"hello"
    # the C call itself, with d_msg_len NULL as well
    import torch
    pmd = _pmd()
    L = pmd._recv_lib()
    wb = pmd.Batch.from_host(bufs)
    n = len(bufs)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")  # noqa: E731
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    out, off, cap = u8(n * 400 + 16), torch.arange(n, dtype=torch.int64, device="cuda") * 400, i32() + 400
    out_len, op, comp, ev, status, consumed = i32(), u8(n), u8(n), u8(n), i32(), i32()
    ctl, ctl_len, code = u8(n, 128), u8(n), torch.zeros(n, dtype=torch.int16, device="cuda")
    p = pmd._ptr
    assert L.bpmd_receive_batch(None, pmd.ROLE_CLIENT, 0, 0, p(wb.data), p(wb.off), p(wb.len), n, None, p(out), p(off),
                                p(cap), p(out_len), p(op), p(comp), p(ev), p(status), p(consumed), p(ctl), p(ctl_len),
                                p(code), None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [g.status for g in got] and ev.tolist() == [g.event for g in got]


def test_argument_errors_and_empty_batches():
    import torch
    pmd = _pmd()
    L = pmd._recv_lib()
    empty = pmd.Batch(torch.empty(16, dtype=torch.uint8, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"),
                      torch.empty(0, dtype=torch.int32, device="cuda"))
    r = pmd.recv_batch(empty, 16, 16, pmd.ROLE_SERVER)
    assert r.event.numel() == 0 and r.msg.len.numel() == 0 and r.to_host() == []
    assert pmd.recv_batch(empty, 16, 16, pmd.ROLE_CLIENT, pmd_on=False).status.numel() == 0
    with pytest.raises(pmd.BpmdError):
        pmd.recv_batch(empty, 16, 16, 2)
    with pytest.raises(pmd.BpmdError):
        pmd.recv_batch(empty, 16, 16, pmd.ROLE_SERVER, window_bits=7)
    one = pmd.Batch.from_host([FM.frame(b"hello", 1)])
    caps = torch.tensor([8], dtype=torch.int32, device="cuda")
    with pytest.raises(pmd.BpmdError):   # capacities on the device: the call would have to wait to size a buffer
        pmd.recv_batch(one, caps, 8, pmd.ROLE_CLIENT)
    with pytest.raises(pmd.BpmdError):
        pmd.recv_batch(one, 8, caps, pmd.ROLE_CLIENT)
    with pytest.raises(pmd.BpmdError):
        pmd.recv_batch(one, 8, 8, pmd.ROLE_CLIENT, state=torch.zeros(3, dtype=torch.uint8, device="cuda"))
    r = pmd.recv_batch(one, 8, 8, pmd.ROLE_CLIENT)
    torch.cuda.synchronize()
    assert r.to_host() == [b"hello"] and r.msg.len.tolist() == [5]
    # the C call: BPMD_F_RAW and a missing workspace are refused with everything else in place
    cfg = pmd._Cfg(0, 15, 8, 0, pmd.F_RAW)
    f, p = r.frames, pmd._ptr
    work = torch.empty(int(L.bpmd_receive_work_bytes(1)), dtype=torch.uint8, device="cuda")
    code = torch.zeros(1, dtype=torch.int16, device="cuda")

    def call(cfg, work):
        return L.bpmd_receive_batch(ctypes.byref(cfg), pmd.ROLE_CLIENT, 1, 0, p(one.data), p(one.off), p(one.len), 1,
                                    None, p(f.out.data), p(f.out.off), p(f.cap), p(f.out.len), p(f.op), p(f.compressed),
                                    p(f.event), p(f.status), p(f.consumed), p(f.ctl), p(f.ctl_len), p(code),
                                    p(r.msg.data), p(r.msg.off), p(f.cap), p(r.msg.len), work, None)

    assert call(cfg, p(work)) == -1
    assert call(pmd._Cfg(0, 15, 8, 0, 0), None) == -1
    assert call(pmd._Cfg(0, 15, 8, 0, 0), p(work)) == 0
    torch.cuda.synchronize()


def test_the_call_reads_nothing_back():
    """As tests/test_gpu_async.py: behind long copies queued on the stream, the
    call returns while they still run.  2 048 binary messages of 64 KiB in
    masked 4 KiB frames (block-parallel inflate); the stream's decode
    workspace is reserved first, so that the documented wait of a stream's
    first block-parallel call is not what is seen."""
    from beast_amd import synth
    torch, pmd, dev, big, big2 = _setup()
    raw, off, ln = synth.make_batch("binary", np.full(2048, 65536, np.uint32), seed=0x5EED0058)
    src = pmd.Batch.from_arrays(raw, off.astype(np.int64), ln.astype(np.int32))
    d = pmd.deflate_batch(src, level=1)
    rng = random.Random(81)
    nk = int(pmd.frame_counts(d.out.len, 4096).sum().item())
    wire = pmd.frame_batch(d.out, 4096, op=2, compressed=True, keys=[rng.getrandbits(32) for _ in range(nk)])
    cap = torch.from_numpy(ln.astype(np.int32)).to(dev)
    gathered = torch.empty_like(d.out.data)
    msg = torch.empty_like(src.data)
    pmd.inflate_reserve(int(d.out.len.sum()), int(ln.sum()), 2048)

    def call():   # every buffer given: the wrapper itself never waits
        return pmd.recv_batch(wire, d.cap, cap, pmd.ROLE_SERVER, out=gathered, out_off=d.out.off, msg=msg,
                              msg_off=src.off)

    for _ in range(3):   # the stream's pools reach this batch's size
        r = call()
    torch.cuda.synchronize()
    assert int((r.status != 0).sum()) == 0 and int((r.event != pmd.EV_MESSAGE).sum()) == 0
    assert torch.equal(msg, src.data) and torch.equal(r.msg.len, src.len)
    assert not _call_behind_copies(torch, call, big, big2), "the call waited for the queued copies"
