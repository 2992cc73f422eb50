"""bpmd_unframe_batch and pmd.receive_batch on the GPU: the receive side from
wire bytes to message payloads, against tests/frame_parse_model.py (Beast's
parse_fh / read_close restated), the known answers of
tests/golden/frame_parse_kat.json, the oracle's framer O.frame_write and the
library's own bpmd_frame_batch.  Entries lie at ragged offsets with guard
bytes between them, out slots likewise; after every call the wire must be
unchanged and the whole out buffer equal to what the expected payloads alone
would have written."""
import random

import numpy as np
import pytest

from beast_amd import synth
from oracle import oracle as O
from tests import frame_parse_model as M
from tests.test_frame_parse import EVENTS, load_kats

pytestmark = pytest.mark.gpu

LENS = [0, 1, 3, 4, 5, 15, 16, 17, 31, 125, 126, 127, 4096, 65535, 65536, 70001]
FRAME_MAX = [5, 16, 125, 126, 4096, 65536]
WIRE_FILL, OUT_FILL = 0xA5, 0x5A


def _pmd():
    import torch  # noqa: F401
    from beast_amd import pmd
    return pmd


@pytest.fixture(params=["lane", "wave"])
def inflate_kernel(request):
    pmd = _pmd()
    assert pmd.lib().bpmd_set_inflate_kernel({"lane": 1, "wave": 2}[request.param]) == 0
    yield request.param
    pmd.lib().bpmd_set_inflate_kernel(0)


def shapes():
    """(payload length, frame_max) of the round-trip tests"""
    return [(n, f) for n in LENS for f in FRAME_MAX] + [(n, 1) for n in LENS if n <= 300]


class Slots:
    """n connections' out slots at ragged offsets in one buffer, their message
    states, and the model's copy of both."""

    def __init__(self, caps, rng, with_state=True):
        self.caps = list(caps)
        self.offs, pos = [], 0
        for c in self.caps:
            pos += rng.randrange(1, 20)
            self.offs.append(pos)
            pos += c
        self.out = bytearray([OUT_FILL]) * (pos + 64)
        self.with_state = with_state
        self.state = bytearray(16 * len(self.caps))
        self.m_state = [M.State() for _ in self.caps]
        self.m_slot = [bytearray([OUT_FILL]) * c for c in self.caps]

    def expected_out(self):
        buf = bytearray([OUT_FILL]) * len(self.out)
        for o, s in zip(self.offs, self.m_slot):
            buf[o:o + len(s)] = s
        return buf

    def call(self, bufs, role, pmd_on=True, msg_max=16 << 20, stream=None):
        """One bpmd_unframe_batch over bufs (one wire buffer per slot); returns
        [M.Stop] as the device reported them and updates out and state."""
        import torch
        pmd = _pmd()
        n = len(bufs)
        assert n == len(self.caps)
        woffs, pos = [], 0
        for b in bufs:
            pos += rng_gap(pos)
            woffs.append(pos)
            pos += len(b)
        wire = bytearray([WIRE_FILL]) * (pos + 64)
        for o, b in zip(woffs, bufs):
            wire[o:o + len(b)] = b
        dev = "cuda"
        wb = pmd.Batch(torch.frombuffer(bytearray(wire), dtype=torch.uint8).to(dev),
                       torch.tensor(woffs, dtype=torch.int64, device=dev),
                       torch.tensor([len(b) for b in bufs], dtype=torch.int32, device=dev))
        out = torch.frombuffer(bytearray(self.out), dtype=torch.uint8).to(dev)
        st = torch.frombuffer(bytearray(self.state), dtype=torch.uint8).to(dev).reshape(n, 16) if self.with_state \
            else None
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        u = pmd.unframe_batch(wb, torch.tensor(self.caps, dtype=torch.int32, device=dev), role, pmd_on, msg_max,
                              state=st, out=out, out_off=torch.tensor(self.offs, dtype=torch.int64, device=dev),
                              stream=stream)
        torch.cuda.synchronize()
        assert wb.data.cpu().numpy().tobytes() == bytes(wire), "the wire was modified"
        self.out = bytearray(out.cpu().numpy().tobytes())
        if self.with_state:
            self.state = bytearray(st.cpu().numpy().tobytes())
        ev, stt, con = u.event.cpu().tolist(), u.status.cpu().tolist(), u.consumed.cpu().tolist()
        ol, op, comp = u.out.len.cpu().tolist(), u.op.cpu().tolist(), u.compressed.cpu().tolist()
        ctl, cl, code = u.ctl.cpu().numpy(), u.ctl_len.cpu().tolist(), u.close_code.cpu().tolist()
        return [M.Stop(ev[i], stt[i], con[i], ol[i], op[i], comp[i], ctl[i, :cl[i]].tobytes(), code[i],
                       bytes(self.state[16 * i:16 * i + 16]) if self.with_state else bytes(16)) for i in range(n)]

    def call_checked(self, bufs, role, pmd_on=True, msg_max=16 << 20, stream=None):
        """call(), compared entry by entry with the model's walk; returns the stops"""
        got = self.call(bufs, role, pmd_on, msg_max, stream)
        for i, b in enumerate(bufs):
            st = self.m_state[i] if self.with_state else M.State()
            want = M.walk(b, role, pmd_on, msg_max, self.caps[i], st, self.m_slot[i])
            if not self.with_state:
                want.state = bytes(16)
            assert got[i] == want, (i, b[:40].hex(), got[i], want)
        assert self.out == self.expected_out(), "out buffer differs from the gathered payloads"
        return got

    def message(self, i, n):
        return bytes(self.out[self.offs[i]:self.offs[i] + n])


_gap = random.Random(99)


def rng_gap(pos):
    return _gap.randrange(0, 20)


def test_known_answers():
    """Every KAT as one batch; chopped cases continue with what the first
    call left plus the next part."""
    cases = load_kats()
    rng = random.Random(1)
    for role in (0, 1):
        for pmd_on in (False, True):
            sel = [c for c in cases if c["role"] == role and c["pmd_on"] == pmd_on]
            if not sel:
                continue
            s = Slots([c.get("out_cap", 4096) for c in sel], rng)
            rest = [b""] * len(sel)
            for k in range(max(len(c["parts"]) for c in sel)):
                live = [k < len(c["parts"]) for c in sel]
                bufs = [rest[i] + bytes.fromhex(c["parts"][k]) if live[i] else b"" for i, c in enumerate(sel)]
                got = s.call_checked(bufs, role, pmd_on)
                for i, c in enumerate(sel):
                    if not live[i]:
                        continue
                    e = c["expect"][k]
                    want = (EVENTS[e["event"]], 0 if e["status"] == "ok" else M.ERR[e["status"]], e["consumed"])
                    assert (got[i].event, got[i].status, got[i].consumed) == want, (c["name"], k)
                    if "close_code" in e:
                        assert got[i].close_code == e["close_code"], c["name"]
                    rest[i] = bufs[i][got[i].consumed:]


def _round_trip_corpus(rng):
    msgs = []
    for rep in range(6):
        for n, fmax in shapes():
            msgs.append((rng.randbytes(n), rng.choice([1, 2]), rng.random() < 0.5, fmax))
    return msgs


def _check_messages(s, got, msgs, wires):
    for i, (payload, op, rsv1, _) in enumerate(msgs):
        g = got[i]
        assert (g.event, g.status, g.consumed) == (M.EV_MESSAGE, 0, len(wires[i])), (i, g)
        assert (g.out_len, g.op, g.compressed) == (len(payload), op, int(rsv1)), (i, g)
        assert g.state == bytes(16), i
        s.m_slot[i][:len(payload)] = payload
    assert s.out == s.expected_out()


def test_round_trip_of_the_oracle_framer():
    """~600 messages framed by O.frame_write, masked with random keys for the
    server role and unmasked for the client role."""
    rng = random.Random(2)
    msgs = _round_trip_corpus(rng)
    assert len(msgs) >= 600
    for masked in (True, False):
        wires = []
        for payload, op, rsv1, fmax in msgs:
            nf = max(1, -(-len(payload) // fmax))
            keys = [rng.getrandbits(32) for _ in range(nf)] if masked else None
            wires.append(O.frame_write(payload, op, rsv1, keys=keys, frame_max=fmax))
        s = Slots([len(m[0]) for m in msgs], rng)
        got = s.call(wires, M.SERVER if masked else M.CLIENT)
        _check_messages(s, got, msgs, wires)


def test_frame_batch_then_unframe_batch():
    """bpmd_frame_batch's wire bytes, read back by bpmd_unframe_batch."""
    import torch
    pmd = _pmd()
    rng = random.Random(3)
    for fmax in FRAME_MAX + [1]:
        msgs = [(rng.randbytes(n), rng.choice([1, 2]), rng.random() < 0.5, fmax)
                for n, f in shapes() if f == fmax for _ in range(2)]
        src = pmd.Batch.from_host([m[0] for m in msgs])
        ops = torch.tensor([m[1] for m in msgs], dtype=torch.uint8)
        comp = torch.tensor([int(m[2]) for m in msgs], dtype=torch.uint8)
        for masked in (True, False):
            nk = int(pmd.frame_counts(src.len, fmax).sum().item())
            keys = [rng.getrandbits(32) for _ in range(nk)] if masked else None
            wb = pmd.frame_batch(src, fmax, op=ops, compressed=comp, keys=keys)
            torch.cuda.synchronize()
            wires = wb.to_host()
            s = Slots([len(m[0]) for m in msgs], rng)
            got = s.call(wires, M.SERVER if masked else M.CLIENT)
            _check_messages(s, got, msgs, wires)


def _control(rng, key_fn, allow_close):
    kind = rng.choice([9, 10, 8] if allow_close else [9, 10])
    if kind == 8:
        p = rng.choice([b"", (1000).to_bytes(2, "big") + b"bye", (1001).to_bytes(2, "big"),
                        (1005).to_bytes(2, "big"), b"\x03", (1000).to_bytes(2, "big") + b"\xc3"])
    else:
        p = rng.randbytes(rng.choice([0, 1, 4, 17, 125]))
    return M.frame(p, kind, key=key_fn())


def _stream_with_controls(rng, masked):
    """(wire, payload, op, rsv1): a message in 1-4 fragments with pings, pongs
    and at most one close between and after them; at most 8 events."""
    key_fn = (lambda: rng.getrandbits(32)) if masked else (lambda: None)
    payload = rng.randbytes(rng.choice([0, 1, 20, 126, 300, 5000]))
    op, rsv1 = rng.choice([1, 2]), rng.random() < 0.5
    nfrag = rng.randrange(1, 5)
    cuts = sorted(rng.randrange(len(payload) + 1) for _ in range(nfrag - 1))
    parts = [payload[a:b] for a, b in zip([0] + cuts, cuts + [len(payload)])]
    wire, events, closed = b"", 1, False
    for k, part in enumerate(parts):
        wire += M.frame(part, op if k == 0 else 0, fin=k == nfrag - 1, rsv=4 if (k == 0 and rsv1) else 0, key=key_fn())
        while events < 8 and rng.random() < 0.45:
            c = _control(rng, key_fn, not closed)
            closed = closed or c[0] == 0x88
            wire += c
            events += 1
    return wire, payload, op, rsv1


def _run_to_the_end(s, wires, role, pmd_on=True, msg_max=16 << 20, rounds=9):
    """Repeat the call on every entry's unconsumed rest until nothing moves;
    returns each entry's stops."""
    rest = list(wires)
    seq = [[] for _ in wires]
    for _ in range(rounds):
        got = s.call_checked(rest, role, pmd_on, msg_max)
        for i, g in enumerate(got):
            if g.consumed or not seq[i]:
                seq[i].append(g)
            rest[i] = rest[i][g.consumed:]
        if all(g.consumed == 0 for g in got):
            break
    return seq, rest


def test_control_frames_between_fragments():
    rng = random.Random(4)
    for masked in (True, False):
        streams = [_stream_with_controls(rng, masked) for _ in range(160)]
        s = Slots([len(p) for _, p, _, _ in streams], rng)
        seq, rest = _run_to_the_end(s, [w for w, _, _, _ in streams], M.SERVER if masked else M.CLIENT)
        kinds = set()
        for i, (wire, payload, op, rsv1) in enumerate(streams):
            assert rest[i] == b"", i
            done = [g for g in seq[i] if g.event == M.EV_MESSAGE]
            assert len(done) == 1 and (done[0].out_len, done[0].op, done[0].compressed) == (len(payload), op, int(rsv1))
            assert s.message(i, len(payload)) == payload
            kinds |= {(g.event, g.status) for g in seq[i]}
        assert {M.EV_PING, M.EV_PONG, M.EV_CLOSE} <= {e for e, _ in kinds}
        assert {M.ERR["bad_close_code"], M.ERR["bad_close_size"], M.ERR["bad_close_payload"]} <= {st for _, st in kinds}


def test_every_cut():
    """Entry k is the k-byte prefix of one stream; each then continues with
    the bytes it was not given and ends as the whole stream does."""
    rng = random.Random(5)
    payload = rng.randbytes(170)
    for masked in (True, False):
        k = (lambda: rng.getrandbits(32)) if masked else (lambda: None)
        wire = M.frame(payload[:60], 2, fin=False, rsv=4, key=k()) + M.frame(payload[60:110], 0, fin=False, key=k()) + \
            M.frame(b"are you there", 9, key=k()) + M.frame(payload[110:], 0, fin=True, key=k())
        assert 190 <= len(wire) <= 215
        role = M.SERVER if masked else M.CLIENT
        n = len(wire) + 1
        s = Slots([len(payload)] * n, rng)
        first = s.call_checked([wire[:j] for j in range(n)], role)
        rest = [wire[g.consumed:] for g in first]
        seq, left = _run_to_the_end(s, rest, role)
        for j in range(n):
            stops = [g for g in [first[j]] + seq[j] if g.event != M.EV_NEED_MORE]
            assert [g.event for g in stops] == [M.EV_PING, M.EV_MESSAGE], j
            assert stops[0].ctl == b"are you there" and stops[1].out_len == len(payload) and stops[1].compressed == 1
            assert left[j] == b"" and s.message(j, len(payload)) == payload, j


def _error_corpus(rng):
    """(wire, role, cap): streams with one header byte changed, and the cases
    no single byte gives"""
    out = []
    for _ in range(1900):
        masked = rng.random() < 0.5
        key_fn = (lambda: rng.getrandbits(32)) if masked else (lambda: None)
        frames, cont = [], False
        for _ in range(rng.randrange(1, 5)):
            if rng.random() < 0.3:
                frames.append(_control(rng, key_fn, True))
                continue
            fin = rng.random() < 0.5
            p = rng.randbytes(rng.choice([0, 1, 7, 125, 126, 300]))
            frames.append(M.frame(p, 0 if cont else rng.choice([1, 2]), fin=fin, rsv=0 if cont else rng.choice([0, 4]),
                                  key=key_fn()))
            cont = not fin
        j = rng.randrange(len(frames))
        f = bytearray(frames[j])
        hl = 2 + (2 if (f[1] & 0x7F) == 126 else 0)
        at = rng.randrange(hl)
        f[at] = rng.choice([f[at] ^ (1 << rng.randrange(8)), rng.randrange(256)])
        frames[j] = bytes(f)
        out.append((b"".join(frames), M.SERVER if masked else M.CLIENT, rng.choice([100, 1000, 4096])))
    key = 0x01020304
    for role in (M.SERVER, M.CLIENT):      # the wrong role for well-formed frames
        for k in (None, key):
            out.append((M.frame(b"abc", 1, key=k) + M.frame(b"", 9, key=k), role, 100))
    for k in (None, key):                  # lengths against the slot
        role = M.SERVER if k else M.CLIENT
        for n, cap in ((10, 9), (10, 10), (126, 125), (300, 299)):
            out.append((M.frame(bytes(n), 2, key=k), role, cap))
            out.append((M.frame(bytes(5), 2, fin=False, key=k) + M.frame(bytes(n - 5), 0, key=k), role, cap))
        # a frame announcing 2^63 - 1 bytes, first and as a continuation; 2^63; a non-canonical length
        big = M.frame(b"", 2, key=k, len_form=64)[:2] + ((1 << 63) - 1).to_bytes(8, "big") + (b"\1\2\3\4" if k else b"")
        out.append((big, role, 4096))
        out.append((M.frame(bytes(5), 2, fin=False, key=k) + bytes([0x80]) + big[1:], role, 4096))
        out.append((big[:2] + (1 << 63).to_bytes(8, "big") + big[10:], role, 4096))
        out.append((M.frame(bytes(100), 2, key=k, len_form=16), role, 4096))
        out.append((M.frame(bytes(300), 2, key=k, len_form=64), role, 4096))
    return out


@pytest.mark.parametrize("msg_max", [0, 200])
def test_errors(msg_max):
    """~2 000 streams with one changed header byte, the wrong role, messages
    over msg_max and over the slot, and a 2^63 - 1 length: status, consumed,
    event, state and the bytes gathered before the error equal the model."""
    rng = random.Random(6)
    corpus = _error_corpus(rng)
    assert len(corpus) >= 1900
    seen = set()
    for role in (M.SERVER, M.CLIENT):
        for pmd_on in (True, False):
            sel = [c for c in corpus if c[1] == role][(0 if pmd_on else 1)::2]
            s = Slots([c[2] for c in sel], rng)
            seq, _ = _run_to_the_end(s, [c[0] for c in sel], role, pmd_on, msg_max)
            seen |= {g.status for q in seq for g in q}
    want = {"buffer_overflow", "bad_opcode", "bad_data_frame", "bad_continuation", "bad_reserved_bits",
            "bad_control_fragment", "bad_control_size", "bad_unmasked_frame", "bad_masked_frame", "bad_size"}
    if msg_max:
        want.add("message_too_big")
    assert {M.ERR[e] for e in want} <= seen


def _json_messages(n, rng, max_len=6000):
    lens = [rng.randrange(0, max_len + 1) for _ in range(n)]
    lens[:3] = [0, 1, max_len]
    data, off, ln = synth.make_batch("json", lens, seed=21)
    return [bytes(data[int(off[i]):int(off[i]) + int(ln[i])]) for i in range(n)]


def test_end_to_end(inflate_kernel):
    """deflate_batch -> frame_batch (masked, 1 000-byte frames) ->
    receive_batch gives back the messages."""
    import torch
    pmd = _pmd()
    rng = random.Random(7)
    msgs = _json_messages(512, rng)
    z = pmd.deflate_batch(pmd.Batch.from_host(msgs), level=6)
    assert z.status.cpu().tolist() == [0] * len(msgs)
    nk = int(pmd.frame_counts(z.out.len, 1000).sum().item())
    wire = pmd.frame_batch(z.out, 1000, op=1, compressed=True, keys=[rng.getrandbits(32) for _ in range(nk)])
    cap = int(z.out.len.max().item())
    r = pmd.receive_batch(wire, cap, 6000, pmd.ROLE_SERVER)
    torch.cuda.synchronize()
    assert r.event.cpu().tolist() == [pmd.EV_MESSAGE] * len(msgs)
    assert r.status.cpu().tolist() == [0] * len(msgs)
    assert r.frames.consumed.cpu().tolist() == wire.len.cpu().tolist()
    assert r.to_host() == msgs


def test_end_to_end_mixed(inflate_kernel):
    """Compressed and uncompressed messages, text and binary, some not UTF-8,
    some cut short on the wire: the read_batch statuses, entry by entry."""
    import torch
    pmd = _pmd()
    rng = random.Random(8)
    plain = _json_messages(240, rng, 3000)
    kinds = []
    for i in range(len(plain)):
        op, comp, bad = rng.choice([1, 2]), rng.random() < 0.5, rng.random() < 0.3
        if bad and plain[i]:
            b = bytearray(plain[i])
            b[rng.randrange(len(b))] = rng.choice([0x80, 0xC0, 0xFF])
            plain[i] = bytes(b)
        kinds.append((op, comp))
    payloads = [O.pmd_deflate(m, 6, 15, 4) if c else m for m, (_, c) in zip(plain, kinds)]
    src = pmd.Batch.from_host(payloads)
    nk = int(pmd.frame_counts(src.len, 1000).sum().item())
    wire = pmd.frame_batch(src, 1000, op=torch.tensor([k[0] for k in kinds], dtype=torch.uint8),
                           compressed=torch.tensor([int(k[1]) for k in kinds], dtype=torch.uint8),
                           keys=[rng.getrandbits(32) for _ in range(nk)])
    cut = [i for i in range(len(plain)) if i % 17 == 5]
    wire.len[cut] -= 1
    r = pmd.receive_batch(wire, 3100, 3000, pmd.ROLE_SERVER)
    torch.cuda.synchronize()
    ev, st, got = r.event.cpu().tolist(), r.status.cpu().tolist(), r.to_host()
    for i, m in enumerate(plain):
        if i in cut:
            assert (ev[i], st[i], got[i]) == (pmd.EV_NEED_MORE, 0, None), i
            continue
        want = pmd.BAD_FRAME_PAYLOAD if kinds[i][0] == 1 and O.utf8_check(m) != 0 else 0
        assert (ev[i], st[i]) == (pmd.EV_MESSAGE, want), (i, kinds[i])
        assert got[i] == m, i


def test_empty_batches_no_state_and_a_second_stream():
    import torch
    pmd = _pmd()
    rng = random.Random(9)
    # n == 0
    empty = pmd.Batch(torch.empty(16, dtype=torch.uint8, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"),
                      torch.empty(0, dtype=torch.int32, device="cuda"))
    u = pmd.unframe_batch(empty, 16, pmd.ROLE_SERVER)
    assert u.event.numel() == 0
    with pytest.raises(pmd.BpmdError):
        pmd.unframe_batch(empty, 16, 2)
    wires = [b"", M.frame(b"hello", 1), b"", M.frame(b"he", 1, fin=False), M.frame(b"x", 0)]
    # entries without a byte; no state: a continuation finds no message to continue
    s = Slots([8] * len(wires), rng, with_state=False)
    got = s.call_checked(wires, M.CLIENT)
    assert [(g.event, g.status, g.consumed) for g in got] == \
        [(0, 0, 0), (1, 0, 7), (0, 0, 0), (0, 0, 4), (0, M.ERR["bad_continuation"], 0)]
    # the same on a second stream, with state
    s2 = Slots([8] * len(wires), rng)
    side = torch.cuda.Stream()
    got2 = s2.call_checked(wires, M.CLIENT, stream=side)
    assert [(g.event, g.status, g.consumed) for g in got2] == [(g.event, g.status, g.consumed) for g in got]
    assert got2[3].state == M.State(2, True, 1, False).pack()
