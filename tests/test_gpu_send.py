"""bpmd_send_batch and pmd.send_batch on the GPU: the send side from messages
to packed wire bytes, against tests/send_model.py (begin_msg's rule and
write_some's frame split over the oracle's framer O.frame_write).  A
compressed message's expected payload is that message's own pmd.deflate_batch
payload at the same cfg.  Messages and staging slots lie at ragged offsets
with guard bytes between them and the wire buffer is canary-filled: after
every call the input must be unchanged, the staging buffer touched inside its
slots only, and the wire equal to the expected messages back to back with the
canary everywhere else."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

from beast_amd import synth
from oracle import oracle as O
from tests import send_model as M
from tests.test_send_plan import FRAME_MAX, lengths

pytestmark = pytest.mark.gpu

IN_FILL, Z_FILL, WIRE_FILL = 0x3C, 0x5A, 0xA5
_zref = {}


def _pmd():
    import torch  # noqa: F401
    from beast_amd import pmd
    return pmd


def ragged(blobs, fill, rng):
    """the blobs at ragged offsets in one buffer, `fill` between them"""
    offs, pos = [], 0
    for b in blobs:
        pos += rng.randrange(1, 20)
        offs.append(pos)
        pos += len(b)
    buf = bytearray([fill]) * (pos + 64)
    for o, b in zip(offs, blobs):
        buf[o:o + len(b)] = b
    return buf, offs


def deflated(msgs):
    """each message's own pmd.deflate_batch payload (level 6, 15 bits, memLevel 4)"""
    import torch
    pmd = _pmd()
    key = hash(tuple(msgs))
    if key not in _zref:
        z = pmd.deflate_batch(pmd.Batch.from_host(msgs))
        torch.cuda.synchronize()
        assert z.status.cpu().tolist() == [0] * len(msgs)
        _zref[key] = z.out.to_host()
    return _zref[key]


def send(msgs, role, frame_max, frag=True, pmd_on=True, threshold=0, ops=None, opts=None, caps=None, wire_cap=None,
         seed=0, stream=None):
    """One pmd.send_batch with every buffer made here; returns what the device left."""
    import torch
    pmd = _pmd()
    rng = random.Random(seed)
    n = len(msgs)
    dev = "cuda"
    masked = role == M.CLIENT
    ops = [2] * n if ops is None else ops
    opts = [1] * n if opts is None else opts
    inbuf, offs = ragged(msgs, IN_FILL, rng)
    caps = [M.upper_bound(len(m)) for m in msgs] if caps is None else caps
    zbuf, zoffs = ragged([bytes(c) for c in caps], Z_FILL, rng)
    zbuf = bytearray([Z_FILL]) * len(zbuf)
    fb = [pmd.send_frame_bound(len(m), frame_max, bool(pmd_on and o), frag) for m, o in zip(msgs, opts)]
    kb = [int(x) for x in np.cumsum([0] + fb[:-1])] if n else []
    keys = [rng.getrandbits(32) for _ in range(sum(fb))]
    bound = sum(pmd.send_wire_bound(len(m), frame_max, masked, bool(pmd_on and o), frag) for m, o in zip(msgs, opts))
    cap = bound if wire_cap is None else wire_cap
    wire = torch.full((max(cap, bound) + 64,), WIRE_FILL, dtype=torch.uint8, device=dev)
    src = pmd.Batch(torch.frombuffer(bytearray(inbuf), dtype=torch.uint8).to(dev),
                    torch.tensor(offs, dtype=torch.int64, device=dev),
                    torch.tensor([len(m) for m in msgs], dtype=torch.int32, device=dev))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    staging = pmd.Result(pmd.Batch(torch.frombuffer(bytearray(zbuf), dtype=torch.uint8).to(dev),
                                   torch.tensor(zoffs, dtype=torch.int64, device=dev), i32([-1] * n)), i32(caps),
                         i32([-1] * n)) if pmd_on else None
    kt = torch.from_numpy(np.array(keys + [0], dtype=np.uint32).view(np.int32)).to(dev) if masked else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    s = pmd.send_batch(src, role, pmd_on=pmd_on, threshold=threshold, frag=frag, frame_max=frame_max,
                       op=torch.tensor(ops, dtype=torch.uint8), opt=torch.tensor(opts, dtype=torch.uint8), keys=kt,
                       key_base=i32(kb) if masked else None, staging=staging, wire=wire, wire_cap=cap, stream=stream)
    torch.cuda.synchronize()
    assert src.data.cpu().numpy().tobytes() == bytes(inbuf), "the input was modified"
    r = SimpleNamespace(n=n, wire=wire.cpu().numpy().tobytes(), off=s.wire.off.cpu().tolist(),
                        len=s.wire.len.cpu().tolist(), status=s.status.cpu().tolist(),
                        comp=s.compressed.cpu().tolist(), total=int(s.total.item()), keys=keys, kb=kb, cap=cap,
                        sent=s, masked=masked)
    if pmd_on:
        r.z = staging.out.data.cpu().numpy().tobytes()
        r.zoffs, r.zlen, r.caps = zoffs, staging.out.len.cpu().tolist(), caps
        guard = bytearray(r.z)
        for o, c in zip(zoffs, caps):
            guard[o:o + c] = bytes([Z_FILL]) * c
        assert bytes(guard) == bytes([Z_FILL]) * len(guard), "a byte outside the staging slots was written"
    return r


def expected(msgs, r, frame_max, frag, pmd_on, threshold, ops, opts, zref=None):
    """[(compressed, payload on the wire, wire bytes)] by the model"""
    zref = zref or (deflated(msgs) if pmd_on else None)
    out = []
    for i, m in enumerate(msgs):
        c = M.compress(pmd_on, opts[i] if opts else True, len(m), threshold)
        payload = zref[i] if c else m
        nf = M.frame_count(len(payload), frame_max, c, frag)
        keys = r.keys[r.kb[i]:r.kb[i] + nf] if r.masked else None
        out.append((c, payload, M.wire(payload, ops[i] if ops else 2, c, keys, frame_max, frag)))
    return out


def check_packed(r, want, statuses=None):
    """offsets, lengths, total and the whole wire buffer; want: wire bytes per
    message (b"" for one that takes no room)"""
    sizes = [len(w) for w in want]
    offs = [int(x) for x in np.cumsum([0] + sizes[:-1])]
    assert r.total == sum(sizes)
    assert r.off == offs
    fits = [o + s <= r.cap for o, s in zip(offs, sizes)]
    assert r.len == [s if f else 0 for s, f in zip(sizes, fits)]
    buf = bytearray([WIRE_FILL]) * len(r.wire)
    for o, w, f in zip(offs, want, fits):
        if f:
            buf[o:o + len(w)] = w
    if bytes(buf) != r.wire:
        bad = next(i for i in range(len(buf)) if buf[i] != r.wire[i])
        raise AssertionError(f"wire differs at byte {bad} (total {r.total}, cap {r.cap})")
    if statuses is None:
        statuses = [0] * r.n
    assert r.status == [st if st or f else M.BUFFER_OVERFLOW for st, f in zip(statuses, fits)]


def _text(rng, n):
    words = [b"alpha", b"beta", b"gamma", b"{\"k\":", b"12345", b"true", b" ", b"\n", "é".encode()]
    return b"".join(rng.choices(words, k=n))[:n]


@pytest.mark.parametrize("role", [M.SERVER, M.CLIENT])
@pytest.mark.parametrize("frag", [False, True])
def test_wire_bytes(role, frag):
    """About 600 messages over the length and frame_max grid, text and binary,
    with threshold, opt and pmd_on cases mixing compressed and plain ones."""
    total, kinds = 0, set()
    for k, fm in enumerate(FRAME_MAX):
        rng = random.Random(100 * k + 10 * role + frag)
        grid = lengths(fm)
        must = [0, 1, 125, 126, 127, 130, 65535, 65536, 65540, fm - 1, fm, fm + 1, 2 * fm, 2 * fm + 1]
        must = [x for x in must if x in grid and (fm > 2 or x <= 130 or x == 65536)]
        lens = must + [rng.choice(grid) if fm > 2 else rng.randrange(0, 131) for _ in range(8)]
        msgs = [_text(rng, ln) if rng.random() < 0.7 else rng.randbytes(ln) for ln in lens]
        ops = [rng.choice([1, 2]) for _ in msgs]
        opts = [int(rng.random() < 0.8) for _ in msgs]
        pmd_on, threshold = k % 4 != 3, [0, 100, 127, 0][k % 4]
        r = send(msgs, role, fm, frag, pmd_on, threshold, ops, opts, seed=k)
        exp = expected(msgs, r, fm, frag, pmd_on, threshold, ops, opts)
        assert r.comp == [int(e[0]) for e in exp], fm
        kinds |= {(pmd_on, c) for c in r.comp}
        if pmd_on:
            for i, (c, payload, _) in enumerate(exp):
                if c:   # the staging slot holds deflate_batch's payload
                    assert r.zlen[i] == len(payload), (fm, i)
                    assert r.z[r.zoffs[i]:r.zoffs[i] + r.zlen[i]] == payload, (fm, i)
        check_packed(r, [e[2] for e in exp])
        total += len(msgs)
    assert total >= 140
    assert kinds == {(True, 0), (True, 1), (False, 0)}, "compressed and plain messages, pmd on and off"


def test_wire_bytes_message_count():
    """the four cases of test_wire_bytes cover about 600 messages"""
    n = 0
    for fm in FRAME_MAX:
        grid = lengths(fm)
        must = [0, 1, 125, 126, 127, 130, 65535, 65536, 65540, fm - 1, fm, fm + 1, 2 * fm, 2 * fm + 1]
        n += len([x for x in must if x in grid and (fm > 2 or x <= 130 or x == 65536)]) + 8
    assert 4 * n >= 560


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097, 20000])
def test_packing(n):
    """d_wire_off is the exclusive sum of the model's sizes and d_total their
    sum, across the scan's tiles; nothing outside [0, total) changes."""
    rng = random.Random(n)
    msgs = [_text(rng, rng.randrange(0, 41)) for _ in range(n)]
    ops = [rng.choice([1, 2]) for _ in msgs]
    role, frag = (M.CLIENT, True) if n % 2 else (M.SERVER, False)
    r = send(msgs, role, 16, frag, True, 20, ops, None, seed=n)
    exp = expected(msgs, r, 16, frag, True, 20, ops, None)
    assert r.comp == [int(len(m) >= 20) for m in msgs]
    check_packed(r, [e[2] for e in exp])
    assert r.wire[r.total:] == bytes([WIRE_FILL]) * (len(r.wire) - r.total)


def test_capacity():
    """wire_cap at total, total - 1, one byte inside a chosen message and 0:
    the messages before the cut are as in the roomy run, the rest are refused
    and nothing is written from the first refused offset on."""
    rng = random.Random(21)
    msgs = [_text(rng, rng.choice([0, 3, 50, 126, 300, 5000])) for _ in range(40)]
    ops = [rng.choice([1, 2]) for _ in msgs]
    roomy = send(msgs, M.CLIENT, 126, True, True, 100, ops, None, seed=3)
    exp = expected(msgs, roomy, 126, True, True, 100, ops, None)
    want = [e[2] for e in exp]
    check_packed(roomy, want)
    assert roomy.status == [0] * len(msgs)
    total = roomy.total
    for cap in (total, total - 1, roomy.off[17] + 1, roomy.off[1], 0):
        r = send(msgs, M.CLIENT, 126, True, True, 100, ops, None, wire_cap=cap, seed=3)
        assert r.total == total and r.off == roomy.off
        check_packed(r, want)
        first = next((i for i in range(len(msgs)) if roomy.off[i] + len(want[i]) > cap), len(msgs))
        cut = roomy.off[first] if first < len(msgs) else total
        assert r.wire[:cut] == roomy.wire[:cut]
        assert r.wire[cut:] == bytes([WIRE_FILL]) * (len(r.wire) - cut)
        assert r.status == [0] * first + [M.BUFFER_OVERFLOW] * (len(msgs) - first)
        assert r.len[first:] == [0] * (len(msgs) - first)
    assert first == 0


def test_status_precedence():
    """bad_opcode, then the deflater's need_buffers, then buffer_overflow: a
    3-byte staging slot and an opcode 9 among good messages take no room, and
    their neighbours' bytes and offsets are as if the two were absent."""
    rng = random.Random(22)
    msgs = [_text(rng, rng.choice([10, 200, 700])) for _ in range(24)]
    msgs[5] = _text(rng, 400)
    msgs[11] = _text(rng, 400)
    ops = [rng.choice([1, 2]) for _ in msgs]
    ops[9], ops[11], ops[20] = 9, 0, 3            # 11: bad opcode and a small slot
    caps = [M.upper_bound(len(m)) for m in msgs]
    caps[5] = caps[11] = 3
    zref = deflated(msgs)
    assert len(zref[5]) > 4
    for role in (M.SERVER, M.CLIENT):
        r = send(msgs, role, 125, True, True, 0, ops, None, caps=caps, seed=5)
        exp = expected(msgs, r, 125, True, True, 0, ops, None, zref)
        want = [e[2] for e in exp]
        st = [0] * len(msgs)
        for i in (9, 11, 20):
            want[i], st[i] = b"", M.BAD_OPCODE
        want[5], st[5] = b"", M.NEED_BUFFERS
        check_packed(r, want, st)
        assert r.zlen[5] == 0
        # the same with room for the first 15 messages only
        cap = r.off[15] + 1
        r2 = send(msgs, role, 125, True, True, 0, ops, None, caps=caps, wire_cap=cap, seed=5)
        check_packed(r2, want, st)
        assert r2.status[14] == 0 and r2.status[15] == M.BUFFER_OVERFLOW and r2.status[20] == M.BAD_OPCODE
        assert r2.status[16:20] == [M.BUFFER_OVERFLOW] * 4


def _mixed_messages(n, rng):
    lens = np.array([rng.choice([0, 1, 7, 90, 200, 900, 2500, 6000]) for _ in range(n)], dtype=np.uint32)
    data, off, ln = synth.make_batch("json", lens, seed=rng.randrange(1 << 30))
    msgs = [bytes(data[int(off[i]):int(off[i]) + int(ln[i])]) for i in range(n)]
    ops = []
    for i in range(n):
        kind = rng.random()
        if kind < 0.25:
            msgs[i] = rng.randbytes(len(msgs[i]))
        elif kind < 0.4 and msgs[i]:
            b = bytearray(msgs[i])
            b[rng.randrange(len(b))] = rng.choice([0x80, 0xC0, 0xFF])
            msgs[i] = bytes(b)
        ops.append(2 if kind < 0.25 and rng.random() < 0.7 else rng.choice([1, 1, 2]))
    return msgs, ops


@pytest.mark.parametrize("role", [M.CLIENT, M.SERVER])
def test_round_trip(role):
    """send_batch feeds receive_batch on the other end and the messages come
    back: about 3 000 JSON, binary and text messages, a threshold that leaves
    some plain, text that is not UTF-8 reported as bad_frame_payload."""
    import torch
    pmd = _pmd()
    rng = random.Random(30 + role)
    msgs, ops = _mixed_messages(3000, rng)
    opts = [int(rng.random() < 0.9) for _ in msgs]
    kt = None
    if role == M.CLIENT:
        nk = sum(pmd.send_frame_bound(len(m), 1000, bool(o), True) for m, o in zip(msgs, opts))
        kt = torch.randint(-2**31, 2**31 - 1, (nk,), dtype=torch.int32, device="cuda")
    s = pmd.send_batch(pmd.Batch.from_host(msgs), role, threshold=150, frame_max=1000,
                       op=torch.tensor(ops, dtype=torch.uint8), opt=torch.tensor(opts, dtype=torch.uint8), keys=kt)
    torch.cuda.synchronize()
    assert s.status.cpu().tolist() == [0] * len(msgs)
    comp = s.compressed.cpu().tolist()
    assert comp == [int(o and len(m) >= 150) for m, o in zip(msgs, opts)] and 0 < sum(comp) < len(msgs)
    assert int(s.total.item()) == int(s.wire.len.to(torch.int64).sum().item())
    r = pmd.receive_batch(s.wire, 7000, 6000, pmd.ROLE_SERVER if role == M.CLIENT else pmd.ROLE_CLIENT)
    torch.cuda.synchronize()
    ev, st, got = r.event.cpu().tolist(), r.status.cpu().tolist(), r.to_host()
    assert r.frames.consumed.cpu().tolist() == s.wire.len.cpu().tolist()
    assert r.frames.compressed.cpu().tolist() == comp and r.frames.op.cpu().tolist() == ops
    bad = 0
    for i, m in enumerate(msgs):
        want = pmd.BAD_FRAME_PAYLOAD if ops[i] == 1 and O.utf8_check(m) != 0 else 0
        bad += want != 0
        assert (ev[i], st[i]) == (pmd.EV_MESSAGE, want), (i, ops[i], comp[i], len(m))
        assert got[i] == m, i
    assert bad > 100


def test_one_long_frame_without_auto_fragment():
    """A 70 000-byte incompressible message with frag == 0 and compression off
    for it goes out as one frame with a 10-byte header."""
    import torch
    pmd = _pmd()
    rng = random.Random(40)
    msgs = [rng.randbytes(70000), _text(rng, 300), b""]
    opts = [0, 1, 0]
    r = send(msgs, M.SERVER, 4096, False, True, 0, [2, 1, 2], opts, seed=1)
    exp = expected(msgs, r, 4096, False, True, 0, [2, 1, 2], opts)
    check_packed(r, [e[2] for e in exp])
    assert r.comp == [0, 1, 0] and r.len[0] == 70010 and r.len[2] == 2
    assert r.wire[:10] == bytes([0x82, 127]) + (70000).to_bytes(8, "big")
    assert r.wire[10:70010] == msgs[0]
    # the receiving client reads it as one message
    u = pmd.unframe_batch(r.sent.wire, 70000, pmd.ROLE_CLIENT)
    torch.cuda.synchronize()
    assert u.event.cpu().tolist() == [pmd.EV_MESSAGE] * 3 and u.out.message(0) == msgs[0]
    # masked, it is one 14-byte-header frame
    rc = send(msgs[:1], M.CLIENT, 4096, False, False, 0, [2], [1], seed=2)
    assert rc.len == [70014] and rc.wire[:70014] == M.wire(msgs[0], 2, False, rc.keys[:1], 4096, False)


def test_empty_batch_and_a_second_stream():
    import torch
    pmd = _pmd()
    e = pmd.Batch.from_host([])
    s = pmd.send_batch(e, pmd.ROLE_SERVER)
    assert s.wire.n == 0 and int(s.total.item()) == 0
    rng = random.Random(50)
    msgs = [_text(rng, rng.choice([0, 5, 130, 4000, 9000])) for _ in range(100)]
    side = torch.cuda.Stream()
    r = send(msgs, M.CLIENT, 4096, True, True, 64, None, None, seed=4, stream=side)
    check_packed(r, [x[2] for x in expected(msgs, r, 4096, True, True, 64, None, None)])
