"""bpmd_control_batch on the GPU: ping, pong and close frames against the
model's control writer (tests/send_model.py, pinned by RFC 6455 5.7) and read
back by bpmd_unframe_batch on the opposite role.  Payload slots and the wire
buffer are canary-filled: a frame changes the bytes of its own length only."""
import random

import numpy as np
import pytest

from tests import send_model as M

pytestmark = pytest.mark.gpu

SLOT_FILL, WIRE_FILL = 0x5A, 0xA5


def _pmd():
    import torch  # noqa: F401
    from beast_amd import pmd
    return pmd


def run(entries, masked, rng):
    """entries: [(op, slot bytes, close code)]; one bpmd_control_batch, checked
    against the model entry by entry.  Returns (Controls, keys)."""
    import torch
    pmd = _pmd()
    n = len(entries)
    ctl = np.full((n, M.CTL_SLOT), SLOT_FILL, dtype=np.uint8)
    for i, (_, slot, _) in enumerate(entries):
        ctl[i, :len(slot)] = np.frombuffer(slot, dtype=np.uint8)
    keys = [rng.getrandbits(32) for _ in range(n)] if masked else None
    wire = torch.full((n * M.CTL_WIRE + 16,), WIRE_FILL, dtype=torch.uint8, device="cuda")
    ctl_t = torch.from_numpy(ctl).cuda()
    c = pmd.control_batch(torch.tensor([e[0] for e in entries], dtype=torch.uint8), ctl_t,
                          torch.tensor([len(e[1]) for e in entries], dtype=torch.uint8),
                          close_code=[e[2] for e in entries], key=keys, wire=wire)
    torch.cuda.synchronize()
    assert ctl_t.cpu().numpy().tobytes() == ctl.tobytes(), "the payload slots were modified"
    got, lens, st = wire.cpu().numpy().tobytes(), c.wire.len.cpu().tolist(), c.status.cpu().tolist()
    assert c.wire.off.cpu().tolist() == [M.CTL_WIRE * i for i in range(n)]
    want = bytearray([WIRE_FILL]) * len(got)
    for i, (op, slot, code) in enumerate(entries):
        est, frame = M.control(op, slot, code, keys[i] if masked else None)
        assert (st[i], lens[i]) == (est, len(frame)), (i, op, len(slot), code)
        want[M.CTL_WIRE * i:M.CTL_WIRE * i + len(frame)] = frame
    assert got == bytes(want)
    return c, keys


def read_back(c, masked):
    """the frames through bpmd_unframe_batch on the receiving role"""
    import torch
    pmd = _pmd()
    u = pmd.unframe_batch(c.wire, 0, pmd.ROLE_SERVER if masked else pmd.ROLE_CLIENT)
    torch.cuda.synchronize()
    return u


@pytest.mark.parametrize("masked", [False, True])
def test_ping_pong_every_length(masked):
    rng = random.Random(60 + masked)
    entries = [(op, rng.randbytes(ln), rng.choice([0, 1000])) for op in (M.OP_PING, M.OP_PONG) for ln in range(126)]
    c, _ = run(entries, masked, rng)
    assert c.status.cpu().tolist() == [0] * len(entries)
    pmd = _pmd()
    u = read_back(c, masked)
    assert u.status.cpu().tolist() == [0] * len(entries)
    assert u.event.cpu().tolist() == [pmd.EV_PING] * 126 + [pmd.EV_PONG] * 126
    assert u.consumed.cpu().tolist() == c.wire.len.cpu().tolist()
    cl, ctl = u.ctl_len.cpu().tolist(), u.ctl.cpu().numpy()
    for i, (_, slot, _) in enumerate(entries):
        assert ctl[i, :cl[i]].tobytes() == slot, i


@pytest.mark.parametrize("masked", [False, True])
def test_close_codes_and_reasons(masked):
    rng = random.Random(62 + masked)
    reasons = [b"", b"x", ("going away " * 12).encode()[:123]]
    entries = [(M.OP_CLOSE, r, code) for code in (0, 1000, 1001, 4999) for r in reasons]
    c, _ = run(entries, masked, rng)
    assert c.status.cpu().tolist() == [0] * len(entries)
    pmd = _pmd()
    u = read_back(c, masked)
    assert u.event.cpu().tolist() == [pmd.EV_CLOSE] * len(entries) and u.status.cpu().tolist() == [0] * len(entries)
    assert u.close_code.cpu().tolist() == [e[2] for e in entries]
    cl, ctl = u.ctl_len.cpu().tolist(), u.ctl.cpu().numpy()
    for i, (_, r, code) in enumerate(entries):
        assert ctl[i, :cl[i]].tobytes() == (code.to_bytes(2, "big") + r if code else b""), i


def test_a_received_ping_goes_back_out_as_a_pong():
    """unframe_batch's control slots, unchanged, are control_batch's input"""
    import torch
    pmd = _pmd()
    rng = random.Random(64)
    payloads = [rng.randbytes(ln) for ln in (0, 1, 4, 5, 64, 124, 125)]
    pings, keys = run([(M.OP_PING, p, 0) for p in payloads], True, rng)      # a client's pings
    u = read_back(pings, True)                                                # the server reads them
    assert u.event.cpu().tolist() == [pmd.EV_PING] * len(payloads)
    pongs = pmd.control_batch(10, u.ctl, u.ctl_len)                          # and answers, unmasked
    torch.cuda.synchronize()
    assert pongs.status.cpu().tolist() == [0] * len(payloads)
    assert pongs.wire.to_host() == [M.control(M.OP_PONG, p)[1] for p in payloads]
    back = pmd.unframe_batch(pongs.wire, 0, pmd.ROLE_CLIENT)
    torch.cuda.synchronize()
    assert back.event.cpu().tolist() == [pmd.EV_PONG] * len(payloads)
    cl, ctl = back.ctl_len.cpu().tolist(), back.ctl.cpu().numpy()
    assert [ctl[i, :cl[i]].tobytes() for i in range(len(payloads))] == payloads


@pytest.mark.parametrize("masked", [False, True])
def test_oversize_and_bad_opcodes_write_nothing(masked):
    rng = random.Random(66 + masked)
    entries = [(op, rng.randbytes(ln), 0) for op in (M.OP_PING, M.OP_PONG) for ln in (125, 126, 127, 128, 200, 255)]
    entries += [(M.OP_CLOSE, rng.randbytes(ln), code) for code in (0, 1000) for ln in (123, 124, 125, 128, 255)]
    entries += [(op, rng.randbytes(ln), code) for op in (0, 1, 2, 3, 7, 11, 15, 16, 255) for ln in (0, 9)
                for code in (0, 1000)]
    # a slot holds 128 bytes: a longer length is refused before any byte of it is read
    entries = [(op, s[:M.CTL_SLOT] + bytes(max(0, len(s) - M.CTL_SLOT)), c) for op, s, c in entries]
    import torch
    pmd = _pmd()
    n = len(entries)
    ctl = np.full((n, M.CTL_SLOT), SLOT_FILL, dtype=np.uint8)
    for i, (_, slot, _) in enumerate(entries):
        k = min(len(slot), M.CTL_SLOT)
        ctl[i, :k] = np.frombuffer(slot[:k], dtype=np.uint8)
    keys = [rng.getrandbits(32) for _ in range(n)] if masked else None
    wire = torch.full((n * M.CTL_WIRE + 16,), WIRE_FILL, dtype=torch.uint8, device="cuda")
    c = pmd.control_batch(torch.tensor([e[0] for e in entries], dtype=torch.uint8), torch.from_numpy(ctl).cuda(),
                          torch.tensor([len(e[1]) for e in entries], dtype=torch.uint8),
                          close_code=[e[2] for e in entries], key=keys, wire=wire)
    torch.cuda.synchronize()
    got, lens, st = wire.cpu().numpy().tobytes(), c.wire.len.cpu().tolist(), c.status.cpu().tolist()
    want = bytearray([WIRE_FILL]) * len(got)
    kinds = set()
    for i, (op, slot, code) in enumerate(entries):
        est, frame = M.control(op, slot, code, keys[i] if masked else None)
        assert (st[i], lens[i]) == (est, len(frame)), (i, op, len(slot), code)
        want[M.CTL_WIRE * i:M.CTL_WIRE * i + len(frame)] = frame
        kinds.add(est)
    assert got == bytes(want)
    assert kinds == {0, M.BAD_CONTROL_SIZE, M.BAD_OPCODE}
    assert pmd.WS_BAD_CONTROL_SIZE == M.BAD_CONTROL_SIZE and pmd.WS_BAD_OPCODE == M.BAD_OPCODE
