"""Expected values for the chained send call for context-takeover connections
(bpmd_send_takeover_batch): one connection, one call, in plain Python and
independent of beast_amd/csrc.

  deflates       begin_msg (tests/send_model.py compress) for a data opcode
  place          pmd.TakeoverDeflater.deflate's rule: a message that does not
                 fit behind the connection's plaintext first slides the last
                 K bytes to the front
  payload        tests/model: model.encode over the connection's buffer with
                 the history place() gives, as test_takeover_deflate_equals_model
  wire           tests/send_model.py wire (the oracle's framer)

An uncompressed message never passes the peer's inflater, so it stays out of
the buffer: `leak=True` is the wrong rule that lets it in, kept here so that
tests/test_send_takeover_plan.py can show the peer then decodes other bytes.
"""
from dataclasses import dataclass

import numpy as np

from tests import send_model as SM

K = 4096          # pmd.TakeoverDeflater.HIST
CHUNK = 4096
MESSAGE_TOO_BIG = 258
OP_IDLE = 0


def room(max_len, slot, keep=K):
    return min(max_len, max(slot - 2 * keep, 0))


def deflates(op, opt, n, threshold):
    return op in (SM.OP_TEXT, SM.OP_BINARY) and SM.compress(True, opt, n, threshold)


def provisional(op, d, n, L):
    if op not in (OP_IDLE, SM.OP_TEXT, SM.OP_BINARY):
        return SM.BAD_OPCODE
    if d and n > L:
        return MESSAGE_TOO_BIG
    return 0


def place(pos, n, slot, keep, enters):
    """(slide, new_pos, deflater length, hist)"""
    if not enters:
        return 0, pos, 0, 0
    slide = int(pos + n > slot)
    new_pos = keep if slide else pos
    return slide, new_pos, n, min(new_pos, keep)


def advance(new_pos, n, enters, status):
    return new_pos + n if enters and status == 0 else new_pos


def chunk_count(n):
    return -(-n // CHUNK)


def chunk_bound(n, L):
    return n * chunk_count(L)


@dataclass
class Entry:
    compressed: int
    z_len: int        # the deflater's input length
    hist: int
    slid: int
    new_pos: int
    pos: int          # the fill after the call when the wire takes the message
    payload: bytes    # what the deflater leaves in the staging slot (b"" after need_buffers)
    need: int         # the staging bytes the deflater asks for (0 when it gets nothing)
    wire: bytes       # the message's frames (b"" when it is not sent)
    status: int       # without the wire's capacity


def z_need(payload, bits):
    """The staging bytes the deflater asks for: stitch_kernel wants the byte
    after a Huffman block's last one, which the tail does not use when the
    block ends 1-5 bits into a byte (tests/test_gpu_takeover.py's sweep)."""
    return len(payload) + (1 if 1 <= bits % 8 <= 5 else 0)


def send(pos, buf, msg, op, opt, threshold, max_len, slot, z_cap, keys, level=6, wbits=15, frame_max=4096, frag=True,
         leak=False):
    """One bpmd_send_takeover_batch call on one connection.  buf: the
    connection's `slot` bytes, a bytearray changed in place; keys: the
    connection's frame keys (None in server role)."""
    from tests.model import model as M
    assert len(buf) == slot > 2 * K and 0 <= pos <= slot
    n = len(msg)
    L = room(max_len, slot)
    d = deflates(op, opt, n, threshold)
    st = provisional(op, d, n, L)
    enters = bool(d and st == 0)
    if leak and not d and st == 0 and op != OP_IDLE and n <= L:   # the wrong rule: every sent message enters
        slide, new_pos, _, _ = place(pos, n, slot, K, True)
        if slide:
            buf[:K] = buf[pos - K:pos]
        buf[new_pos:new_pos + n] = msg
        pos = new_pos + n
    slide, new_pos, z_len, hist = place(pos, n, slot, K, enters)
    if slide:
        assert pos - K >= K          # the move never overlaps itself
        buf[:K] = buf[pos - K:pos]
    payload, need = b"", 0
    if enters:
        buf[new_pos:new_pos + n] = msg
        bits = []
        (payload,) = M.encode(np.frombuffer(bytes(buf), dtype=np.uint8), [new_pos], [n], level=level, wbits=wbits,
                              hist=[hist], bits=bits)
        need = z_need(payload, bits[0])
        if need > z_cap:
            payload, st = b"", SM.NEED_BUFFERS
    wire = b""
    if st == 0 and op != OP_IDLE:
        body = payload if d else bytes(msg)
        nf = SM.frame_count(len(body), frame_max, bool(d), frag)
        wire = SM.wire(body, op, bool(d), None if keys is None else list(keys[:nf]), frame_max, frag)
    return Entry(int(d), z_len, hist, slide, new_pos, advance(new_pos, n, enters, st), payload, need, wire, st)


def pack(entries, wire_cap):
    """The batch's packed wire: [(offset, written length, final status, final
    pos)] per entry and the total; an entry whose frames do not fit
    [0, wire_cap) is refused and its connection does not advance."""
    out, at = [], 0
    for e in entries:
        size = len(e.wire)
        fits = size != 0 and at + size <= wire_cap
        st = e.status if (size == 0 or fits) else SM.BUFFER_OVERFLOW
        out.append((at, size if fits else 0, st, e.pos if st == 0 else e.new_pos))
        at += size
    return out, at
