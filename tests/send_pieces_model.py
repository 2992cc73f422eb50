"""Expected values for the chained send call that takes messages in pieces
(bpmd_send_pieces_batch): one connection, one call, in plain Python and
independent of beast_amd/csrc, on top of tests/send_takeover_model.py.

  begin          write_some's begin_msg on the first piece (this piece's
                 length decides), the stored decision and opcode after it
  payload        tests/model's encode over the connection's buffer, as
                 send_takeover_model.send; a non-final compressed piece gets
                 00 00 FF FF back behind it
  wire_piece     the oracle's framer over the piece's payload, then the
                 opcode / RSV1 taken off a continuation piece's first frame
                 and FIN off a non-final piece's last
  commit         wr_cont = !fin, pos advanced, reset under no_takeover
"""
from dataclasses import dataclass

import numpy as np

from tests import send_model as SM
from tests import send_takeover_model as TM

K = TM.K
MARKER = b"\x00\x00\xff\xff"
OP_IDLE = 0
ZERO = (0, 0, 0)    # (wr_cont, wr_compress, wr_op): no message open


def begin(state, op, opt, n, threshold):
    """(compress, opcode) of the message this piece belongs to"""
    cont, comp, sop = state
    if op not in (SM.OP_TEXT, SM.OP_BINARY):
        return 0, op
    if cont:
        return int(bool(comp)), sop
    return int(TM.deflates(op, opt, n, threshold)), op


def provisional(op, compress, n, L):
    return TM.provisional(op, compress, n, L)


def status(prov, enters, zst, fin, z_len, z_cap):
    st = prov or (zst if enters else 0)
    if st == 0 and enters and not fin and z_len + 4 > z_cap:
        return SM.NEED_BUFFERS
    return st


def payload_len(compress, fin, n, z_len):
    return (z_len + (0 if fin else 4)) if compress else n


def commit(state, new_pos, n, enters, b, idle, final_status, fin, no_takeover):
    """(pos, state) after the call"""
    if idle or final_status != 0:
        return new_pos, tuple(state)
    pos = new_pos + n if enters else new_pos
    if fin and b[0] and no_takeover:
        pos = 0
    return pos, (0 if fin else 1, int(b[0]), b[1])


def piece_frame_bound(n, frame_max, may_compress, frag, fin):
    plain = SM.frame_count(n, frame_max, False, frag)
    if not may_compress:
        return plain
    return max(plain, SM.frame_count(SM.upper_bound(n) + (0 if fin else 4), frame_max, True, frag))


def piece_wire_bound(n, frame_max, masked, may_compress, frag, fin):
    plain = SM.wire_size(n, frame_max, masked, False, frag)
    if not may_compress:
        return plain
    return max(plain, SM.wire_size(SM.upper_bound(n) + (0 if fin else 4), frame_max, masked, True, frag))


def wire_piece(body, op, compressed, first, fin, keys, frame_max, frag):
    """The frames of one piece: a whole message's frames from the oracle's
    framer, the first frame's opcode and RSV1 cleared unless the piece opens
    the message, the last frame's FIN cleared unless it ends it."""
    masked = keys is not None
    w = bytearray(SM.wire(body, op, compressed, keys, frame_max, frag))
    offs = SM.frame_offsets(len(body), frame_max, masked, compressed, frag)
    if not first:
        w[offs[0][1]] &= 0x80
    if not fin:
        w[offs[-1][1]] &= 0x7F
    return bytes(w)


@dataclass
class Entry:
    compressed: int
    z_len: int        # the deflater's input length
    hist: int
    slid: int
    new_pos: int
    pos: int          # d_pos after the call when the wire takes the piece
    state: tuple      # d_state after the call when the wire takes the piece
    payload: bytes    # the staging slot's d_z_len bytes (b"" after need_buffers from the deflater)
    marked: int       # the marker was written
    need: int         # the staging bytes the deflater asks for
    wire: bytes       # the piece's frames (b"" when it is not sent)
    status: int       # without the wire's capacity


def send(pos, state, buf, piece, op, opt, fin, no_takeover, threshold, max_len, slot, z_cap, keys, level=6, wbits=15,
         frame_max=4096, frag=True):
    """One bpmd_send_pieces_batch call on one connection.  buf: the
    connection's `slot` bytes, a bytearray changed in place; keys: the
    piece's frame keys (None in server role)."""
    from tests.model import model as M
    assert len(buf) == slot > 2 * K and 0 <= pos <= slot
    n = len(piece)
    L = TM.room(max_len, slot)
    b = begin(state, op, opt, n, threshold)
    c = b[0]
    prov = provisional(op, c, n, L)
    enters = bool(c and prov == 0)
    slide, new_pos, z_len, hist = TM.place(pos, n, slot, K, enters)
    if slide:
        assert pos - K >= K
        buf[:K] = buf[pos - K:pos]
    payload, need, zst, marked = b"", 0, 0, 0
    if enters:
        buf[new_pos:new_pos + n] = piece
        bits = []
        (payload,) = M.encode(np.frombuffer(bytes(buf), dtype=np.uint8), [new_pos], [n], level=level, wbits=wbits,
                              hist=[hist], bits=bits)
        need = TM.z_need(payload, bits[0])
        if need > z_cap:
            payload, zst = b"", SM.NEED_BUFFERS
    st = status(prov, enters, zst, fin, len(payload), z_cap)
    if st == 0 and enters and not fin:
        payload, marked = payload + MARKER, 1
    wire = b""
    if st == 0 and op != OP_IDLE:
        body = payload if c else bytes(piece)
        assert len(body) == payload_len(c, fin, n, len(payload) - 4 * marked)
        nf = SM.frame_count(len(body), frame_max, bool(c), frag)
        wire = wire_piece(body, b[1], bool(c), not state[0], bool(fin), None if keys is None else list(keys[:nf]),
                          frame_max, frag)
    p1, s1 = commit(state, new_pos, n, enters, b, op == OP_IDLE, st, fin, no_takeover)
    return Entry(c, z_len, hist, slide, new_pos, p1, s1, payload, marked, need, wire, st)


def pack(entries, states, wire_cap):
    """The batch's packed wire: [(offset, written length, final status, final
    pos, final state)] per entry and the total; states: d_state before the
    call.  An entry whose frames do not fit [0, wire_cap) is refused: its
    connection does not advance and its state stays."""
    out, at = [], 0
    for e, s0 in zip(entries, states):
        size = len(e.wire)
        fits = size != 0 and at + size <= wire_cap
        st = e.status if (size == 0 or fits) else SM.BUFFER_OVERFLOW
        out.append((at, size if fits else 0, st, e.pos if st == 0 else e.new_pos, e.state if st == 0 else tuple(s0)))
        at += size
    return out, at
