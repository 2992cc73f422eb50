"""Expected values for the chained receive call that hands a message over in
pieces (bpmd_receive_pieces_batch): one connection, call by call, in plain
Python and independent of beast_amd/csrc/receive_pieces_plan.h.

  walk        the piece walk of include/beast_pmd.h around the frame model's
              parse_fh (tests/frame_parse_model.py): partial data frames,
              rd_remain, the rotated key, the slot reused from call to call
  Conn        one connection: its state, the oracle's inflate_stream
              (oracle.Inflater, one write(Flush::sync) per piece over piece +
              tail with the room the call gives) and the oracle's streaming
              utf8_checker (oracle.Utf8Checker, one write() per piece, finish()
              at the message's end)

The delivered bytes, the statuses and the UTF-8 carry are therefore Beast's
own for these call shapes, bit for bit."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

from oracle import oracle as O
from tests import frame_parse_model as FM

TAIL = b"\x00\x00\xff\xff"
MIN_CAP = 8
NEED_BUFFERS = 1
BAD_FRAME_PAYLOAD, BUFFER_OVERFLOW, MESSAGE_TOO_BIG = 256, 257, 258
U64 = (1 << 64) - 1


def rot_key(key: int, n: int) -> int:
    """the key for the payload bytes after the first n (mask.ipp:29-36)"""
    r = 8 * (n & 3)
    return ((key >> r) | (key << (32 - r))) & 0xFFFFFFFF if r else key


@dataclass
class PState:
    """bpmd_rd_piece_state"""
    rd_size: int = 0
    rd_remain: int = 0
    rd_key: int = 0
    rd_cont: bool = False
    rd_op: int = 0
    rd_deflated: bool = False
    rd_fin: bool = False
    utf8: bytes = b""

    def pack(self) -> bytes:
        return (self.rd_size.to_bytes(8, "little") + self.rd_remain.to_bytes(8, "little") +
                self.rd_key.to_bytes(4, "little") +
                bytes([self.rd_cont, self.rd_op, self.rd_deflated, self.rd_fin, len(self.utf8)]) +
                self.utf8.ljust(3, b"\0") + bytes(4))


ZERO = PState().pack()


@dataclass
class Stop:
    event: int = FM.EV_NEED_MORE
    status: int = 0
    consumed: int = 0
    piece: bytes = b""       # gathered in this call, unmasked
    tail: bool = False
    op: int = 0
    compressed: int = 0
    ctl: bytes = b""
    close_code: int = 0


def walk(b: bytes, role: int, pmd_on: bool, msg_max: int, out_cap: int, st: PState) -> Stop:
    """One call's walk on one connection; updates st except for the reset at a
    message's end, which the caller does once the piece is delivered."""
    s = Stop()
    if out_cap < MIN_CAP:
        s.status = BUFFER_OVERFLOW
        s.op, s.compressed = st.rd_op, int(st.rd_deflated)
        return s
    room, pos, got = out_cap - len(TAIL), 0, bytearray()
    in_frame = st.rd_remain > 0
    while True:
        if in_frame:
            take = min(st.rd_remain, len(b) - pos, room - len(got))
            got += O.mask(b[pos:pos + take], st.rd_key)
            st.rd_key = rot_key(st.rd_key, take)
            st.rd_remain -= take
            if not st.rd_deflated:
                st.rd_size += take
            pos += take
            if st.rd_remain:
                break
            in_frame = False
            if st.rd_fin:
                s.event, s.tail = FM.EV_MESSAGE, bool(st.rd_deflated)
                break
            continue
        view = FM.State(st.rd_size, st.rd_cont, st.rd_op, st.rd_deflated)
        r, h = FM.parse_fh(b[pos:pos + 14], role, pmd_on, msg_max, U64, view)
        if r == FM.NEED_MORE:
            break
        if r != FM.FRAME:
            s.status = r
            break
        if h.op >= 8:
            if h.len > len(b) - pos - h.hdr_len:
                break
            s.ctl = O.mask(b[pos + h.hdr_len:pos + h.hdr_len + h.len], h.key)
            pos += h.hdr_len + h.len
            s.event = {8: FM.EV_CLOSE, 9: FM.EV_PING, 10: FM.EV_PONG}[h.op]
            if h.op == 8:
                s.status, s.close_code = FM.read_close(s.ctl)
            break
        if h.op != 0:
            st.rd_size, st.rd_op, st.rd_deflated = 0, h.op, bool(pmd_on and h.rsv1)
        st.rd_cont, st.rd_fin, st.rd_remain, st.rd_key = not h.fin, h.fin, h.len, h.key
        pos += h.hdr_len
        in_frame = True
    s.piece, s.consumed = bytes(got), pos
    s.op, s.compressed = st.rd_op, int(st.rd_deflated)
    return s


def limit_room(msg_cap: int, msg_max: int, rd_size: int) -> int:
    return msg_cap if msg_max == 0 else min(msg_cap, max(msg_max - rd_size, 0) + 1)


def merge(ec: int, in_used: int, n_in: int, out_used: int, rd_size: int, msg_max: int) -> int:
    if ec not in (0, NEED_BUFFERS):
        return ec
    if msg_max and rd_size + out_used > msg_max:
        return MESSAGE_TOO_BIG
    if in_used < n_in:
        return BUFFER_OVERFLOW
    return 0


@dataclass
class Piece:
    stop: Stop
    status: int                  # d_status
    out_len: int                 # d_out_len: the gathered length
    out: bytes                   # what the out slot holds from its offset 0: piece (+ tail)
    ran: bool                    # the inflater ran
    eff: int                     # its room
    ec: int = 0                  # its own status
    in_used: int = 0
    delivered: bytes = b""       # d_msg_len bytes: inflated, or the gathered piece of a plain message
    state: bytes | None = None   # d_state after the call; None: unspecified (an error)


@dataclass
class Conn:
    role: int
    wbits: int = 15
    pmd_on: bool = True
    msg_max: int = 0
    st: PState = field(default_factory=PState)

    def __post_init__(self):
        self.z = O.Inflater(self.wbits) if self.pmd_on else None
        self.u = O.Utf8Checker()

    def _inflate(self, data: bytes, room: int):
        src = ctypes.create_string_buffer(data, max(len(data), 1))
        dst = ctypes.create_string_buffer(max(room, 1))
        zs = O.ZParams(ctypes.addressof(src) if data else None, len(data), 0, ctypes.addressof(dst), room, 0, 0)
        ec = self.z.write(zs, "sync")
        return ec, zs.total_in, dst.raw[:zs.total_out]

    def call(self, b: bytes, out_cap: int, msg_cap: int = 0) -> Piece:
        st = self.st
        s = walk(b, self.role, self.pmd_on, self.msg_max, out_cap, st)
        last = s.event == FM.EV_MESSAGE
        out = s.piece + (TAIL if s.tail else b"")
        ran = bool(s.compressed and (s.piece or s.tail))
        p = Piece(s, 0, len(s.piece), out, ran, 0)
        if ran:
            p.eff = limit_room(msg_cap, self.msg_max, st.rd_size)
            p.ec, p.in_used, p.delivered = self._inflate(out, p.eff)
            p.status = merge(p.ec, p.in_used, len(out), len(p.delivered), st.rd_size, self.msg_max)
        elif not s.compressed:
            p.delivered = s.piece
        if st.rd_op == 1 and p.status == 0 and (p.delivered or last):   # read.hpp:1372-1384
            if not self.u.write(p.delivered) or (last and not self.u.finish()):
                p.status = BAD_FRAME_PAYLOAD
        bad = p.status != 0 or s.status != 0
        if p.status == 0:
            p.status = s.status
        if last:
            self.st = PState()
            self.u.reset()
        else:
            if st.rd_deflated:
                st.rd_size += len(p.delivered)
            need, have = self.u._s.need, self.u._s.have
            st.utf8 = bytes(self.u._s.cp[:have]) if need else b""
        p.state = None if bad else self.st.pack()
        return p


def deflate_chunks(chunks, wbits: int = 15, level: int = 6):
    """One message deflated chunk by chunk by the oracle's deflater, a sync
    flush behind every chunk: segment k inflates to exactly chunks[k] and ends
    in 00 00 FF FF (an empty chunk's segment is empty).  Joined, with the last
    four bytes dropped, they are one permessage-deflate payload; a test frames
    the segments one by one to know what each piece inflates to."""
    z = O.Deflater(level, wbits, 4, 0)
    segs = []
    for c in chunks:
        if not c:
            segs.append(b"")
            continue
        cap = O.upper_bound(len(c)) + 64
        src = ctypes.create_string_buffer(bytes(c), max(len(c), 1))
        dst = ctypes.create_string_buffer(cap)
        zs = O.ZParams(ctypes.addressof(src), len(c), 0, ctypes.addressof(dst), cap, 0, 0)
        z.write(zs, "sync")
        assert zs.avail_in == 0 and dst.raw[:zs.total_out].endswith(TAIL)
        segs.append(dst.raw[:zs.total_out])
    return segs
