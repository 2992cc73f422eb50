"""Expected values for the chained receive call over context-takeover
connections (bpmd_receive_takeover_batch): one connection, one call.  The
frame model's walk (tests/frame_parse_model.py), the merge rule of
tests/receive_model.py and the connection rules of include/beast_pmd.h --
room, slide, window, advance -- restated in plain Python, independent of
beast_amd/csrc/receive_takeover_plan.h.

The model keeps no inflater between calls: what a connection carries from
message to message is its buffer and its position, exactly what the device
keeps.  The oracle's inflater is given the window first -- the last
min(pos, W) bytes before pos, as one stored block, which leaves it with those
bytes as its window and nothing else (inflate_stream.ipp: the window is the
last 2^windowBits bytes of output) -- and then the message.
tests/test_receive_takeover_plan.py checks that this equals the oracle's
inflater kept across a connection's messages (O.pmd_inflate_stream)."""
from __future__ import annotations

import zlib
from dataclasses import dataclass

from oracle import oracle as O
from tests import frame_parse_model as FM
from tests import receive_model as M


def room(msg_cap: int, slot: int, W: int) -> int:
    """the most bytes one message may claim: "the message capacity" of every other rule"""
    return min(msg_cap, slot - 2 * W)


def place(pos: int, eff_cap: int, slot: int, W: int, inflates: bool):
    """(slide, new_pos, hist)"""
    if not inflates:
        return 0, pos, 0
    slide = pos + eff_cap > slot
    if slide:
        pos = W
    return int(slide), pos, min(pos, W)


def advance(pos: int, inflates: bool, zst: int, z_len: int) -> int:
    return pos + z_len if inflates and zst == 0 else pos


def stored(window: bytes) -> bytes:
    """a permessage-deflate payload of stored blocks that inflates to `window`"""
    z = zlib.compressobj(0, zlib.DEFLATED, -15)
    p = z.compress(window) + z.flush(zlib.Z_SYNC_FLUSH)
    assert p.endswith(b"\x00\x00\xff\xff")
    return p[:-4]


def inflate_after(window: bytes, payload: bytes, cap: int, wbits: int):
    """(status, output) of the oracle's inflater for `payload` when `window` is what it has put out so far"""
    if not window:
        return O.pmd_inflate(payload, cap=cap, wbits=wbits)
    first, res = O.pmd_inflate_stream([stored(window), payload], cap=[len(window), cap], wbits=wbits)
    assert first == (0, window)
    return res


@dataclass
class Expected:
    stop: FM.Stop            # the frame pass's result, status included
    status: int              # the merged status
    msg_off: int             # relative to the connection's base: the position after any slide
    msg_len: int
    pos: int                 # the connection's position after the call
    slid: bool
    zst: int                 # the inflater's own status (0 when the entry was not inflated)
    inflated: bytes | None   # what the inflater produced (None: the entry was not inflated)
    eff_cap: int             # the room the inflater had: the called slot is [msg_off, msg_off + eff_cap)
    message: bytes | None    # the message after EV_MESSAGE with status 0 or bad_frame_payload


def receive(b: bytes, role: int, msg_max: int, out_cap: int, msg_cap: int, st: FM.State, out: bytearray, pos: int,
            buf: bytearray, wbits: int) -> Expected:
    """One bpmd_receive_takeover_batch call on one connection: FM.walk's effect
    on st and out; on buf the slide and the inflated bytes (the called slot's
    bytes past them are the inflater's scratch and stay as they were here)."""
    W, slot = 1 << wbits, len(buf)
    assert slot > 2 * W and 0 <= pos <= slot
    s = FM.walk(b, role, True, msg_max, out_cap, st, out)
    cap = room(msg_cap, slot, W)
    z = M.inflates(s.event, s.status, s.compressed)
    in_len, eff, _ = M.select(s.event, s.status, s.compressed, s.op, s.out_len, cap, msg_max)
    slide, new_pos, hist = place(pos, eff, slot, W, z)
    zst, zout = 0, None
    if slide:
        assert pos - W >= W
        buf[:W] = buf[pos - W:pos]
    if z:
        zst, zout = inflate_after(bytes(buf[new_pos - hist:new_pos]), bytes(out[:in_len]), eff, wbits)
        assert new_pos + eff <= slot and len(zout) <= eff
        buf[new_pos:new_pos + len(zout)] = zout
    status, src, msg_len = M.merge(s.event, s.status, s.compressed, s.op, s.out_len, cap if z else 0, msg_max, zst,
                                   len(zout) if z else 0)
    data = None
    if s.event == FM.EV_MESSAGE and s.status == 0:
        data = zout if s.compressed else bytes(out[:s.out_len])
    if src != M.SRC_NONE and O.utf8_check(data) != 0:
        status = M.BAD_FRAME_PAYLOAD
    return Expected(s, status, new_pos, msg_len, advance(new_pos, z, zst, len(zout) if z else 0), bool(slide), zst,
                    zout, eff, data if status in (0, M.BAD_FRAME_PAYLOAD) else None)
