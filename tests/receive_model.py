"""Expected values for the batch receive side in one chained call
(bpmd_receive_batch): one entry's result, built from the frame model's walk
(tests/frame_parse_model.py), the oracle's inflater at the effective capacity,
the oracle's UTF-8 check and the merge rule of include/beast_pmd.h, restated
here in plain Python, independent of beast_amd/csrc/receive_plan.h.

  read_some's inflate branch   websocket/impl/read.hpp:1284-1385
  rd_msg_max on inflated size  read.hpp:1357-1367
  check_utf8 of text           read.hpp:1372-1384
"""
from __future__ import annotations

from dataclasses import dataclass

from oracle import oracle as O
from tests import frame_parse_model as FM

NEED_BUFFERS = 1
BAD_FRAME_PAYLOAD = FM.ERR["bad_frame_payload"]
BUFFER_OVERFLOW = FM.ERR["buffer_overflow"]
MESSAGE_TOO_BIG = FM.ERR["message_too_big"]
SRC_NONE, SRC_GATHERED, SRC_INFLATED = 0, 1, 2
U32 = (1 << 32) - 1


def inflates(event, status, compressed) -> bool:
    return event == FM.EV_MESSAGE and status == 0 and compressed != 0


def effective_cap(msg_cap: int, msg_max: int) -> int:
    """One byte past the limit tells a message over it from one that reaches
    it; unbounded integers, so msg_max + 1 needs no care here."""
    return min(msg_cap, msg_max + 1) if msg_max else msg_cap


def select(event, status, compressed, op, out_len, msg_cap, msg_max):
    """(inflate input length, effective capacity, text flag)"""
    if not inflates(event, status, compressed):
        return 0, 0, 0
    return out_len, effective_cap(msg_cap, msg_max), int(op == 1)


def merge(event, status, compressed, op, out_len, msg_cap, msg_max, zst, z_len):
    """(status before the UTF-8 check, source of that check, msg_len)"""
    if event != FM.EV_MESSAGE or status != 0:
        return status, SRC_NONE, 0
    if not compressed:
        return 0, SRC_GATHERED if op == 1 else SRC_NONE, out_len
    if zst == NEED_BUFFERS:
        st = MESSAGE_TOO_BIG if msg_max and msg_max <= msg_cap else BUFFER_OVERFLOW
    elif zst:
        st = zst
    elif msg_max and z_len > msg_max:
        st = MESSAGE_TOO_BIG
    else:
        st = 0
    return st, SRC_INFLATED if st == 0 and op == 1 else SRC_NONE, z_len


@dataclass
class Expected:
    stop: FM.Stop            # the frame pass's result, status included
    status: int              # the merged status
    msg_len: int
    inflated: bytes | None   # what the inflater produced (None: the entry was not inflated)
    eff_cap: int             # the room the inflater had
    message: bytes | None    # the message after EV_MESSAGE with status 0 or bad_frame_payload


def receive(b: bytes, role: int, pmd_on: bool, msg_max: int, out_cap: int, msg_cap: int, st: FM.State,
            out: bytearray, wbits: int = 15) -> Expected:
    """One bpmd_receive_batch call on one entry: FM.walk's effect on st and out,
    then the message's fate."""
    s = FM.walk(b, role, pmd_on, msg_max, out_cap, st, out)
    in_len, eff, _ = select(s.event, s.status, s.compressed, s.op, s.out_len, msg_cap, msg_max)
    zst, zout = 0, None
    if pmd_on and inflates(s.event, s.status, s.compressed):
        zst, zout = O.pmd_inflate(bytes(out[:in_len]), cap=eff, wbits=wbits)
    status, src, msg_len = merge(s.event, s.status, s.compressed, s.op, s.out_len, msg_cap, msg_max, zst,
                                 len(zout) if zout is not None else 0)
    data = None
    if s.event == FM.EV_MESSAGE and s.status == 0:
        data = zout if s.compressed else bytes(out[:s.out_len])
    if src != SRC_NONE and O.utf8_check(data) != 0:
        status = BAD_FRAME_PAYLOAD
    return Expected(s, status, msg_len, zout, eff, data if status in (0, BAD_FRAME_PAYLOAD) else None)
