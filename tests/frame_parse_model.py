"""Expected values for the batch receive side (bpmd_unframe_batch): Beast's
frame parsing restated in plain Python, independent of beast_amd/csrc.

  parse_fh             websocket/impl/stream_impl.hpp:701-913
  is_valid_close_code  websocket/detail/frame.hpp:94-126
  read_close           websocket/detail/frame.hpp:196-240
  walk                 the stop rules of bpmd_unframe_batch (include/beast_pmd.h)
                       around read_some's frame loop (websocket/impl/read.hpp:1063-1283)

The byte work is the oracle's: O.mask unmasks, O.utf8_check is check_utf8.
"""
from dataclasses import dataclass, field

from oracle import oracle as O

SERVER, CLIENT = 0, 1
NEED_MORE, FRAME = 0, 1
EV_NEED_MORE, EV_MESSAGE, EV_PING, EV_PONG, EV_CLOSE = 0, 1, 2, 3, 4
# websocket::error (websocket/error.hpp), numbered as include/beast_pmd.h does
ERR = {name: 256 + i for i, name in enumerate(
    ["bad_frame_payload", "buffer_overflow", "message_too_big", "bad_opcode", "bad_data_frame", "bad_continuation",
     "bad_reserved_bits", "bad_control_fragment", "bad_control_size", "bad_unmasked_frame", "bad_masked_frame",
     "bad_size", "bad_close_code", "bad_close_size", "bad_close_payload"])}
ERR_NAME = {v: k for k, v in ERR.items()}
U64 = (1 << 64) - 1


@dataclass
class State:
    """rd_size, rd_cont, rd_op (stream_impl.hpp:78-87) and the pmd's rd_set
    (impl_base.hpp:61-78)"""
    rd_size: int = 0
    rd_cont: bool = False
    rd_op: int = 0
    rd_deflated: bool = False

    def pack(self) -> bytes:
        """bpmd_rd_state"""
        return self.rd_size.to_bytes(8, "little") + bytes([self.rd_cont, self.rd_op, self.rd_deflated]) + bytes(5)

    def copy(self):
        return State(self.rd_size, self.rd_cont, self.rd_op, self.rd_deflated)


@dataclass
class Header:
    hdr_len: int = 0
    len: int = 0
    fin: bool = False
    rsv1: bool = False
    op: int = 0
    masked: bool = False
    key: int = 0


def parse_fh(b: bytes, role: int, pmd_on: bool, msg_max: int, out_room: int, st: State):
    """(NEED_MORE | FRAME | error, Header or None); reads only b, changes nothing."""
    if len(b) < 2:                                   # :706-711
        return NEED_MORE, None
    len7 = b[1] & 0x7F                               # :720-727
    need = {126: 2, 127: 8}.get(len7, 0)
    masked = bool(b[1] & 0x80)                       # :728-730
    if masked:
        need += 4
    if len(b) - 2 < need:                            # :731-736
        return NEED_MORE, None
    op = b[0] & 0x0F                                 # :737-742
    fin, rsv1, rsv2, rsv3 = (bool(b[0] & m) for m in (0x80, 0x40, 0x20, 0x10))
    if op in (1, 2):                                 # :746-761
        if st.rd_cont:
            return ERR["bad_data_frame"], None
        # rd_deflated(rsv1) is false only without the extension (impl_base.hpp:68-78, 381-390)
        if rsv2 or rsv3 or (rsv1 and not pmd_on):
            return ERR["bad_reserved_bits"], None
    elif op == 0:                                    # :763-776
        if not st.rd_cont:
            return ERR["bad_continuation"], None
        if rsv1 or rsv2 or rsv3:
            return ERR["bad_reserved_bits"], None
    else:                                            # :778-803
        if 3 <= op <= 7 or 11 <= op <= 15:           # is_reserved, frame.hpp:69-76
            return ERR["bad_opcode"], None
        if not fin:
            return ERR["bad_control_fragment"], None
        if len7 > 125:
            return ERR["bad_control_size"], None
        if rsv1 or rsv2 or rsv3:
            return ERR["bad_reserved_bits"], None
    if role == SERVER and not masked:                # :805-810
        return ERR["bad_unmasked_frame"], None
    if role == CLIENT and masked:                    # :811-816
        return ERR["bad_masked_frame"], None
    # :817-823 (a control frame waits for its payload): walk() does so for every frame
    at, ln = 2, len7
    if len7 == 126:                                  # :826-840
        ln, at = int.from_bytes(b[2:4], "big"), 4
        if ln < 126:
            return ERR["bad_size"], None
    elif len7 == 127:                                # :841-861
        ln, at = int.from_bytes(b[2:10], "big"), 10
        if ln < 65536:
            return ERR["bad_size"], None
        if ln >> 63:
            return ERR["bad_size"], None
    key = 0
    if masked:                                       # :863-871
        key, at = int.from_bytes(b[at:at + 4], "little"), at + 4
    if op < 8:                                       # :877-909
        size, deflated = 0, pmd_on and rsv1
        if op == 0:
            size, deflated = st.rd_size, pmd_on and st.rd_deflated
            if size > U64 - ln:                      # :886-892
                return ERR["message_too_big"], None
        if not deflated and msg_max and (ln > msg_max or size > msg_max - ln):   # :897-906, clamp.hpp:44-51
            return ERR["message_too_big"], None
        if size + ln > out_room:                     # this library's own (include/beast_pmd.h)
            return ERR["buffer_overflow"], None
    return FRAME, Header(at, ln, fin, rsv1, op, masked, key)


def close_code_valid(v: int) -> bool:
    """is_valid_close_code (frame.hpp:94-126)"""
    if v in (1000, 1001, 1002, 1003, 1007, 1008, 1009, 1010, 1011, 1012, 1013, 1014):
        return True
    if v in (1004, 1005, 1006, 1015):
        return False
    if 1016 <= v <= 2999:
        return False
    if v <= 999:
        return False
    return True


def read_close(payload: bytes):
    """(status, code) of read_close (frame.hpp:196-240)"""
    n = len(payload)
    if n == 0:
        return 0, 0
    if n == 1:
        return ERR["bad_close_size"], 0
    code = int.from_bytes(payload[:2], "big")
    if not close_code_valid(code):
        return ERR["bad_close_code"], code
    if n > 2 and O.utf8_check(payload[2:]) != 0:
        return ERR["bad_close_payload"], code
    return 0, code


@dataclass
class Stop:
    event: int = EV_NEED_MORE
    status: int = 0
    consumed: int = 0
    out_len: int = 0        # the message's length (complete, or gathered so far)
    op: int = 0
    compressed: int = 0
    ctl: bytes = b""
    close_code: int = 0
    state: bytes = field(default_factory=lambda: State().pack())   # after the stop


def walk(b: bytes, role: int, pmd_on: bool, msg_max: int, out_cap: int, st: State, out: bytearray) -> Stop:
    """One bpmd_unframe_batch call on one entry: consumes whole frames of b up
    to the first stop, appends data payloads to out (len(out) >= out_cap is the
    slot; bytes [0, rd_size) hold the message so far) and updates st."""
    pos, s = 0, Stop()
    while True:
        r, h = parse_fh(b[pos:pos + 14], role, pmd_on, msg_max, out_cap, st)
        if r == NEED_MORE:
            break
        if r != FRAME:
            s.status = r
            break
        if h.len > len(b) - pos - h.hdr_len:         # whole frames only
            break
        body = O.mask(b[pos + h.hdr_len:pos + h.hdr_len + h.len], h.key)
        pos += h.hdr_len + h.len
        if h.op >= 8:
            s.ctl = body
            s.event = {8: EV_CLOSE, 9: EV_PING, 10: EV_PONG}[h.op]
            if h.op == 8:
                s.status, s.close_code = read_close(body)
            break
        if h.op != 0:                                # :879-883
            st.rd_size, st.rd_op, st.rd_deflated = 0, h.op, pmd_on and h.rsv1
        out[st.rd_size:st.rd_size + h.len] = body
        st.rd_size += h.len
        st.rd_cont = not h.fin                       # :907
        if h.fin:
            s.event, s.out_len, s.op, s.compressed = EV_MESSAGE, st.rd_size, st.rd_op, int(st.rd_deflated)
            st.rd_size, st.rd_cont, st.rd_op, st.rd_deflated = 0, False, 0, False
            break
    if s.event != EV_MESSAGE:
        s.out_len, s.op, s.compressed = st.rd_size, st.rd_op, int(st.rd_deflated)
    s.consumed = pos
    s.state = st.pack()
    return s


def frame(payload: bytes, op: int, fin=True, rsv=0, key=None, len_form=None) -> bytes:
    """One frame, for building streams: rsv = RSV1..3 as bits 4, 2, 1;
    len_form forces a 7 / 16 / 64-bit length field (non-canonical ones too)."""
    n = len(payload)
    form = len_form or (7 if n <= 125 else 16 if n <= 65535 else 64)
    b = bytes([(0x80 if fin else 0) | (rsv & 7) << 4 | op])
    m = 0x80 if key is not None else 0
    if form == 7:
        b += bytes([m | n])
    elif form == 16:
        b += bytes([m | 126]) + n.to_bytes(2, "big")
    else:
        b += bytes([m | 127]) + n.to_bytes(8, "big")
    if key is not None:
        b += key.to_bytes(4, "little") + O.mask(payload, key)
    else:
        b += payload
    return b
