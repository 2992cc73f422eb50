"""Expected values for the batch send side (bpmd_send_batch,
bpmd_control_batch): Beast's send decisions restated in plain Python,
independent of beast_amd/csrc.

  compress       begin_msg, websocket/impl/stream_impl.hpp:225-252
  frame_max_of   which branch of write_some a message takes and the frame size
                 it sends with, websocket/impl/write.hpp:625-831
  wire / size    the message's frames: the oracle's framer (O.frame_write,
                 bzo_frame_wire_size) at that frame size
  control        write_ping / write_close, stream_impl.hpp:915-996

The control writer is pinned by RFC 6455 5.7's examples and by
tests/frame_parse_model.py parsing its frames back (tests/test_send_plan.py).
"""
from oracle import oracle as O

SERVER, CLIENT = 0, 1
OP_TEXT, OP_BINARY, OP_CLOSE, OP_PING, OP_PONG = 1, 2, 8, 9, 10
NEED_BUFFERS, BUFFER_OVERFLOW, BAD_OPCODE, BAD_CONTROL_SIZE = 1, 257, 259, 264
CTL_SLOT, CTL_WIRE = 128, 144


def upper_bound(n: int) -> int:
    """deflate_upper_bound (zlib/deflate_stream.hpp:402-410)"""
    return n + ((n + 7) >> 3) + ((n + 63) >> 6) + 11


def compress(pmd_on: bool, opt: bool, n: int, threshold: int) -> bool:
    """begin_msg: wr_compress_ = pmd_enabled && wr_compress_opt_ && n >= msg_size_threshold"""
    return bool(pmd_on and opt and n >= threshold)


def frame_max_of(n: int, frame_max: int, compressed: bool, frag: bool) -> int:
    """The frame size the message's n wire payload bytes go out with: the
    deflate branch sends one frame per wr_buf fill whatever auto_fragment
    says (write.hpp:655-703), the plain branches do so with auto_fragment
    (:721-748, :795-829) and send one frame without (:706-720, :750-794)."""
    return frame_max if (compressed or frag) else max(n, 1)


def frame_count(n: int, frame_max: int, compressed: bool, frag: bool) -> int:
    return max(1, -(-n // frame_max_of(n, frame_max, compressed, frag)))


def wire_size(n: int, frame_max: int, masked: bool, compressed: bool, frag: bool) -> int:
    return O.lib().bzo_frame_wire_size(n, frame_max_of(n, frame_max, compressed, frag), int(masked))


def wire(payload: bytes, op: int, compressed: bool, keys, frame_max: int, frag: bool) -> bytes:
    """The message's frames; payload is what goes on the wire (the deflated
    bytes of a compressed message), keys None in server role."""
    return O.frame_write(payload, op, compressed, keys=keys,
                         frame_max=frame_max_of(len(payload), frame_max, compressed, frag))


def frame_offsets(n: int, frame_max: int, masked: bool, compressed: bool, frag: bool):
    """[(payload offset, wire offset, payload length)] of every frame, by a serial walk"""
    fm = frame_max_of(n, frame_max, compressed, frag)
    out, src, at = [], 0, 0
    for f in range(frame_count(n, frame_max, compressed, frag)):
        ln = min(fm, n - src)
        out.append((src, at, ln))
        at += (2 if ln <= 125 else 4 if ln <= 65535 else 10) + (4 if masked else 0) + ln
        src += ln
    assert at == wire_size(n, frame_max, masked, compressed, frag)
    return out


def control(op: int, slot: bytes, code: int = 0, key=None):
    """(status, frame bytes) of one bpmd_control_batch entry: slot is the
    entry's payload slot's bytes, code the close code, key None in server role."""
    slot = bytes(slot)
    if op in (OP_PING, OP_PONG):
        if len(slot) > 125:
            return BAD_CONTROL_SIZE, b""
        payload = slot
    elif op == OP_CLOSE:
        if code == 0:
            payload = b""
        elif len(slot) > 123:
            return BAD_CONTROL_SIZE, b""
        else:
            payload = code.to_bytes(2, "big") + slot
    else:
        return BAD_OPCODE, b""
    head = bytes([0x80 | op, (0x80 if key is not None else 0) | len(payload)])
    if key is None:
        return 0, head + payload
    return 0, head + (key & 0xFFFFFFFF).to_bytes(4, "little") + O.mask(payload, key)
