"""Host-side binding of the MI355X permessage-deflate engine.

The engine itself is `libbeast_pmd.so` (HIP kernels + the C ABI declared in
include/beast_pmd.h).  This module is plumbing around it: torch provides the
device memory and the stream, ctypes passes raw device pointers.  There is no
CPU fallback: if the library or a GPU is missing every call raises.

Batch layout (struct of arrays, all device tensors):
    data  uint8  [total]      payload bytes, message i at off[i] .. off[i]+len[i]
    off   int64  [n]          byte offsets (uint64 in the C ABI)
    len   int32  [n]          byte lengths (uint32 in the C ABI)
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import build as _build

_LIB = None

# zlib::error names (include/boost/beast/zlib/error.hpp:48-138)
ERRORS = ("ok", "need_buffers", "end_of_stream", "need_dict", "stream_error", "invalid_block_type",
          "invalid_stored_length", "too_many_symbols", "invalid_code_lengths", "invalid_bit_length_repeat",
          "missing_eob", "invalid_literal_length", "invalid_distance_code", "invalid_distance",
          "over_subscribed_length", "incomplete_length_set", "general")
F_RAW = 1
F_EXACT = 2   # deflate: bit-identical to Beast (BPMD_F_EXACT)
# utf8_checker verdicts (bpmd_utf8) and websocket::error::bad_frame_payload
UTF8_VALID, UTF8_INCOMPLETE, UTF8_INVALID = 0, 1, 2
BAD_FRAME_PAYLOAD = 256


class BpmdError(RuntimeError):
    pass


class _Cfg(ctypes.Structure):
    _fields_ = [("level", ctypes.c_int), ("window_bits", ctypes.c_int), ("mem_level", ctypes.c_int),
                ("strategy", ctypes.c_int), ("flags", ctypes.c_uint32)]


def lib():
    """Load libbeast_pmd.so (building it first if this checkout has none)."""
    global _LIB
    if _LIB is None:
        # BPMD_LIB selects a diagnostic variant (e.g. libbeast_pmd_prof.so)
        path = os.environ.get("BPMD_LIB", _build.LIB)
        if not os.path.exists(path):
            _build.build()
        L = ctypes.CDLL(path)
        vp = ctypes.c_void_p
        L.bpmd_init.restype = ctypes.c_int
        L.bpmd_version.restype = ctypes.c_char_p
        L.bpmd_deflate_upper_bound.argtypes = [ctypes.c_size_t]
        L.bpmd_deflate_upper_bound.restype = ctypes.c_size_t
        L.bpmd_inflate_batch.argtypes = [ctypes.POINTER(_Cfg), vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
        L.bpmd_inflate_batch.restype = ctypes.c_int
        L.bpmd_deflate_batch.argtypes = [ctypes.POINTER(_Cfg), vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
        L.bpmd_diag_set_wave_walk.argtypes = [ctypes.c_int]
        L.bpmd_diag_bp_counters.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
        L.bpmd_inflate_reserve.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
        L.bpmd_inflate_reserve.restype = ctypes.c_int
        L.bpmd_shard_ranges.argtypes = [vp, ctypes.c_uint32, ctypes.c_int, vp]
        L.bpmd_inflate_batch_multi.argtypes = [ctypes.POINTER(_Cfg), vp, ctypes.c_int, vp]
        L.bpmd_deflate_batch_multi.argtypes = [ctypes.POINTER(_Cfg), vp, ctypes.c_int, vp]
        L.bpmd_deflate_batch.restype = ctypes.c_int
        u32 = ctypes.c_uint32
        L.bpmd_mask_batch.argtypes = [vp, vp, vp, u32, vp, vp, vp]
        L.bpmd_utf8_check_batch.argtypes = [vp, vp, vp, u32, vp, vp]
        L.bpmd_frame_wire_size.argtypes = [ctypes.c_uint64, u32, ctypes.c_int]
        L.bpmd_frame_wire_size.restype = ctypes.c_uint64
        L.bpmd_frame_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp]
        L.bpmd_unframe_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, vp, vp, vp, u32] + [vp] * 14
        L.bpmd_unframe_batch.restype = ctypes.c_int
        L.bpmd_read_batch.argtypes = [ctypes.POINTER(_Cfg), vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
        L.bpmd_write_batch.argtypes = [ctypes.POINTER(_Cfg), vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
        L.bpmd_inflate_takeover_batch.argtypes = [ctypes.POINTER(_Cfg), vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
        L.bpmd_slide_batch.argtypes = [vp, vp, vp, vp, u32, vp]
        L.bpmd_deflate_takeover_batch.argtypes = [ctypes.POINTER(_Cfg), vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
        L.bpmd_deflate_takeover_batch.restype = ctypes.c_int
        L.bpmd_batcher_create.argtypes = [ctypes.POINTER(_Cfg), ctypes.c_int, u32, ctypes.c_size_t, ctypes.c_size_t,
                                          u32, ctypes.POINTER(vp)]
        L.bpmd_batcher_submit.argtypes = [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp]
        L.bpmd_batcher_flush.argtypes = [vp]
        L.bpmd_batcher_destroy.argtypes = [vp]
        L.bpmd_batcher_destroy.restype = None
        for f in ("bpmd_batcher_create", "bpmd_batcher_submit", "bpmd_batcher_flush", "bpmd_mask_batch", "bpmd_utf8_check_batch", "bpmd_read_batch", "bpmd_write_batch",
                  "bpmd_inflate_takeover_batch", "bpmd_slide_batch"):
            getattr(L, f).restype = ctypes.c_int
        _LIB = L
    return _LIB


def _check(r: int, what: str):
    if r != 0:
        names = {-1: "invalid_argument", -2: "domain_error", -3: "hip_error", -4: "no_device"}
        raise BpmdError(f"{what}: {names.get(r, r)}")


def _ptr(t: torch.Tensor):
    return ctypes.c_void_p(t.data_ptr())


def _stream_handle(stream):
    if stream is None:
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def _on(stream):
    """torch work that follows a launch on `stream` runs on it too"""
    return contextlib.nullcontext() if stream is None else torch.cuda.stream(stream)


def upper_bound(n: int) -> int:
    """deflate_upper_bound (include/boost/beast/zlib/deflate_stream.hpp:402-410)."""
    return lib().bpmd_deflate_upper_bound(n)


def slot_offsets(cap: torch.Tensor, align: int = 16) -> torch.Tensor:
    """Exclusive prefix sum of slot capacities rounded up to `align` bytes."""
    c = (cap.to(torch.int64) + (align - 1)) // align * align
    off = torch.zeros_like(c)
    if c.numel() > 1:
        off[1:] = torch.cumsum(c[:-1], 0)
    return off


@dataclass
class Batch:
    data: torch.Tensor   # uint8
    off: torch.Tensor    # int64
    len: torch.Tensor    # int32

    @property
    def n(self) -> int:
        return int(self.len.numel())

    def message(self, i: int) -> bytes:
        o, l = int(self.off[i]), int(self.len[i])
        return bytes(self.data[o:o + l].cpu().numpy().tobytes())

    @staticmethod
    def from_host(msgs, device="cuda", align: int = 16) -> "Batch":
        """Pack a list of bytes (or numpy arrays) into one device batch."""
        lens = np.array([len(m) for m in msgs], dtype=np.int64)
        pad = (lens + (align - 1)) // align * align
        off = np.zeros(len(msgs), dtype=np.int64)
        if len(msgs) > 1:
            off[1:] = np.cumsum(pad[:-1])
        buf = np.zeros(int(pad.sum()) + 16, dtype=np.uint8)
        for i, m in enumerate(msgs):
            a = np.frombuffer(bytes(m), dtype=np.uint8) if not isinstance(m, np.ndarray) else m
            buf[off[i]:off[i] + len(a)] = a
        return Batch(torch.from_numpy(buf).to(device), torch.from_numpy(off).to(device),
                     torch.from_numpy(lens.astype(np.int32)).to(device))

    @staticmethod
    def from_arrays(data: np.ndarray, off: np.ndarray, lens: np.ndarray, device="cuda") -> "Batch":
        d = torch.from_numpy(np.ascontiguousarray(data, dtype=np.uint8))
        return Batch(d.to(device), torch.from_numpy(np.asarray(off, dtype=np.int64)).to(device),
                     torch.from_numpy(np.asarray(lens, dtype=np.int32)).to(device))

    def to_host(self):
        return [self.message(i) for i in range(self.n)]


@dataclass
class Result:
    out: Batch           # out.len = produced bytes
    cap: torch.Tensor    # int32 slot capacities
    status: torch.Tensor  # int32 zlib::error per message


def inflate_batch(src: Batch, out_cap, window_bits: int = 15, raw: bool = False, stream=None,
                  out: torch.Tensor | None = None, out_off: torch.Tensor | None = None) -> Result:
    """Inflate every message of `src` on the current GPU (asynchronous on `stream`).

    `out_cap` (int or int32 tensor): output capacity per message.  Messages
    that would produce more report status need_buffers and keep `cap` bytes.
    """
    L = lib()
    dev = src.data.device
    n = src.n
    if isinstance(out_cap, int):
        cap = torch.full((n,), out_cap, dtype=torch.int32, device=dev)
    else:
        cap = out_cap.to(device=dev, dtype=torch.int32)
    if out_off is None:
        out_off = slot_offsets(cap)
    if out is None:
        total = int(out_off[-1].item() + cap[-1].item()) if n else 0
        out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    cfg = _Cfg(0, window_bits, 8, 0, F_RAW if raw else 0)
    _check(L.bpmd_inflate_batch(ctypes.byref(cfg), _ptr(src.data), _ptr(src.off), _ptr(src.len), n, _ptr(out),
                                _ptr(out_off), _ptr(cap), _ptr(out_len), _ptr(status), _stream_handle(stream)),
           "bpmd_inflate_batch")
    return Result(Batch(out, out_off, out_len), cap, status)


def inflate_reserve(in_bytes: int, out_bytes: int, n_long: int, stream=None) -> None:
    """bpmd_inflate_reserve: size `stream`'s block-parallel decode workspace
    for batches whose long payloads total at most in_bytes / out_bytes /
    n_long, so that no call on it waits to size it (include/beast_pmd.h)."""
    _check(lib().bpmd_inflate_reserve(_stream_handle(stream), in_bytes, out_bytes, n_long), "bpmd_inflate_reserve")


def bp_counters(reset: bool = True) -> list:
    """bpmd_diag_bp_counters: [0] payloads resolved block-parallel, [1] their
    segments, [2] resolve fallbacks to the wave kernel, [3] capacity spills
    to it (pmd_inflate_bp.hip)."""
    c = (ctypes.c_ulonglong * 12)()
    _check(lib().bpmd_diag_bp_counters(c, 1 if reset else 0), "bpmd_diag_bp_counters")
    return list(c)


def deflate_batch(src: Batch, level: int = 6, window_bits: int = 15, mem_level: int = 4, strategy: int = 0,
                  stream=None, out_cap=None, out: torch.Tensor | None = None,
                  out_off: torch.Tensor | None = None, exact: bool = False) -> Result:
    """Deflate every message of `src` into a permessage-deflate payload
    (tail stripped) on the current GPU, asynchronous on `stream`.

    Slots default to deflate_upper_bound(len) bytes, which always suffices.
    exact=True (BPMD_F_EXACT): payloads bit-identical to Beast's deflater.
    """
    L = lib()
    dev = src.data.device
    n = src.n
    if out_cap is None:
        ln = src.len.to(torch.int64)
        cap = (ln + (ln + 7) // 8 + (ln + 63) // 64 + 11).to(torch.int32)
    elif isinstance(out_cap, int):
        cap = torch.full((n,), out_cap, dtype=torch.int32, device=dev)
    else:
        cap = out_cap.to(device=dev, dtype=torch.int32)
    if out_off is None:
        out_off = slot_offsets(cap)
    if out is None:
        total = int(out_off[-1].item() + cap[-1].item()) if n else 0
        out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    cfg = _Cfg(level, window_bits, mem_level, strategy, F_EXACT if exact else 0)
    _check(L.bpmd_deflate_batch(ctypes.byref(cfg), _ptr(src.data), _ptr(src.off), _ptr(src.len), n, _ptr(out),
                                _ptr(out_off), _ptr(cap), _ptr(out_len), _ptr(status), _stream_handle(stream)),
           "bpmd_deflate_batch")
    return Result(Batch(out, out_off, out_len), cap, status)


# ------------------------------------------------------------------------
# Frame passes

def _optr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _keys(key, n: int, dev):
    """Per-message 32-bit masking keys (frame-header order, stream_impl.hpp:866-870)
    as an int32 device tensor holding the same bits; None stays None."""
    if key is None:
        return None
    if isinstance(key, torch.Tensor):
        if key.dtype == torch.int32:
            return key.to(dev).contiguous()
        key = key.cpu().numpy()
    a = np.array(np.broadcast_to(np.asarray(key, dtype=np.int64) & 0xFFFFFFFF, (n,)), dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32)).to(dev)


def _u8(v, n: int, dev):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        return v.to(device=dev, dtype=torch.uint8).contiguous()
    a = np.array(np.broadcast_to(np.asarray(v, dtype=np.uint8), (n,)), dtype=np.uint8)
    return torch.from_numpy(a).to(dev)


def mask_batch(b: Batch, key, phase=None, stream=None) -> None:
    """Beast's mask_inplace (websocket/detail/mask.ipp:38-59) over every message
    of `b`, in place; `phase` = bytes of the frame already masked, mod 4."""
    L = lib()
    dev = b.data.device
    k = _keys(key, b.n, dev)
    ph = _u8(phase, b.n, dev)
    _check(L.bpmd_mask_batch(_ptr(b.data), _ptr(b.off), _ptr(b.len), b.n, _optr(k), _optr(ph),
                             _stream_handle(stream)), "bpmd_mask_batch")


def frame_counts(lens: torch.Tensor, frame_max: int) -> torch.Tensor:
    """Frames per message (an empty payload is one empty frame)."""
    lens = lens.to(torch.int64)
    return torch.clamp((lens + frame_max - 1) // frame_max, min=1)


def frame_wire_sizes(lens: torch.Tensor, frame_max: int, masked: bool) -> torch.Tensor:
    """bpmd_frame_wire_size per message, on the lengths' device."""
    lens = lens.to(torch.int64)
    k = frame_counts(lens, frame_max)
    last = lens - (k - 1) * frame_max
    hdr = lambda x: torch.where(x <= 125, 2, torch.where(x <= 65535, 4, 10)) + (4 if masked else 0)  # noqa: E731
    full = torch.full_like(lens, frame_max)
    return lens + (k - 1) * hdr(full) + hdr(last)


def frame_plan(b: Batch, frame_max: int = 4096, masked: bool = False):
    """Wire sizes, wire offsets, total bytes and (masked) each message's first
    key index for bpmd_frame_batch; reusable across calls on same-shaped batches."""
    dev = b.data.device
    n = b.n
    sizes = frame_wire_sizes(b.len, frame_max, masked)
    woff = torch.zeros(n, dtype=torch.int64, device=dev)
    if n > 1:
        woff[1:] = torch.cumsum(sizes, 0)[:-1]
    total = int(sizes.sum().item()) if n else 0
    kb = nkeys = None
    if masked:
        cnt = frame_counts(b.len, frame_max)
        nkeys = int(cnt.sum().item())
        kb = torch.zeros(n, dtype=torch.int32, device=dev)
        if n > 1:
            kb[1:] = torch.cumsum(cnt, 0)[:-1].to(torch.int32)
    return {"frame_max": frame_max, "masked": masked, "sizes": sizes.to(torch.int32), "woff": woff, "total": total,
            "key_base": kb, "n_keys": nkeys}


def frame_batch(b: Batch, frame_max: int = 4096, op=2, compressed=True, keys=None, stream=None, plan=None,
                wire: torch.Tensor | None = None) -> Batch:
    """The wire bytes of every message of `b` (write.hpp:463-545 frame loop,
    frame.hpp:134-175 headers): frames of at most frame_max payload bytes,
    opcode `op` (per message or one value) and RSV1 when `compressed` on the
    first frame, FIN on the last; `keys` (client role) holds one key per
    frame, message by message (frame_counts gives how many), and masks each
    frame with its own key.  Returns one wire message per input message;
    `plan` (frame_plan) and `wire` skip the sizing and allocation."""
    L = lib()
    dev = b.data.device
    n = b.n
    masked = keys is not None
    if plan is None:
        plan = frame_plan(b, frame_max, masked)
    if plan["frame_max"] != frame_max or plan["masked"] != masked:
        raise BpmdError("frame_batch: plan made for another frame size or role")
    if wire is None:
        wire = torch.empty(plan["total"] + 16, dtype=torch.uint8, device=dev)
    opt = _u8(op, n, dev)
    fl = _u8(1 if compressed is True else 0 if compressed is False else compressed, n, dev)
    kt = None
    if masked:
        nk = int(keys.numel()) if isinstance(keys, torch.Tensor) else len(keys)
        kt = _keys(keys, nk, dev)
        if kt.numel() < plan["n_keys"]:
            raise BpmdError("frame_batch: keys must hold one key per frame (frame_counts)")
    _check(L.bpmd_frame_batch(_ptr(b.data), _ptr(b.off), _ptr(b.len), _optr(opt), _optr(fl), _optr(kt),
                              _optr(plan["key_base"]), frame_max, n, _ptr(wire), _ptr(plan["woff"]),
                              _stream_handle(stream)), "bpmd_frame_batch")
    return Batch(wire, plan["woff"], plan["sizes"])


def utf8_check_batch(b: Batch, stream=None, result: torch.Tensor | None = None) -> torch.Tensor:
    """utf8_checker verdict per message (UTF8_VALID / UTF8_INCOMPLETE / UTF8_INVALID)."""
    L = lib()
    res = result if result is not None else torch.empty(b.n, dtype=torch.int32, device=b.data.device)
    _check(L.bpmd_utf8_check_batch(_ptr(b.data), _ptr(b.off), _ptr(b.len), b.n, _ptr(res), _stream_handle(stream)),
           "bpmd_utf8_check_batch")
    return res


def _out_slots(n: int, dev, out_cap, out, out_off):
    if isinstance(out_cap, int):
        cap = torch.full((n,), out_cap, dtype=torch.int32, device=dev)
    else:
        cap = out_cap.to(device=dev, dtype=torch.int32)
    if out_off is None:
        out_off = slot_offsets(cap)
    if out is None:
        total = int(out_off[-1].item() + cap[-1].item()) if n else 0
        out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    return cap, out, out_off


def read_batch(src: Batch, out_cap, key=None, text=None, window_bits: int = 15, raw: bool = False, stream=None,
               out: torch.Tensor | None = None, out_off: torch.Tensor | None = None) -> Result:
    """Receive path, fused (read.hpp:1284-1385): unmask with `key` (per message,
    or None), inflate, and check the output of `text` messages; a text message
    that is not UTF-8 gets status BAD_FRAME_PAYLOAD.  `src` is not modified."""
    L = lib()
    dev = src.data.device
    n = src.n
    cap, out, out_off = _out_slots(n, dev, out_cap, out, out_off)
    k = _keys(key, n, dev)
    t = _u8(text, n, dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    cfg = _Cfg(0, window_bits, 8, 0, F_RAW if raw else 0)
    _check(L.bpmd_read_batch(ctypes.byref(cfg), _ptr(src.data), _ptr(src.off), _ptr(src.len), _optr(k), _optr(t), n,
                             _ptr(out), _ptr(out_off), _ptr(cap), _ptr(out_len), _ptr(status), _stream_handle(stream)),
           "bpmd_read_batch")
    return Result(Batch(out, out_off, out_len), cap, status)


def write_batch(src: Batch, key=None, level: int = 6, window_bits: int = 15, mem_level: int = 4, strategy: int = 0,
                stream=None, out_cap=None, out: torch.Tensor | None = None,
                out_off: torch.Tensor | None = None, exact: bool = False) -> Result:
    """Send path, fused (write.hpp:655-703): deflate_batch with each payload
    masked by `key` in the kernel's output stores (client role)."""
    L = lib()
    dev = src.data.device
    n = src.n
    if out_cap is None:
        ln = src.len.to(torch.int64)
        out_cap = (ln + (ln + 7) // 8 + (ln + 63) // 64 + 11).to(torch.int32)
    cap, out, out_off = _out_slots(n, dev, out_cap, out, out_off)
    k = _keys(key, n, dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    cfg = _Cfg(level, window_bits, mem_level, strategy, F_EXACT if exact else 0)
    _check(L.bpmd_write_batch(ctypes.byref(cfg), _ptr(src.data), _ptr(src.off), _ptr(src.len), _optr(k), n,
                              _ptr(out), _ptr(out_off), _ptr(cap), _ptr(out_len), _ptr(status),
                              _stream_handle(stream)), "bpmd_write_batch")
    return Result(Batch(out, out_off, out_len), cap, status)


# ------------------------------------------------------------------------
# Receive side: wire bytes -> frames -> messages (bpmd_unframe_batch)

ROLE_SERVER, ROLE_CLIENT = 0, 1
# bpmd_event: what stopped an entry's walk
EV_NEED_MORE, EV_MESSAGE, EV_PING, EV_PONG, EV_CLOSE = 0, 1, 2, 3, 4
# bpmd_ws_error: websocket::error values of the status array (websocket/error.hpp)
WS_ERRORS = {256: "bad_frame_payload", 257: "buffer_overflow", 258: "message_too_big", 259: "bad_opcode",
             260: "bad_data_frame", 261: "bad_continuation", 262: "bad_reserved_bits", 263: "bad_control_fragment",
             264: "bad_control_size", 265: "bad_unmasked_frame", 266: "bad_masked_frame", 267: "bad_size",
             268: "bad_close_code", 269: "bad_close_size", 270: "bad_close_payload"}
(WS_BUFFER_OVERFLOW, WS_MESSAGE_TOO_BIG, WS_BAD_OPCODE, WS_BAD_DATA_FRAME, WS_BAD_CONTINUATION, WS_BAD_RESERVED_BITS,
 WS_BAD_CONTROL_FRAGMENT, WS_BAD_CONTROL_SIZE, WS_BAD_UNMASKED_FRAME, WS_BAD_MASKED_FRAME, WS_BAD_SIZE,
 WS_BAD_CLOSE_CODE, WS_BAD_CLOSE_SIZE, WS_BAD_CLOSE_PAYLOAD) = range(257, 271)
CTL_SLOT = 128        # bytes of an entry's control payload slot
RD_STATE_BYTES = 16   # sizeof(bpmd_rd_state)


def rd_state(n: int, device="cuda") -> torch.Tensor:
    """n bpmd_rd_state records, all between messages (uint8 [n, 16]: rd_size
    little-endian in bytes 0-7, then rd_cont, rd_op, rd_deflated)."""
    return torch.zeros((n, RD_STATE_BYTES), dtype=torch.uint8, device=device)


@dataclass
class Unframed:
    out: Batch                 # gathered payloads: out.len = bytes of the message (complete or in progress)
    cap: torch.Tensor          # int32 slot capacities
    op: torch.Tensor           # uint8: 1 text, 2 binary
    compressed: torch.Tensor   # uint8: the message's RSV1
    event: torch.Tensor        # uint8 EV_*
    status: torch.Tensor       # int32: 0 or a WS_* error
    consumed: torch.Tensor     # int32 wire bytes consumed
    ctl: torch.Tensor          # uint8 [n, 128] control payloads
    ctl_len: torch.Tensor      # uint8
    close_code: torch.Tensor   # int32 (0 = none)
    state: torch.Tensor | None  # uint8 [n, 16], the caller's, updated in place


def unframe_batch(wire: Batch, out_cap, role: int, pmd_on: bool = True, msg_max: int = 16 << 20,
                  state: torch.Tensor | None = None, out: torch.Tensor | None = None,
                  out_off: torch.Tensor | None = None, stream=None) -> Unframed:
    """bpmd_unframe_batch: walk the frames of every entry of `wire` as
    read_some does around parse_fh (read.hpp:1063-1283, stream_impl.hpp:
    701-913), unmask data payloads into the entry's out slot and stop at the
    first complete message, control frame, refused header or end of buffer
    (include/beast_pmd.h).  Whole frames only: drop `consumed` bytes of each
    entry, keep the rest and call again with the same `state` (rd_state) and
    out slots; `state` None starts every entry between messages."""
    L = lib()
    dev = wire.data.device
    n = wire.n
    cap, out, out_off = _out_slots(n, dev, out_cap, out, out_off)
    if state is not None and (state.dtype != torch.uint8 or state.numel() != n * RD_STATE_BYTES
                              or not state.is_contiguous()):
        raise BpmdError("unframe_batch: state must be rd_state(n)")
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    op, comp, event, ctl_len, ctl = u8(n), u8(n), u8(n), u8(n), u8(n, CTL_SLOT)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    consumed = torch.empty(n, dtype=torch.int32, device=dev)
    code = torch.empty(n, dtype=torch.int16, device=dev)
    _check(L.bpmd_unframe_batch(role, 1 if pmd_on else 0, msg_max, _ptr(wire.data), _ptr(wire.off), _ptr(wire.len), n,
                                _optr(state), _ptr(out), _ptr(out_off), _ptr(cap), _ptr(out_len), _ptr(op),
                                _ptr(comp), _ptr(event), _ptr(status), _ptr(consumed), _ptr(ctl), _ptr(ctl_len),
                                _ptr(code), _stream_handle(stream)), "bpmd_unframe_batch")
    with _on(stream):
        code = code.to(torch.int32) & 0xFFFF
    return Unframed(Batch(out, out_off, out_len), cap, op, comp, event, status, consumed, ctl, ctl_len, code, state)


@dataclass
class Received:
    frames: Unframed            # the frame pass's results, entry by entry
    event: torch.Tensor         # uint8 EV_* (frames.event)
    status: torch.Tensor        # int32: the frame status, else the message's read_batch status
    inflated: Result | None     # read_batch over the entries in `inflated_idx`
    inflated_idx: torch.Tensor  # int64: entries that completed a compressed message

    def to_host(self):
        """Per entry: the message's bytes after EV_MESSAGE (inflated if it was
        compressed), else None."""
        ev = self.event.cpu().tolist()
        plain = self.frames.out
        msgs = [plain.message(i) if e == EV_MESSAGE else None for i, e in enumerate(ev)]
        for j, i in enumerate(self.inflated_idx.cpu().tolist()):
            msgs[i] = self.inflated.out.message(j)
        return msgs


def receive_batch(wire: Batch, out_cap, inflate_cap, role: int, pmd_on: bool = True, msg_max: int = 16 << 20,
                  state: torch.Tensor | None = None, out: torch.Tensor | None = None,
                  out_off: torch.Tensor | None = None, window_bits: int = 15, stream=None) -> Received:
    """From wire bytes to messages (read.hpp:1063-1385): unframe_batch, then
    read_batch (inflate + UTF-8 check of text) over the entries that completed
    a compressed message -- a batch over the same out buffer with the gathered
    offsets and lengths, `inflate_cap` output bytes each (Beast checks
    rd_msg_max while inflating, read.hpp:1357-1366; here need_buffers says the
    message outgrew inflate_cap) -- and utf8_check_batch over the complete
    uncompressed text messages, which keep their gathered payload.  A text
    message that is not UTF-8 gets BAD_FRAME_PAYLOAD.  Picking the entries
    waits for the frame pass."""
    with _on(stream):
        return _receive(wire, out_cap, inflate_cap, role, pmd_on, msg_max, state, out, out_off, window_bits, stream)


def _receive(wire, out_cap, inflate_cap, role, pmd_on, msg_max, state, out, out_off, window_bits, stream):
    u = unframe_batch(wire, out_cap, role, pmd_on, msg_max, state, out, out_off, stream)
    status = u.status.clone()
    done = (u.event == EV_MESSAGE) & (u.status == 0)
    zi = torch.nonzero(done & (u.compressed != 0)).flatten()
    ti = torch.nonzero(done & (u.compressed == 0) & (u.op == 1)).flatten()
    inflated = None
    if zi.numel():
        sub = Batch(u.out.data, u.out.off[zi].contiguous(), u.out.len[zi].contiguous())
        icap = inflate_cap if isinstance(inflate_cap, int) else inflate_cap.to(u.out.data.device)[zi].contiguous()
        inflated = read_batch(sub, icap, key=None, text=(u.op[zi] == 1), window_bits=window_bits, stream=stream)
        status[zi] = inflated.status
    if ti.numel():
        sub = Batch(u.out.data, u.out.off[ti].contiguous(), u.out.len[ti].contiguous())
        verdict = utf8_check_batch(sub, stream=stream)
        status[ti] = torch.where(verdict != 0, BAD_FRAME_PAYLOAD, 0).to(torch.int32)
    return Received(u, u.event, status, inflated, zi)


def _recv_lib():
    """lib() with bpmd_receive_batch's prototype, bound on first use so that a
    BPMD_LIB variant built without it still serves every other call"""
    L = lib()
    if not getattr(L, "_recv_ready", False):
        vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        L.bpmd_receive_work_bytes.argtypes = [u32]
        L.bpmd_receive_work_bytes.restype = ctypes.c_size_t
        L.bpmd_receive_batch.argtypes = [ctypes.POINTER(_Cfg), ci, ci, ctypes.c_uint64, vp, vp, vp, u32] + [vp] * 19
        L.bpmd_receive_batch.restype = ci
        L._recv_ready = True
    return L


def _host_slots(what: str, n: int, dev, cap, buf, off):
    """_out_slots without a wait: one capacity for all entries sizes the
    buffer on the host; capacities in a tensor need the caller's buffer."""
    if isinstance(cap, int):
        stride = (cap + 15) // 16 * 16
        if off is None:
            off = torch.arange(n, dtype=torch.int64, device=dev) * stride
        if buf is None:
            buf = torch.empty(n * stride + 16, dtype=torch.uint8, device=dev)
        return torch.full((n,), cap, dtype=torch.int32, device=dev), buf, off
    if buf is None or off is None:
        raise BpmdError(f"recv_batch: {what} capacities in a tensor need the {what} buffer and its offsets")
    return cap.to(device=dev, dtype=torch.int32), buf, off


@dataclass
class Recv:
    frames: Unframed       # the frame pass's results, entry by entry; frames.out holds the uncompressed messages
    msg: Batch             # the inflated messages' slots; msg.len = every complete message's length (d_msg_len)
    event: torch.Tensor    # uint8 EV_* (frames.event)
    status: torch.Tensor   # int32: 0, a WS_* error, BAD_FRAME_PAYLOAD or a zlib::error (frames.status, merged in place)

    def to_host(self):
        """Per entry: the message's bytes after EV_MESSAGE with status 0 or
        BAD_FRAME_PAYLOAD (from the slot frames.compressed names), else None."""
        ev, st = self.event.cpu().tolist(), self.status.cpu().tolist()
        comp, ln = self.frames.compressed.cpu().tolist(), self.msg.len.cpu().tolist()
        msgs = []
        for i, e in enumerate(ev):
            if e != EV_MESSAGE or st[i] not in (0, BAD_FRAME_PAYLOAD):
                msgs.append(None)
                continue
            b = self.msg if comp[i] else self.frames.out
            o = int(b.off[i])
            msgs.append(bytes(b.data[o:o + ln[i]].cpu().numpy().tobytes()))
        return msgs


def recv_batch(wire: Batch, out_cap, msg_cap, role: int, pmd_on: bool = True, msg_max: int = 16 << 20,
               state: torch.Tensor | None = None, out: torch.Tensor | None = None,
               out_off: torch.Tensor | None = None, msg: torch.Tensor | None = None,
               msg_off: torch.Tensor | None = None, window_bits: int = 15, stream=None) -> Recv:
    """bpmd_receive_batch: from wire bytes to checked messages in one chained
    call (read.hpp:1063-1385): the frame pass of unframe_batch, the inflater
    over the entries that completed a compressed message (gathered slot ->
    message slot of `msg_cap` bytes), rd_msg_max on the inflated size
    (WS_MESSAGE_TOO_BIG; WS_BUFFER_OVERFLOW when the slot is the smaller) and
    the UTF-8 check of text where the message lies (BAD_FRAME_PAYLOAD).
    Everything is enqueued on `stream` and the call never waits: `out_cap` /
    `msg_cap` as one int size their buffers here, as tensors they need `out` +
    `out_off` / `msg` + `msg_off`.  With pmd_on False nothing is inflated and
    `msg` has no bytes."""
    L = _recv_lib()
    dev = wire.data.device
    n = wire.n
    if state is not None and (state.dtype != torch.uint8 or state.numel() != n * RD_STATE_BYTES
                              or not state.is_contiguous()):
        raise BpmdError("recv_batch: state must be rd_state(n)")
    with _on(stream):
        cap, out, out_off = _host_slots("out", n, dev, out_cap, out, out_off)
        out_len = torch.empty(n, dtype=torch.int32, device=dev)
        u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        op, comp, event, ctl_len, ctl = u8(n), u8(n), u8(n), u8(n), u8(n, CTL_SLOT)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        consumed = torch.empty(n, dtype=torch.int32, device=dev)
        code = torch.empty(n, dtype=torch.int16, device=dev)
        msg_len = torch.empty(n, dtype=torch.int32, device=dev)
        mcap = work = None
        if pmd_on:
            mcap, msg, msg_off = _host_slots("msg", n, dev, msg_cap, msg, msg_off)
            work = u8(max(int(L.bpmd_receive_work_bytes(n)), 1))
        else:
            msg, msg_off = u8(0), torch.zeros(n, dtype=torch.int64, device=dev)
    cfg = _Cfg(0, window_bits, 8, 0, 0)
    _check(L.bpmd_receive_batch(ctypes.byref(cfg) if pmd_on else None, role, 1 if pmd_on else 0, msg_max, _ptr(wire.data), _ptr(wire.off),
                                _ptr(wire.len), n, _optr(state), _ptr(out), _ptr(out_off), _ptr(cap), _ptr(out_len),
                                _ptr(op), _ptr(comp), _ptr(event), _ptr(status), _ptr(consumed), _ptr(ctl),
                                _ptr(ctl_len), _ptr(code), _ptr(msg) if pmd_on else None,
                                _ptr(msg_off) if pmd_on else None, _optr(mcap), _ptr(msg_len), _optr(work),
                                _stream_handle(stream)), "bpmd_receive_batch")
    with _on(stream):
        code = code.to(torch.int32) & 0xFFFF
    frames = Unframed(Batch(out, out_off, out_len), cap, op, comp, event, status, consumed, ctl, ctl_len, code, state)
    return Recv(frames, Batch(msg, msg_off, msg_len), event, status)


# ------------------------------------------------------------------------
# Context takeover

def _check_unique(conn, n):
    """One message per connection per call: two messages of one connection
    would share an output position and history and overwrite each other."""
    if n and int(torch.unique(conn).numel()) != n:
        raise BpmdError("a connection appears more than once in one batch; submit its messages in separate calls")


class TakeoverInflater:
    """Receive side of context-takeover connections: Beast's inflater keeps its
    window across messages (impl_base.hpp:192-202; inflate_stream::clear() is a
    no-op, inflate_stream.ipp:49-53).  Each connection owns a device buffer of
    2 * 2^window_bits + max_msg bytes holding its latest output; message k of a
    connection is decoded right after its earlier output, whose last
    2^window_bits bytes are the window.  When a buffer cannot take the next
    message, its window slides to the front on the device (bpmd_slide_batch).
    Bookkeeping stays on the device except for that fullness test."""

    def __init__(self, n_conn: int, window_bits: int = 15, max_msg: int = 1 << 16, device="cuda"):
        self.wbits = window_bits
        self.W = 1 << window_bits
        self.max_msg = max_msg
        self.slot = (2 * self.W + max_msg + 15) // 16 * 16
        self.buf = torch.zeros(n_conn * self.slot + 16, dtype=torch.uint8, device=device)
        self.base = torch.arange(n_conn, dtype=torch.int64, device=device) * self.slot
        self.pos = torch.zeros(n_conn, dtype=torch.int64, device=device)

    def inflate(self, src: Batch, out_cap, conn=None, stream=None) -> Result:
        """Inflate src's messages, message i continuing connection conn[i]
        (default i); at most one message per connection per call."""
        L = lib()
        dev = self.buf.device
        n = src.n
        conn = torch.arange(n, device=dev) if conn is None else torch.as_tensor(conn, device=dev).long()
        _check_unique(conn, n)
        cap = torch.full((n,), out_cap, dtype=torch.int32, device=dev) if isinstance(out_cap, int) \
            else out_cap.to(device=dev, dtype=torch.int32)
        if int(cap.max().item() if n else 0) > self.max_msg:
            raise BpmdError("out_cap exceeds max_msg")
        pos = self.pos[conn]
        full = pos + cap.to(torch.int64) > self.slot
        if n and bool(full.any()):
            idx = conn[full]
            keep = torch.minimum(self.pos[idx], torch.tensor(self.W, device=dev))
            p32 = self.pos[idx].to(torch.int32)
            k32 = keep.to(torch.int32)
            b64 = self.base[idx].contiguous()
            _check(L.bpmd_slide_batch(_ptr(self.buf), _ptr(b64), _ptr(p32), _ptr(k32), int(idx.numel()),
                                      _stream_handle(stream)), "bpmd_slide_batch")
            self.pos[idx] = keep
            pos = self.pos[conn]
        hist = torch.minimum(pos, torch.tensor(self.W, device=dev)).to(torch.int32)
        out_off = (self.base[conn] + pos).contiguous()
        out_len = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        cfg = _Cfg(0, self.wbits, 8, 0, 0)
        _check(L.bpmd_inflate_takeover_batch(ctypes.byref(cfg), _ptr(src.data), _ptr(src.off), _ptr(src.len),
                                             _ptr(hist), n, _ptr(self.buf), _ptr(out_off), _ptr(cap), _ptr(out_len),
                                             _ptr(status), _stream_handle(stream)), "bpmd_inflate_takeover_batch")
        # a connection whose message failed is left where it was: its window
        # is undefined from here on (the reference's stream goes BAD), so the
        # caller drops it (check_stop_now fails the websocket connection)
        self.pos[conn] = pos + torch.where(status == 0, out_len, torch.zeros_like(out_len)).to(torch.int64)
        return Result(Batch(self.buf, out_off, out_len), cap, status)


def _recv_tk_lib():
    """lib() with bpmd_receive_takeover_batch's prototype, bound on first use
    as _recv_lib binds bpmd_receive_batch's"""
    L = lib()
    if not getattr(L, "_recv_tk_ready", False):
        vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        L.bpmd_receive_takeover_work_bytes.argtypes = [u32]
        L.bpmd_receive_takeover_work_bytes.restype = ctypes.c_size_t
        L.bpmd_receive_takeover_batch.argtypes = [ctypes.POINTER(_Cfg), ci, ctypes.c_uint64, vp, vp, vp, u32] + \
            [vp] * 15 + [u32] + [vp] * 6
        L.bpmd_receive_takeover_batch.restype = ci
        L._recv_tk_ready = True
    return L


class TakeoverReceiver:
    """bpmd_receive_takeover_batch over n_conn context-takeover connections:
    recv_batch's chained call (frame pass, inflater, rd_msg_max, UTF-8 check)
    with TakeoverInflater's buffers -- 2 * 2^window_bits + max_msg bytes per
    connection, the next message decoded right behind the earlier output, the
    window slid to the front when a message would not fit -- and that
    bookkeeping done on the device, so recv never waits.  Entry i of every
    batch is connection i.  The receiver owns the connections' buffers (`buf`,
    `base`, `pos`), their message states (`rd_state`), the gathered slots and
    the workspace; a Recv's tensors of one call are valid until the next.  A
    connection whose message fails in the inflater (a zlib::error,
    WS_BUFFER_OVERFLOW, or WS_MESSAGE_TOO_BIG with the limit outgrown) keeps
    its position and an undefined window: drop it, as with TakeoverInflater."""

    def __init__(self, n_conn: int, role: int, window_bits: int = 15, max_msg: int = 1 << 16,
                 msg_max: int = 16 << 20, device="cuda"):
        L = _recv_tk_lib()
        self.n, self.role, self.wbits, self.msg_max = n_conn, role, window_bits, msg_max
        self.W = 1 << window_bits
        self.max_msg = max_msg
        self.slot = (2 * self.W + max_msg + 15) // 16 * 16
        self.buf = torch.zeros(n_conn * self.slot + 16, dtype=torch.uint8, device=device)
        self.base = torch.arange(n_conn, dtype=torch.int64, device=device) * self.slot
        self.pos = torch.zeros(n_conn, dtype=torch.int32, device=device)
        self.rd_state = rd_state(n_conn, device)
        self.work = torch.empty(max(int(L.bpmd_receive_takeover_work_bytes(n_conn)), 1), dtype=torch.uint8,
                                device=device)
        self._out_cap = self._out = self._out_off = None

    def recv(self, wire: Batch, out_cap: int, msg_cap=None, stream=None) -> Recv:
        """One call over wire (entry i: connection i's bytes; an idle connection
        sends length 0).  `out_cap`: bytes of every gathered slot, one int, the
        same in every call (the slots keep a message's fragments from call to
        call).  `msg_cap`: the most a message may inflate to, one int or an
        int32 tensor, default and at most max_msg.  Recv.msg is Batch(buf,
        msg_off, msg_len): an inflated message lies in its connection's buffer,
        an uncompressed one in frames.out."""
        L = _recv_tk_lib()
        dev = self.buf.device
        n = wire.n
        if n != self.n:
            raise BpmdError("TakeoverReceiver.recv: one entry per connection")
        if not isinstance(out_cap, int) or (self._out_cap is not None and out_cap != self._out_cap):
            raise BpmdError("TakeoverReceiver.recv: out_cap is one int, the same in every call")
        if isinstance(msg_cap, int) and msg_cap > self.max_msg:
            raise BpmdError("msg_cap exceeds max_msg")
        with _on(stream):
            if self._out_cap is None:
                _, self._out, self._out_off = _host_slots("out", n, dev, out_cap, None, None)
                self._out_cap = out_cap
            cap = torch.full((n,), out_cap, dtype=torch.int32, device=dev)
            if msg_cap is None or isinstance(msg_cap, int):
                mcap = torch.full((n,), self.max_msg if msg_cap is None else msg_cap, dtype=torch.int32, device=dev)
            else:   # the call itself clamps a capacity to the room of a connection's buffer
                mcap = msg_cap.to(device=dev, dtype=torch.int32)
            out_len = torch.empty(n, dtype=torch.int32, device=dev)
            u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)  # noqa: E731
            op, comp, event, ctl_len, ctl = u8(n), u8(n), u8(n), u8(n), u8(n, CTL_SLOT)
            status = torch.empty(n, dtype=torch.int32, device=dev)
            consumed = torch.empty(n, dtype=torch.int32, device=dev)
            code = torch.empty(n, dtype=torch.int16, device=dev)
            msg_len = torch.empty(n, dtype=torch.int32, device=dev)
            msg_off = torch.empty(n, dtype=torch.int64, device=dev)
        cfg = _Cfg(0, self.wbits, 8, 0, 0)
        _check(L.bpmd_receive_takeover_batch(
            ctypes.byref(cfg), self.role, self.msg_max, _ptr(wire.data), _ptr(wire.off), _ptr(wire.len), n,
            _ptr(self.rd_state), _ptr(self._out), _ptr(self._out_off), _ptr(cap), _ptr(out_len), _ptr(op), _ptr(comp),
            _ptr(event), _ptr(status), _ptr(consumed), _ptr(ctl), _ptr(ctl_len), _ptr(code), _ptr(self.buf),
            _ptr(self.base), self.slot, _ptr(self.pos), _ptr(mcap), _ptr(msg_off), _ptr(msg_len), _ptr(self.work),
            _stream_handle(stream)), "bpmd_receive_takeover_batch")
        with _on(stream):
            code = code.to(torch.int32) & 0xFFFF
        frames = Unframed(Batch(self._out, self._out_off, out_len), cap, op, comp, event, status, consumed, ctl,
                          ctl_len, code, self.rd_state)
        return Recv(frames, Batch(self.buf, msg_off, msg_len), event, status)


# ------------------------------------------------------------------------
# Cross-connection micro-batcher

_DONE = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int32, ctypes.c_size_t)


class Completion:
    """Result of one submitted message: wait() returns (status, bytes)."""

    def __init__(self, cap: int):
        import threading
        self.buf = ctypes.create_string_buffer(max(cap, 1))
        self.cap = cap
        self.event = threading.Event()
        self.status = None
        self.length = 0

    def wait(self, timeout=None):
        if not self.event.wait(timeout):
            raise TimeoutError("message not completed")
        return self.status, self.buf.raw[:self.length]


class Batcher:
    """Host-buffer front end that coalesces single messages from many
    connections (threads) into batch launches (bpmd_batcher_*)."""

    def __init__(self, op: str = "inflate", level: int = 6, window_bits: int = 15, mem_level: int = 4,
                 strategy: int = 0, raw: bool = False, max_msgs: int = 4096, max_in_bytes: int = 16 << 20,
                 max_out_bytes: int = 64 << 20, max_delay_us: int = 200):
        import threading
        self.L = lib()
        self.op = op
        cfg = _Cfg(level, window_bits, mem_level, strategy, F_RAW if raw else 0)
        h = ctypes.c_void_p()
        _check(self.L.bpmd_batcher_create(ctypes.byref(cfg), 0 if op == "inflate" else 1, max_msgs, max_in_bytes,
                                          max_out_bytes, max_delay_us, ctypes.byref(h)), "bpmd_batcher_create")
        self._h = h
        self._lock = threading.Lock()
        self._pending = {}
        self._next = 1
        self._cb = _DONE(self._done)

    def _done(self, user, status, n):
        with self._lock:
            c = self._pending.pop(user)
        c.status, c.length = int(status), int(n)
        c.event.set()

    def submit(self, data: bytes, out_cap: int) -> Completion:
        data = bytes(data)
        c = Completion(out_cap)
        with self._lock:
            key = self._next
            self._next += 1
            self._pending[key] = c
        src = ctypes.create_string_buffer(data, max(len(data), 1))
        r = self.L.bpmd_batcher_submit(self._h, src, len(data), c.buf, out_cap, self._cb, ctypes.c_void_p(key))
        if r:
            with self._lock:
                self._pending.pop(key, None)
            _check(r, "bpmd_batcher_submit")
        return c

    def flush(self):
        _check(self.L.bpmd_batcher_flush(self._h), "bpmd_batcher_flush")

    def close(self):
        if self._h:
            self.L.bpmd_batcher_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TakeoverDeflater:
    """Send side of context-takeover connections: Beast's deflater keeps its
    window across messages unless no_context_takeover was negotiated
    (impl_base.hpp:156-166).  Each connection's plaintext accumulates in a
    device buffer; message k is placed right after the connection's earlier
    plaintext, whose last 4 KiB its matches may reach into.  Payloads decode
    with any inflater that keeps its window (TakeoverInflater, Beast's)."""

    HIST = 4096

    def __init__(self, n_conn: int, level: int = 6, window_bits: int = 15, mem_level: int = 4,
                 max_msg: int = 1 << 16, device="cuda"):
        self.cfg = _Cfg(level, window_bits, mem_level, 0, 0)
        self.max_msg = max_msg
        self.slot = (2 * self.HIST + max_msg + 15) // 16 * 16
        self.buf = torch.zeros(n_conn * self.slot + 16, dtype=torch.uint8, device=device)
        self.base = torch.arange(n_conn, dtype=torch.int64, device=device) * self.slot
        self.pos = torch.zeros(n_conn, dtype=torch.int64, device=device)

    def deflate(self, src: Batch, conn=None, stream=None) -> Result:
        L = lib()
        dev = self.buf.device
        n = src.n
        conn = torch.arange(n, device=dev) if conn is None else torch.as_tensor(conn, device=dev).long()
        _check_unique(conn, n)
        lens = src.len.to(torch.int64)
        if n and int(lens.max().item()) > self.max_msg:
            raise BpmdError("message exceeds max_msg")
        full = self.pos[conn] + lens > self.slot
        if n and bool(full.any()):
            idx = conn[full]
            keep = torch.minimum(self.pos[idx], torch.tensor(self.HIST, device=dev))
            p32, k32, b64 = self.pos[idx].to(torch.int32), keep.to(torch.int32), self.base[idx].contiguous()
            _check(L.bpmd_slide_batch(_ptr(self.buf), _ptr(b64), _ptr(p32), _ptr(k32), int(idx.numel()),
                                      _stream_handle(stream)), "bpmd_slide_batch")
            self.pos[idx] = keep
        pos = self.pos[conn]
        in_off = (self.base[conn] + pos).contiguous()
        total = int(lens.sum().item()) if n else 0
        if total:   # place the messages after each connection's plaintext
            start = torch.cumsum(lens, 0) - lens
            j = torch.arange(total, device=dev) - torch.repeat_interleave(start, lens)
            self.buf[torch.repeat_interleave(in_off, lens) + j] = src.data[torch.repeat_interleave(src.off, lens) + j]
        hist = torch.minimum(pos, torch.tensor(self.HIST, device=dev)).to(torch.int32)
        cap = (lens + (lens + 7) // 8 + (lens + 63) // 64 + 11).to(torch.int32)
        out_off = slot_offsets(cap)
        out = torch.empty(int(out_off[-1].item() + cap[-1].item()) + 16 if n else 16, dtype=torch.uint8,
                          device=dev)
        out_len = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        in_len = src.len.to(torch.int32).contiguous()
        _check(L.bpmd_deflate_takeover_batch(ctypes.byref(self.cfg), _ptr(self.buf), _ptr(in_off), _ptr(in_len),
                                             _ptr(hist), n, _ptr(out), _ptr(out_off), _ptr(cap), _ptr(out_len),
                                             _ptr(status), _stream_handle(stream)), "bpmd_deflate_takeover_batch")
        self.pos[conn] = pos + lens
        return Result(Batch(out, out_off, out_len), cap, status)


# ------------------------------------------------- one process, several GPUs

class _Shard(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("stream", ctypes.c_void_p), ("d_in", ctypes.c_void_p),
                ("d_in_off", ctypes.c_void_p), ("d_in_len", ctypes.c_void_p), ("n_msgs", ctypes.c_uint32),
                ("d_out", ctypes.c_void_p), ("d_out_off", ctypes.c_void_p), ("d_out_cap", ctypes.c_void_p),
                ("d_out_len", ctypes.c_void_p), ("d_status", ctypes.c_void_p)]


def shard_ranges(lens, n_parts: int):
    """bpmd_shard_ranges: [(start, end)] byte-balanced contiguous ranges."""
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    starts = np.zeros(n_parts + 1, dtype=np.uint32)
    _check(lib().bpmd_shard_ranges(lens.ctypes.data_as(ctypes.c_void_p), len(lens), n_parts,
                                   starts.ctypes.data_as(ctypes.c_void_p)), "bpmd_shard_ranges")
    return [(int(starts[i]), int(starts[i + 1])) for i in range(n_parts)]


def _multi(fn, cfg, parts):
    """parts: [(src Batch, out buffer, out_off, cap, out_len, status, stream)]."""
    arr = (_Shard * len(parts))()
    for i, (src, out, out_off, cap, out_len, status, stream) in enumerate(parts):
        arr[i] = _Shard(src.data.device.index or 0, _stream_handle(stream), _ptr(src.data), _ptr(src.off),
                        _ptr(src.len), src.n, _ptr(out), _ptr(out_off), _ptr(cap), _ptr(out_len), _ptr(status))
    totals = np.zeros(len(parts), dtype=np.uint64)
    _check(fn(ctypes.byref(cfg), arr, len(parts), totals.ctypes.data_as(ctypes.c_void_p)), fn.__name__)
    return totals


def inflate_batch_multi(srcs, out_caps, window_bits: int = 15, streams=None):
    """bpmd_inflate_batch_multi over shards (each a Batch on its own device):
    returns ([Result], per-shard output byte totals)."""
    streams = streams or [None] * len(srcs)
    parts, res = [], []
    for src, c, st in zip(srcs, out_caps, streams):
        dev = src.data.device
        cap = torch.full((src.n,), c, dtype=torch.int32, device=dev) if isinstance(c, int) else c.to(dev)
        off = slot_offsets(cap)
        out = torch.empty((int(off[-1].item() + cap[-1].item()) if src.n else 0) + 16, dtype=torch.uint8, device=dev)
        out_len = torch.empty(src.n, dtype=torch.int32, device=dev)
        status = torch.empty(src.n, dtype=torch.int32, device=dev)
        parts.append((src, out, off, cap, out_len, status, st))
        res.append(Result(Batch(out, off, out_len), cap, status))
    totals = _multi(lib().bpmd_inflate_batch_multi, _Cfg(0, window_bits, 8, 0, 0), parts)
    return res, totals


def deflate_batch_multi(srcs, level: int = 6, window_bits: int = 15, mem_level: int = 4, strategy: int = 0,
                        streams=None):
    """bpmd_deflate_batch_multi over shards; slots of deflate_upper_bound."""
    streams = streams or [None] * len(srcs)
    parts, res = [], []
    for src, st in zip(srcs, streams):
        dev = src.data.device
        l64 = src.len.to(torch.int64)
        cap = (l64 + (l64 + 7) // 8 + (l64 + 63) // 64 + 11).to(torch.int32)
        off = slot_offsets(cap)
        out = torch.empty((int(off[-1].item() + cap[-1].item()) if src.n else 0) + 16, dtype=torch.uint8, device=dev)
        out_len = torch.empty(src.n, dtype=torch.int32, device=dev)
        status = torch.empty(src.n, dtype=torch.int32, device=dev)
        parts.append((src, out, off, cap, out_len, status, st))
        res.append(Result(Batch(out, off, out_len), cap, status))
    totals = _multi(lib().bpmd_deflate_batch_multi, _Cfg(level, window_bits, mem_level, strategy, 0), parts)
    return res, totals


# ------------------------------------------------------------------------
# Send side: messages -> decision -> deflate -> frames -> packed wire
# (bpmd_send_batch, bpmd_control_batch)

CTL_WIRE = 144   # bytes of a control frame's wire slot


def _send_lib():
    """lib() with the send side's prototypes, bound on first use so that a
    BPMD_LIB variant built without them still serves every other call"""
    L = lib()
    if not getattr(L, "_send_ready", False):
        vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        L.bpmd_send_frame_bound.argtypes = [u64, u32, ci, ci]
        L.bpmd_send_frame_bound.restype = u64
        L.bpmd_send_wire_bound.argtypes = [u64, u32, ci, ci, ci]
        L.bpmd_send_wire_bound.restype = u64
        L.bpmd_send_batch.argtypes = ([ctypes.POINTER(_Cfg), vp, vp, vp, u32, ci, ci, u64, ci, u32] + [vp] * 9 + [u64]
                                      + [vp] * 6)
        L.bpmd_send_batch.restype = ci
        L.bpmd_control_batch.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
        L.bpmd_control_batch.restype = ci
        L.bpmd_internal_send_frames.argtypes = ([vp, vp, vp, u32, ci, ci, ci, u32] + [vp] * 7 + [u64] + [vp] * 6)
        L.bpmd_internal_send_frames.restype = ci
        L._send_ready = True
    return L


def send_frame_bound(n: int, frame_max: int = 4096, may_compress: bool = True, frag: bool = True) -> int:
    """bpmd_send_frame_bound: the most frames (keys, in client role) a message
    of n input bytes can take, whatever the decision and the deflater give."""
    return _send_lib().bpmd_send_frame_bound(n, frame_max, int(may_compress), int(frag))


def send_wire_bound(n: int, frame_max: int = 4096, masked: bool = False, may_compress: bool = True,
                    frag: bool = True) -> int:
    """bpmd_send_wire_bound: the most wire bytes of a message of n input bytes."""
    return _send_lib().bpmd_send_wire_bound(n, frame_max, int(masked), int(may_compress), int(frag))


def send_bounds(lens: torch.Tensor, frame_max: int = 4096, masked: bool = False, may_compress=True, frag: bool = True):
    """(frame bound, wire bound) per message as int64 tensors on the lengths'
    device: bpmd_send_frame_bound / bpmd_send_wire_bound without a host loop.
    may_compress: one value, or a tensor with one per message."""
    lens = lens.to(torch.int64)
    mk = 4 if masked else 0
    hdr = lambda x: torch.where(x <= 125, 2, torch.where(x <= 65535, 4, 10)) + mk  # noqa: E731

    def plan(ln, multi):
        if multi:
            frames = torch.clamp((ln + frame_max - 1) // frame_max, min=1)
            unit = torch.where(ln > 0, torch.full_like(ln, frame_max), ln)
        else:
            frames, unit = torch.ones_like(ln), ln
        last = ln - (frames - 1) * unit
        return frames, (frames - 1) * (hdr(unit) + unit) + hdr(last) + last

    pf, pw = plan(lens, frag)
    zf, zw = plan(lens + (lens + 7) // 8 + (lens + 63) // 64 + 11, True)
    if isinstance(may_compress, torch.Tensor):
        mc = may_compress.to(device=lens.device) != 0
    else:
        mc = torch.full_like(lens, bool(may_compress), dtype=torch.bool)
    return torch.where(mc, torch.maximum(pf, zf), pf), torch.where(mc, torch.maximum(pw, zw), pw)


@dataclass
class Sent:
    wire: Batch                # packed wire: off = exclusive sum of the sizes, len = size (0 = not written)
    status: torch.Tensor       # int32: 0, WS_BAD_OPCODE, need_buffers or WS_BUFFER_OVERFLOW
    compressed: torch.Tensor   # uint8: begin_msg's decision
    total: torch.Tensor        # int64 [1]: the sum of all sizes, written or not
    deflated: Result | None    # the staging slots (deflate_batch's result over the compressed messages)
    key_base: torch.Tensor | None   # int32: message i's first key index (client role)


def send_batch(src: Batch, role: int, pmd_on: bool = True, threshold: int = 0, frag: bool = True,
               frame_max: int = 4096, op=None, opt=None, keys=None, key_base: torch.Tensor | None = None,
               level: int = 6, window_bits: int = 15, mem_level: int = 4, strategy: int = 0, exact: bool = False,
               staging: Result | None = None, wire: torch.Tensor | None = None, wire_cap: int | None = None,
               stream=None) -> Sent:
    """bpmd_send_batch: decide (begin_msg), deflate and frame every message of
    `src` into one packed wire buffer, as write_some sends a message
    (write.hpp:625-831); `role` is the sending end's (ROLE_CLIENT masks).
    `op`: 1 text / 2 binary, per message or one value (None = binary); `opt`:
    wr_compress_opt per message (None = on).  In client role frame f of
    message i takes keys[key_base[i] + f]; without `key_base` the bases are
    the exclusive sum of send_bounds' frame bounds and `keys` must hold at
    least their sum.

    Everything is enqueued on `stream`.  The call itself waits only to size
    what it allocates: pass `staging` (a Result with the slots, e.g. an earlier
    call's `deflated`), `key_base` and `wire` to avoid every wait.  `wire_cap`
    defaults to the bytes of `wire`."""
    L = _send_lib()
    dev = src.data.device
    n = src.n
    masked = role == ROLE_CLIENT
    with _on(stream):
        opt_t = _u8(opt, n, dev)
        op_t = _u8(op, n, dev)
        may = (opt_t != 0) if (pmd_on and opt_t is not None) else bool(pmd_on)
        fb = wb = None
        if (masked and key_base is None) or wire is None:
            fb, wb = send_bounds(src.len, frame_max, masked, may, frag)
        kt = None
        if masked:
            if keys is None:
                raise BpmdError("send_batch: client role needs keys")
            nk = int(keys.numel()) if isinstance(keys, torch.Tensor) else len(keys)
            kt = _keys(keys, nk, dev)
            if key_base is None:
                if kt.numel() < (int(fb.sum().item()) if n else 0):
                    raise BpmdError("send_batch: keys must hold one key per frame of the bound (send_bounds)")
                key_base = (torch.cumsum(fb, 0) - fb).to(torch.int32)
        if pmd_on and staging is None:
            ln = src.len.to(torch.int64)
            cap = (ln + (ln + 7) // 8 + (ln + 63) // 64 + 11).to(torch.int32)
            z_off = slot_offsets(cap)
            z = torch.empty((int(z_off[-1].item() + cap[-1].item()) if n else 0) + 16, dtype=torch.uint8, device=dev)
            staging = Result(Batch(z, z_off, torch.zeros(n, dtype=torch.int32, device=dev)), cap,
                             torch.zeros(n, dtype=torch.int32, device=dev))
        if wire is None:
            wire = torch.empty((int(wb.sum().item()) if n else 0) + 16, dtype=torch.uint8, device=dev)
            if wire_cap is None:
                wire_cap = wire.numel() - 16
        if wire_cap is None:
            wire_cap = wire.numel()
        if wire_cap > wire.numel():
            raise BpmdError("send_batch: wire_cap exceeds the wire buffer")
        w_off = torch.zeros(n, dtype=torch.int64, device=dev)
        w_len = torch.zeros(n, dtype=torch.int32, device=dev)
        comp = torch.zeros(n, dtype=torch.uint8, device=dev)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
    cfg = _Cfg(level, window_bits, mem_level, strategy, F_EXACT if exact else 0)
    zs = staging
    _check(L.bpmd_send_batch(ctypes.byref(cfg), _ptr(src.data), _ptr(src.off), _ptr(src.len), n, role,
                             1 if pmd_on else 0, threshold, 1 if frag else 0, frame_max, _optr(op_t), _optr(opt_t),
                             _optr(zs.out.data if zs else None), _optr(zs.out.off if zs else None),
                             _optr(zs.cap if zs else None), _optr(zs.out.len if zs else None), _optr(kt),
                             _optr(key_base), _ptr(wire), wire_cap, _ptr(w_off), _ptr(w_len), _ptr(comp),
                             _ptr(status), _ptr(total), _stream_handle(stream)), "bpmd_send_batch")
    return Sent(Batch(wire, w_off, w_len), status, comp, total, staging if pmd_on else None, key_base)


def _send_tk_lib():
    """_send_lib() with bpmd_send_takeover_batch's prototype, bound on first use"""
    L = _send_lib()
    if not getattr(L, "_send_tk_ready", False):
        vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        L.bpmd_send_takeover_work_bytes.argtypes = [u32]
        L.bpmd_send_takeover_work_bytes.restype = ctypes.c_size_t
        L.bpmd_send_takeover_batch.argtypes = ([ctypes.POINTER(_Cfg), vp, vp, vp, u32, ci, u64, ci, u32, u32] + [vp] * 4
                                               + [u32] + [vp] * 8 + [u64] + [vp] * 7)
        L.bpmd_send_takeover_batch.restype = ci
        L._send_tk_ready = True
    return L


class TakeoverSender:
    """bpmd_send_takeover_batch over n_conn context-takeover connections:
    send_batch's chained call (begin_msg's decision, deflater, frames, packed
    wire) with TakeoverDeflater's buffers -- 2 * 4096 + max_msg bytes per
    connection, a compressed message placed right behind the connection's
    earlier compressed plaintext, the last 4 KiB slid to the front when a
    message would not fit -- and that bookkeeping done on the device.  An
    uncompressed message is framed straight from the caller's bytes and never
    enters the history, as the peer's inflater never sees it.  Entry i of every
    batch is connection i; op 0 marks a connection with nothing to send.  The
    sender owns the connections' buffers (`buf`, `base`, `pos`), the staging
    slots and the workspace; a Sent's tensors of one call are valid until the
    next.  `max_msg` bounds every message, compressed or not: keys (client
    role: `key_stride` per connection, frame f of connection i takes
    keys[i * key_stride + f]) and the default wire are sized from it with
    send_frame_bound / send_wire_bound.  A connection whose message came back
    with need_buffers or WS_BUFFER_OVERFLOW has not advanced: send the message
    again with more room, the others idle."""

    HIST = 4096

    def __init__(self, n_conn: int, role: int, level: int = 6, window_bits: int = 15, mem_level: int = 4,
                 max_msg: int = 1 << 16, threshold: int = 0, frag: bool = True, frame_max: int = 4096, device="cuda"):
        L = _send_tk_lib()
        self.n, self.role, self.max_msg = n_conn, role, max_msg
        self.threshold, self.frag, self.frame_max = threshold, frag, frame_max
        self.cfg = _Cfg(level, window_bits, mem_level, 0, 0)
        self.slot = (2 * self.HIST + max_msg + 15) // 16 * 16
        self.buf = torch.zeros(n_conn * self.slot + 16, dtype=torch.uint8, device=device)
        self.base = torch.arange(n_conn, dtype=torch.int64, device=device) * self.slot
        self.pos = torch.zeros(n_conn, dtype=torch.int32, device=device)
        masked = role == ROLE_CLIENT
        self.key_stride = int(L.bpmd_send_frame_bound(max_msg, frame_max, 1, int(frag)))
        self.wire_bound = int(L.bpmd_send_wire_bound(max_msg, frame_max, int(masked), 1, int(frag)))
        self.key_base = (torch.arange(n_conn, dtype=torch.int32, device=device) * self.key_stride) if masked else None
        zc = (upper_bound(max_msg) + 15) // 16 * 16
        self.z = torch.empty(n_conn * zc + 16, dtype=torch.uint8, device=device)
        self.z_off = torch.arange(n_conn, dtype=torch.int64, device=device) * zc
        self.z_cap = torch.full((n_conn,), zc, dtype=torch.int32, device=device)
        self.work = torch.empty(max(int(L.bpmd_send_takeover_work_bytes(n_conn)), 1), dtype=torch.uint8, device=device)

    def send(self, src: Batch, op, opt=None, keys=None, wire: torch.Tensor | None = None, stream=None) -> Sent:
        """One call over src (entry i: connection i's message).  `op`: 0 idle,
        1 text, 2 binary, per connection or one value; `opt`: wr_compress_opt
        per message (None = on).  Everything is enqueued on `stream`; with
        `wire` given (wire_bound bytes per connection always suffice) the call
        reads nothing back, without it the call also checks the lengths
        against max_msg."""
        L = _send_tk_lib()
        dev = self.buf.device
        n = src.n
        if n != self.n:
            raise BpmdError("TakeoverSender.send: one entry per connection")
        masked = self.role == ROLE_CLIENT
        kt = None
        if masked:
            if keys is None:
                raise BpmdError("TakeoverSender.send: client role needs keys")
            kt = _keys(keys, int(keys.numel()) if isinstance(keys, torch.Tensor) else len(keys), dev)
            if kt.numel() < n * self.key_stride:
                raise BpmdError("TakeoverSender.send: keys must hold key_stride keys per connection")
        with _on(stream):
            op_t, opt_t = _u8(op, n, dev), _u8(opt, n, dev)
            if wire is None:
                if n and int(src.len.max().item()) > self.max_msg:
                    raise BpmdError("message exceeds max_msg")
                wire = torch.empty(n * self.wire_bound + 16, dtype=torch.uint8, device=dev)
            z_len = torch.zeros(n, dtype=torch.int32, device=dev)
            w_off = torch.zeros(n, dtype=torch.int64, device=dev)
            w_len = torch.zeros(n, dtype=torch.int32, device=dev)
            comp = torch.zeros(n, dtype=torch.uint8, device=dev)
            status = torch.zeros(n, dtype=torch.int32, device=dev)
            total = torch.zeros(1, dtype=torch.int64, device=dev)
        _check(L.bpmd_send_takeover_batch(
            ctypes.byref(self.cfg), _ptr(src.data), _ptr(src.off), _ptr(src.len), n, self.role, self.threshold,
            1 if self.frag else 0, self.frame_max, self.max_msg, _optr(op_t), _optr(opt_t), _ptr(self.buf),
            _ptr(self.base), self.slot, _ptr(self.pos), _ptr(self.z), _ptr(self.z_off), _ptr(self.z_cap), _ptr(z_len),
            _optr(kt), _optr(self.key_base), _ptr(wire), wire.numel(), _ptr(w_off), _ptr(w_len), _ptr(comp),
            _ptr(status), _ptr(total), _ptr(self.work), _stream_handle(stream)), "bpmd_send_takeover_batch")
        return Sent(Batch(wire, w_off, w_len), status, comp, total,
                    Result(Batch(self.z, self.z_off, z_len), self.z_cap, status), self.key_base)


WR_STATE_BYTES = 4   # sizeof(bpmd_wr_state)


def wr_state(n: int, device="cuda") -> torch.Tensor:
    """n zeroed bpmd_wr_state records (uint8 [n, 4]: wr_cont, wr_compress,
    wr_op, reserved): no message open on any connection."""
    return torch.zeros((n, WR_STATE_BYTES), dtype=torch.uint8, device=device)


def _send_pc_lib():
    """_send_tk_lib() with bpmd_send_pieces_batch's prototypes, bound on first use"""
    L = _send_tk_lib()
    if not getattr(L, "_send_pc_ready", False):
        vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        L.bpmd_send_piece_frame_bound.argtypes = [u64, u32, ci, ci, ci]
        L.bpmd_send_piece_frame_bound.restype = u64
        L.bpmd_send_piece_wire_bound.argtypes = [u64, u32, ci, ci, ci, ci]
        L.bpmd_send_piece_wire_bound.restype = u64
        L.bpmd_send_pieces_work_bytes.argtypes = [u32]
        L.bpmd_send_pieces_work_bytes.restype = ctypes.c_size_t
        L.bpmd_send_pieces_batch.argtypes = ([ctypes.POINTER(_Cfg), vp, vp, vp, u32, ci, u64, ci, u32, u32] + [vp] * 7
                                             + [u32] + [vp] * 8 + [u64] + [vp] * 7)
        L.bpmd_send_pieces_batch.restype = ci
        L._send_pc_ready = True
    return L


def send_piece_bounds(n: int, frame_max: int = 4096, masked: bool = False, may_compress: bool = True,
                      frag: bool = True, fin: bool = False):
    """(bpmd_send_piece_frame_bound, bpmd_send_piece_wire_bound): the most
    frames (keys, in client role) and wire bytes one piece of n input bytes can
    take; a non-final piece (`fin` false) counts its 00 00 FF FF."""
    L = _send_pc_lib()
    return (int(L.bpmd_send_piece_frame_bound(n, frame_max, int(may_compress), int(frag), int(fin))),
            int(L.bpmd_send_piece_wire_bound(n, frame_max, int(masked), int(may_compress), int(frag), int(fin))))


class PieceSender:
    """bpmd_send_pieces_batch over n_conn connections: TakeoverSender for
    messages that arrive in pieces, as an application calls Beast's
    write_some(fin, buffers).  Entry i of every call is connection i's next
    piece (op 0: nothing to send); the first piece of a message decides
    whether the message is compressed, from its own length, and carries the
    opcode; `fin` marks a message's last piece.  `state` (wr_state) and `pos`
    stay on the device, so connections at any point of their messages share a
    call.  `no_takeover`: per connection (or one value), whether
    no_context_takeover was negotiated -- its history is reset after every
    compressed message -- None = none.  `max_piece` bounds a piece, not a
    message: keys (client role: `key_stride` per connection, frame f of
    connection i's piece takes keys[i * key_stride + f]) and the default wire
    (`wire_bound` bytes per connection) are sized from it with
    send_piece_bounds.  A connection whose piece came back with a non-zero
    status has not moved: send the piece again (a shorter one after
    WS_MESSAGE_TOO_BIG), the others idle.  A Sent's tensors of one call are
    valid until the next."""

    HIST = 4096

    def __init__(self, n_conn: int, role: int, level: int = 6, window_bits: int = 15, mem_level: int = 4,
                 max_piece: int = 1 << 16, threshold: int = 0, frag: bool = True, frame_max: int = 4096,
                 no_takeover=None, device="cuda"):
        L = _send_pc_lib()
        self.n, self.role, self.max_piece = n_conn, role, max_piece
        self.threshold, self.frag, self.frame_max = threshold, frag, frame_max
        self.cfg = _Cfg(level, window_bits, mem_level, 0, 0)
        self.slot = (2 * self.HIST + max_piece + 15) // 16 * 16
        self.buf = torch.zeros(n_conn * self.slot + 16, dtype=torch.uint8, device=device)
        self.base = torch.arange(n_conn, dtype=torch.int64, device=device) * self.slot
        self.pos = torch.zeros(n_conn, dtype=torch.int32, device=device)
        self.state = wr_state(n_conn, device)
        self.no_takeover = _u8(no_takeover, n_conn, device)
        masked = role == ROLE_CLIENT
        self.key_stride, self.wire_bound = send_piece_bounds(max_piece, frame_max, masked, True, frag, False)
        self.key_base = (torch.arange(n_conn, dtype=torch.int32, device=device) * self.key_stride) if masked else None
        zc = (upper_bound(max_piece) + 4 + 15) // 16 * 16
        self.z = torch.empty(n_conn * zc + 16, dtype=torch.uint8, device=device)
        self.z_off = torch.arange(n_conn, dtype=torch.int64, device=device) * zc
        self.z_cap = torch.full((n_conn,), zc, dtype=torch.int32, device=device)
        self.work = torch.empty(max(int(L.bpmd_send_pieces_work_bytes(n_conn)), 1), dtype=torch.uint8, device=device)

    def send(self, src: Batch, op, fin, opt=None, keys=None, wire: torch.Tensor | None = None, stream=None) -> Sent:
        """One call over src (entry i: connection i's piece).  `op`: 0 idle,
        1 text, 2 binary, per connection or one value (a continuation piece's
        only has to be 1 or 2); `fin`: the piece is its message's last, per
        connection or one value (None = all); `opt`: wr_compress_opt, looked at
        on a message's first piece (None = on).  Everything is enqueued on
        `stream`; with `wire` given the call reads nothing back, without it
        the call also checks the lengths against max_piece."""
        L = _send_pc_lib()
        dev = self.buf.device
        n = src.n
        if n != self.n:
            raise BpmdError("PieceSender.send: one entry per connection")
        masked = self.role == ROLE_CLIENT
        kt = None
        if masked:
            if keys is None:
                raise BpmdError("PieceSender.send: client role needs keys")
            kt = _keys(keys, int(keys.numel()) if isinstance(keys, torch.Tensor) else len(keys), dev)
            if kt.numel() < n * self.key_stride:
                raise BpmdError("PieceSender.send: keys must hold key_stride keys per connection")
        with _on(stream):
            op_t, opt_t, fin_t = _u8(op, n, dev), _u8(opt, n, dev), _u8(fin, n, dev)
            if wire is None:
                if n and int(src.len.max().item()) > self.max_piece:
                    raise BpmdError("piece exceeds max_piece")
                wire = torch.empty(n * self.wire_bound + 16, dtype=torch.uint8, device=dev)
            z_len = torch.zeros(n, dtype=torch.int32, device=dev)
            w_off = torch.zeros(n, dtype=torch.int64, device=dev)
            w_len = torch.zeros(n, dtype=torch.int32, device=dev)
            comp = torch.zeros(n, dtype=torch.uint8, device=dev)
            status = torch.zeros(n, dtype=torch.int32, device=dev)
            total = torch.zeros(1, dtype=torch.int64, device=dev)
        _check(L.bpmd_send_pieces_batch(
            ctypes.byref(self.cfg), _ptr(src.data), _ptr(src.off), _ptr(src.len), n, self.role, self.threshold,
            1 if self.frag else 0, self.frame_max, self.max_piece, _optr(op_t), _optr(opt_t), _optr(fin_t),
            _optr(self.no_takeover), _ptr(self.state), _ptr(self.buf), _ptr(self.base), self.slot, _ptr(self.pos),
            _ptr(self.z), _ptr(self.z_off), _ptr(self.z_cap), _ptr(z_len), _optr(kt), _optr(self.key_base), _ptr(wire),
            wire.numel(), _ptr(w_off), _ptr(w_len), _ptr(comp), _ptr(status), _ptr(total), _ptr(self.work),
            _stream_handle(stream)), "bpmd_send_pieces_batch")
        return Sent(Batch(wire, w_off, w_len), status, comp, total,
                    Result(Batch(self.z, self.z_off, z_len), self.z_cap, status), self.key_base)


RD_PIECE_STATE_BYTES = 32   # sizeof(bpmd_rd_piece_state)


def rd_piece_state(n: int, device="cuda") -> torch.Tensor:
    """n zeroed bpmd_rd_piece_state records (uint8 [n, 32]: rd_size and
    rd_remain little-endian in bytes 0-7 and 8-15, rd_key in 16-19, then
    rd_cont, rd_op, rd_deflated, rd_fin, utf8_n, utf8_b[3]): every connection
    between messages."""
    return torch.zeros((n, RD_PIECE_STATE_BYTES), dtype=torch.uint8, device=device)


def _recv_pc_lib():
    """lib() with bpmd_receive_pieces_batch's prototypes, bound on first use"""
    L = lib()
    if not getattr(L, "_recv_pc_ready", False):
        vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        L.bpmd_receive_pieces_zstate_bytes.argtypes = []
        L.bpmd_receive_pieces_zstate_bytes.restype = ctypes.c_size_t
        L.bpmd_receive_pieces_work_bytes.argtypes = [u32]
        L.bpmd_receive_pieces_work_bytes.restype = ctypes.c_size_t
        L.bpmd_receive_pieces_batch.argtypes = [ctypes.POINTER(_Cfg), ci, ci, ctypes.c_uint64, vp, vp, vp, u32] + \
            [vp] * 20
        L.bpmd_receive_pieces_batch.restype = ci
        L._recv_pc_ready = True
    return L


@dataclass
class RecvPieces(Recv):
    """A Recv whose entries are pieces: frames.out.len is the gathered length
    of this call's piece, msg.len the bytes delivered, and EV_MESSAGE marks a
    message's last piece."""

    def to_host(self):
        """Per entry the bytes this call delivered (from the slot
        frames.compressed names), b"" when there are none."""
        comp, ln = self.frames.compressed.cpu().tolist(), self.msg.len.cpu().tolist()
        # each buffer and offset array crosses to the host once
        host = [(b.data.cpu().numpy(), b.off.cpu().tolist()) for b in (self.frames.out, self.msg)]
        out = []
        for i, k in enumerate(ln):
            data, off = host[1 if comp[i] else 0]
            out.append(data[off[i]:off[i] + k].tobytes())
        return out


class PieceReceiver:
    """bpmd_receive_pieces_batch over n_conn connections: PieceSender's
    counterpart, Beast's read_some with its state on the device.  Entry i of
    every call is connection i's unconsumed wire bytes (length 0: idle); a call
    delivers one piece per connection -- what has arrived of the current
    message, inflated by the connection's own state machine, checked as UTF-8
    with the cut code point carried -- and EV_MESSAGE marks a message's last.
    The caller drops `consumed` bytes of each connection and calls again with
    the rest (after EV_NEED_MORE with nothing consumed: once more has come).
    The receiver owns `state` (rd_piece_state), the inflater states `zstate`
    and the workspace; slots are sized per call, and a RecvPieces' tensors are
    valid until the next call.  A connection that reported an error is dropped
    by the caller: its states are unspecified."""

    def __init__(self, n_conn: int, role: int, window_bits: int = 15, pmd_on: bool = True, msg_max: int = 16 << 20,
                 device="cuda"):
        L = _recv_pc_lib()
        self.n, self.role, self.wbits, self.pmd_on, self.msg_max = n_conn, role, window_bits, pmd_on, msg_max
        self.state = rd_piece_state(n_conn, device)
        self.zstate = self.work = None
        if pmd_on:
            self.zstate = torch.zeros(max(n_conn * int(L.bpmd_receive_pieces_zstate_bytes()), 16), dtype=torch.uint8,
                                      device=device)
            self.work = torch.empty(max(int(L.bpmd_receive_pieces_work_bytes(n_conn)), 1), dtype=torch.uint8,
                                    device=device)

    def recv(self, wire: Batch, out_cap, msg_cap, stream=None, out: torch.Tensor | None = None,
             out_off: torch.Tensor | None = None, msg: torch.Tensor | None = None,
             msg_off: torch.Tensor | None = None) -> RecvPieces:
        """One call over wire.  `out_cap` (>= 8): bytes of every gathered slot,
        of which a call fills at most out_cap - 4; `msg_cap`: the room of every
        inflated piece.  Each is one int, or an int32 tensor with the caller's
        buffer and offsets (`out` must stay readable for 15 bytes past every
        slot).  Everything is enqueued on `stream`; the call never waits."""
        L = _recv_pc_lib()
        dev = self.state.device
        n = wire.n
        if n != self.n:
            raise BpmdError("PieceReceiver.recv: one entry per connection")
        if isinstance(out_cap, int) and out_cap < 8:
            raise BpmdError("PieceReceiver.recv: out_cap below 8")
        with _on(stream):
            cap, out, out_off = _host_slots("out", n, dev, out_cap, out, out_off)
            out_len = torch.empty(n, dtype=torch.int32, device=dev)
            u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)  # noqa: E731
            op, comp, event, ctl_len, ctl = u8(n), u8(n), u8(n), u8(n), u8(n, CTL_SLOT)
            status = torch.empty(n, dtype=torch.int32, device=dev)
            consumed = torch.empty(n, dtype=torch.int32, device=dev)
            code = torch.empty(n, dtype=torch.int16, device=dev)
            msg_len = torch.empty(n, dtype=torch.int32, device=dev)
            mcap = None
            if self.pmd_on:
                mcap, msg, msg_off = _host_slots("msg", n, dev, msg_cap, msg, msg_off)
            else:
                msg, msg_off = u8(0), torch.zeros(n, dtype=torch.int64, device=dev)
        on = self.pmd_on
        cfg = _Cfg(0, self.wbits, 8, 0, 0)
        _check(L.bpmd_receive_pieces_batch(
            ctypes.byref(cfg) if on else None, self.role, 1 if on else 0, self.msg_max, _ptr(wire.data),
            _ptr(wire.off), _ptr(wire.len), n, _ptr(self.state), _optr(self.zstate), _ptr(out), _ptr(out_off),
            _ptr(cap), _ptr(out_len), _ptr(op), _ptr(comp), _ptr(event), _ptr(status), _ptr(consumed), _ptr(ctl),
            _ptr(ctl_len), _ptr(code), _ptr(msg) if on else None, _ptr(msg_off) if on else None, _optr(mcap),
            _ptr(msg_len), _optr(self.work), _stream_handle(stream)), "bpmd_receive_pieces_batch")
        with _on(stream):
            code = code.to(torch.int32) & 0xFFFF
        frames = Unframed(Batch(out, out_off, out_len), cap, op, comp, event, status, consumed, ctl, ctl_len, code,
                          self.state)
        return RecvPieces(frames, Batch(msg, msg_off, msg_len), event, status)


@dataclass
class Controls:
    wire: Batch            # one frame per entry at 144 * i; len 0 = refused
    status: torch.Tensor   # int32: 0, WS_BAD_CONTROL_SIZE or WS_BAD_OPCODE


def control_batch(op, ctl: torch.Tensor, ctl_len, close_code=None, key=None, wire: torch.Tensor | None = None,
                  stream=None) -> Controls:
    """bpmd_control_batch: ping (9), pong (10) and close (8) frames as
    write_ping / write_close build them (stream_impl.hpp:915-996).  `ctl`
    (uint8 [n, 128]) and `ctl_len` are unframe_batch's control slots, so a
    received ping's slot goes back out as a pong unchanged; a close with a
    non-zero `close_code` carries the code and then the slot as its reason.
    `key` (client role): one masking key per entry; `wire`: the caller's
    buffer of 144 bytes per entry."""
    L = _send_lib()
    dev = ctl.device
    n = int(ctl.numel()) // CTL_SLOT
    if ctl.dtype != torch.uint8 or ctl.numel() != n * CTL_SLOT or not ctl.is_contiguous():
        raise BpmdError("control_batch: ctl must be uint8 [n, 128]")
    with _on(stream):
        op_t = _u8(op, n, dev)
        len_t = _u8(ctl_len, n, dev)
        if close_code is None:
            code = torch.zeros(n, dtype=torch.int16, device=dev)
        elif isinstance(close_code, torch.Tensor):
            code = close_code.to(device=dev, dtype=torch.int16).contiguous()
        else:
            a = np.array(np.broadcast_to(np.asarray(close_code, dtype=np.int64) & 0xFFFF, (n,)), dtype=np.uint16)
            code = torch.from_numpy(a.view(np.int16)).to(dev)
        k = _keys(key, n, dev)
        if wire is None:
            wire = torch.empty(n * CTL_WIRE + 16, dtype=torch.uint8, device=dev)
        elif wire.dtype != torch.uint8 or wire.numel() < n * CTL_WIRE or not wire.is_contiguous():
            raise BpmdError("control_batch: wire must hold 144 bytes per entry")
        w_len = torch.zeros(n, dtype=torch.int32, device=dev)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        w_off = torch.arange(n, dtype=torch.int64, device=dev) * CTL_WIRE
    _check(L.bpmd_control_batch(_ptr(op_t), _ptr(ctl), _ptr(len_t), _ptr(code), _optr(k), n, _ptr(wire), _ptr(w_len),
                                _ptr(status), _stream_handle(stream)), "bpmd_control_batch")
    return Controls(Batch(wire, w_off, w_len), status)
