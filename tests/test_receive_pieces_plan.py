"""The rules of the chained receive in pieces
(beast_amd/csrc/receive_pieces_plan.h) on the CPU: the header compiles with
plain g++ into a shim (tests/cpp/receive_pieces_plan_shim.cpp) and is compared
with the Python model (tests/receive_pieces_model.py) -- the walk over random
connections cut at random and at every byte, the key rotation, the room, the
status rule exhaustively over small values, and the UTF-8 carry against the
oracle's streaming utf8_checker at every split.  The model itself is checked
against the oracle's whole-message inflate, and
tests/cpp/receive_pieces_plan_main.cpp runs the header under the address and
undefined-behaviour sanitizers."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

from oracle import oracle as O
from tests import frame_parse_model as FM
from tests import receive_pieces_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beast_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
U32, U64 = (1 << 32) - 1, (1 << 64) - 1


class WalkOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in ("piece_len", "consumed", "event")] + [("status", ctypes.c_int32)] + \
        [(k, ctypes.c_uint32) for k in ("msg_op", "msg_deflated", "tail", "ctl_len", "close_code")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("receive_pieces_plan")
    lib = d / "librpp.so"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC,
                    os.path.join(CPP, "receive_pieces_plan_shim.cpp"), "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    u64, u32, i32, ci, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p
    L.rpp_state_bytes.restype = u32
    L.rpp_rot_key.argtypes, L.rpp_rot_key.restype = [u32, u64], u32
    L.rpp_walk.argtypes, L.rpp_walk.restype = [vp, u32, u32, ci, u64, u32, vp, vp, vp, vp], None
    L.rpp_inflates.argtypes, L.rpp_inflates.restype = [u32, u32, u32], ci
    L.rpp_limit_room.argtypes, L.rpp_limit_room.restype = [u32, u64, u64], u32
    L.rpp_merge.argtypes, L.rpp_merge.restype = [i32, u64, u64, u64, u64, u64], i32
    L.rpp_utf8_head.argtypes, L.rpp_utf8_head.restype = [u32, vp, vp, u32, vp], None
    L.rpp_utf8_tail.argtypes, L.rpp_utf8_tail.restype = [vp, u32, vp], None
    L.rpp_commit.argtypes, L.rpp_commit.restype = [vp, ci, u64, u32, vp], None
    return L


def c_walk(L, b, role, pmd_on, msg_max, cap, state: bytes):
    """(WalkOut, state after, out slot, control slot) of the header's walk"""
    wire = ctypes.create_string_buffer(bytes(b), max(len(b), 1))
    st = ctypes.create_string_buffer(state, 32)
    out = ctypes.create_string_buffer(b"\xA5" * max(cap, 1), max(cap, 1))
    ctl = ctypes.create_string_buffer(b"\xA5" * 128, 128)
    w = WalkOut()
    L.rpp_walk(wire, len(b), role, int(pmd_on), msg_max, cap, st, out, ctl, ctypes.byref(w))
    return w, st.raw, out.raw[:cap], ctl.raw


def test_state_is_32_bytes_and_zero_between_messages(shim):
    from beast_amd import pmd
    assert shim.rpp_state_bytes() == 32 == pmd.RD_PIECE_STATE_BYTES == len(M.ZERO)
    assert M.ZERO == bytes(32)
    assert pmd.rd_piece_state(3, device="cpu").tolist() == [[0] * 32] * 3


def test_key_rotation(shim):
    """byte 0 of the rotated key is the byte the next payload byte takes"""
    rng = random.Random(1)
    for key in [0, 0x01020304, 0xFFFFFFFF] + [rng.getrandbits(32) for _ in range(20)]:
        for n in list(range(9)) + [U32, U32 + 1, U64]:
            r = shim.rpp_rot_key(key, n)
            assert r == M.rot_key(key, n)
            data = bytes(range(1, 9))
            assert O.mask(data, r) == O.mask(bytes(n & 3) + data, key)[n & 3:]


def _connection(rng, masked, errors=True):
    """one connection's wire: fragmented messages with control frames between
    the fragments, every length form that fits, sometimes an error at the end"""
    w = b""
    key = (lambda: rng.getrandbits(32)) if masked else (lambda: None)
    for _ in range(rng.randint(1, 4)):
        op, rsv = rng.choice([1, 2]), rng.choice([0, 4])
        frags = rng.randint(1, 4)
        for f in range(frags):
            n = rng.choice([0, 1, 2, 5, 17, 64, 125, 126, 300])
            w += FM.frame(rng.randbytes(n), op if f == 0 else 0, f + 1 == frags, rsv if f == 0 else 0, key(),
                          len_form=rng.choice([None, None, 16]) if n >= 126 else None)
            if f + 1 < frags and rng.random() < 0.3:
                w += FM.frame(rng.randbytes(rng.randint(0, 125)), rng.choice([9, 10]), True, 0, key())
    kind = rng.randint(0, 5) if errors else 0
    if kind == 0:
        w += FM.frame(b"\x03\xe9" + b"going", 8, True, 0, key())
    elif kind == 1:
        w += FM.frame(b"xy", 1, True, 2, key())                       # reserved bits
    elif kind == 2:
        w += FM.frame(b"xy", 0, True, 0, key())                       # continuation of nothing
    elif kind == 3:
        w += FM.frame(b"x" * 300, 2, True, 0, key())                  # over a small msg_max
    elif kind == 4:
        w += FM.frame(b"x", 2, False, 0, key()) + FM.frame(b"y", 1, True, 0, key())   # data frame inside a message
    else:
        w += FM.frame(b"\x03", 8, True, 0, key())                     # close of one byte
    return w


def _compare_connection(L, w, role, pmd_on, msg_max, cap, feed):
    """the header's walk and the model's, call by call, on one connection fed
    feed() more bytes whenever a call took nothing"""
    st = M.PState()
    raw = M.ZERO
    fed = used = 0
    events = 0
    while True:
        b = w[used:fed]
        pre = raw
        got, raw, out, ctl = c_walk(L, b, role, pmd_on, msg_max, cap, raw)
        s = M.walk(b, role, pmd_on, msg_max, cap, st)
        tag = (used, fed, cap, role, pmd_on, msg_max)
        assert (got.event, got.status, got.consumed, got.piece_len, got.tail, got.msg_op, got.msg_deflated) == \
            (s.event, s.status, s.consumed, len(s.piece), int(s.tail), s.op, s.compressed), tag
        assert got.ctl_len == len(s.ctl) and ctl[:got.ctl_len] == s.ctl and ctl[got.ctl_len:] == b"\xA5" * (128 - got.ctl_len)
        assert got.close_code == s.close_code
        want = s.piece + (M.TAIL if s.tail else b"")
        assert out == want + b"\xA5" * (cap - len(want)), tag
        assert len(s.piece) <= max(cap - 4, 0)
        assert raw == st.pack(), tag
        if s.consumed == 0:
            assert raw == pre
        used += s.consumed
        if s.status:
            return events
        last = s.event == FM.EV_MESSAGE
        events += s.event != FM.EV_NEED_MORE
        # the finish step's commit, with nothing delivered and no carry
        buf = ctypes.create_string_buffer(raw, 32)
        L.rpp_commit(buf, int(last), 0, 0, bytes(3))
        raw = buf.raw
        if last:
            st = M.PState()
        assert raw == st.pack()
        if s.consumed == 0 and s.event == FM.EV_NEED_MORE:
            if fed == len(w):
                return events
            fed = min(len(w), fed + feed())


def test_walk_matches_model_on_random_connections(shim):
    rng = random.Random(7)
    total = 0
    for k in range(300):
        role = k & 1
        w = _connection(rng, masked=role == FM.SERVER)
        pmd_on = rng.random() < 0.8
        msg_max = rng.choice([0, 0, 200, 1000])
        cap = rng.choice([8, 9, 12, 16, 100, 4096])
        step = rng.choice([1, 2, 3, 7, 50, 10000])
        total += _compare_connection(shim, w, role, pmd_on, msg_max, cap, lambda: rng.randint(1, step))
    assert total > 600


def test_walk_matches_model_at_every_cut(shim):
    """one connection, the bytes arriving in two parts cut at every byte, and a byte at a time"""
    rng = random.Random(11)
    for role in (FM.SERVER, FM.CLIENT):
        w = _connection(rng, masked=role == FM.SERVER, errors=False)
        for cut in range(1, len(w)):
            parts = iter([cut, len(w)])
            assert _compare_connection(shim, w, role, True, 0, 64, lambda: next(parts)) >= 2
        assert _compare_connection(shim, w, role, True, 0, 12, lambda: 1) >= 2


def test_small_slots_gather_nothing(shim):
    w = FM.frame(b"hello", 2, True)
    for cap in range(8):
        got, raw, out, _ = c_walk(shim, w, FM.CLIENT, True, 0, cap, M.ZERO)
        assert (got.status, got.consumed, got.piece_len, got.event) == (M.BUFFER_OVERFLOW, 0, 0, 0)
        assert raw == M.ZERO and out == b"\xA5" * cap
        assert M.walk(w, FM.CLIENT, True, 0, cap, M.PState()).status == M.BUFFER_OVERFLOW


def test_room_and_status_rules(shim):
    vals = [0, 1, 2, 99, 100, 101, U32 - 1, U32, U32 + 1, U64 - 1, U64]
    for cap, mx, size in itertools.product([0, 1, 100, 101, U32], vals, vals):
        if mx and size > mx:
            continue            # a message over its limit has been refused already
        assert shim.rpp_limit_room(cap, mx, size) == M.limit_room(cap, mx, size), (cap, mx, size)
    small = [0, 1, 2, 3, 10]
    for ec, iu, ni, ou, size, mx in itertools.product([0, 1, 2, 13], small, small, small, small, small):
        if iu > ni:
            continue
        assert shim.rpp_merge(ec, iu, ni, ou, size, mx) == M.merge(ec, iu, ni, ou, size, mx), (ec, iu, ni, ou, size, mx)
    assert shim.rpp_merge(0, 5, 5, 1, U64, 0) == 0 and shim.rpp_merge(0, 5, 5, 2, U64 - 1, U64) == M.MESSAGE_TOO_BIG
    for d, n, t in itertools.product([0, 1], [0, 1, 9], [0, 1]):
        assert bool(shim.rpp_inflates(d, n, t)) == bool(d and (n or t))


def _device_utf8(L, carry: bytes, piece: bytes, last: bool):
    """the finish step's check, the wave's scan stood in for by check_utf8 over
    the same bytes: (fails, new carry)"""
    r = ctypes.create_string_buffer(6)
    L.rpp_utf8_head(len(carry), carry.ljust(3, b"\0"), piece, len(piece), r)
    bad, skip, n, b = r.raw[0], r.raw[1], r.raw[2], r.raw[3:6]
    rest = piece[skip:]
    err = bool(bad)
    if not err:
        err = O.utf8_check(rest) == 2 or (rest[:1] != b"" and rest[0] & 0xC0 == 0x80)
    if not err and n == 0:
        L.rpp_utf8_tail(rest, len(rest), r)
        n, b = r.raw[2], r.raw[3:6]
    return err or (last and n != 0), b[:n]


TEXTS = ["aé€😀z".encode(), "߿ࠀ￿\U00010000\U0010ffff".encode(), b"\xe0\x80x", b"ab\xf4\x90\x80\x80",
         b"\x80abc", b"a\xc0\xafb", b"\xed\xa0\x80", b"\xf0\x9f\x98", b"\xc3", b"ok\xe2\x82", b"\xf5\x80\x80\x80",
         b"plain ascii text of some length", b"\xf0\x90\x80\x80\xf4\x8f\xbf\xbf", b"a\xe2\x28\xa1"]


def test_utf8_carry_matches_the_streaming_checker(shim):
    """every text split into up to three pieces at every position: verdict by
    verdict and carry by carry Beast's utf8_checker"""
    for t in TEXTS:
        for i, j in itertools.combinations_with_replacement(range(len(t) + 1), 2):
            pieces = [t[:i], t[i:j], t[j:]]
            u, carry = O.Utf8Checker(), b""
            for k, p in enumerate(pieces):
                last = k == 2
                if not p and not last:
                    continue
                ok = u.write(p) and (not last or u.finish())
                fails, carry = _device_utf8(shim, carry, p, last)
                assert fails == (not ok), (t, i, j, k)
                if fails:
                    break
                if not last:
                    assert carry == (bytes(u._s.cp[:u._s.have]) if u._s.need else b""), (t, i, j, k)


def _pieces_of(conn, w, cap, msg_cap, step):
    """feed w to the model step bytes at a time; [(kind, bytes or status)]"""
    fed = used = 0
    out, cur = [], b""
    while True:
        p = conn.call(w[used:fed], cap, msg_cap)
        used += p.stop.consumed
        cur += p.delivered
        if p.status:
            out.append(("error", p.status))
            return out
        if p.stop.event == FM.EV_MESSAGE:
            out.append(("message", cur))
            cur = b""
        elif p.stop.event != FM.EV_NEED_MORE:
            out.append(("control", p.stop.ctl))
        elif p.stop.consumed == 0:
            if fed == len(w):
                return out
            fed = min(len(w), fed + step)


def test_model_delivers_what_the_oracle_inflates():
    """the model's pieces of compressed messages with kept context, put
    together, are the messages (the oracle's own inflate of the payloads)"""
    msgs = [b"hello hello hello hello", "café €".encode() * 9, b"", bytes(range(256)) * 3, b"hello hello again"]
    pays = O.pmd_deflate_stream(msgs, 6, 15, 4)
    assert [o for _, o in O.pmd_inflate_stream(pays)] == msgs
    for step, cap in [(1, 8), (3, 12), (10000, 4096), (7, 64)]:
        w = b""
        for k, p in enumerate(pays):
            cut = len(p) // 2
            w += FM.frame(p[:cut], 2 if k != 1 else 1, False, 4, 0x11223344 + k) + \
                FM.frame(b"!", 9, True, 0, 5) + FM.frame(p[cut:], 0, True, 0, 99)
        got = _pieces_of(M.Conn(FM.SERVER), w, cap, 4096, step)
        assert [b for k, b in got if k == "message"] == msgs
        assert [k for k, _ in got] == ["control", "message"] * len(msgs)


def test_entry_points_validate_before_device_use():
    """bpmd_receive_pieces_batch: bad arguments are refused and n == 0 is a
    no-op; none of it touches a device."""
    from beast_amd import pmd
    L = pmd._recv_pc_lib()
    cfg = pmd._Cfg(0, 15, 8, 0, 0)
    NP = 22    # pointer arguments besides cfg and stream

    def recv(n=0, role=pmd.ROLE_SERVER, cfg=cfg, pmd_on=1, ptrs=None):
        p = ptrs or [None] * NP
        return L.bpmd_receive_pieces_batch(ctypes.byref(cfg) if cfg else None, role, pmd_on, 0, p[0], p[1], p[2], n,
                                           *p[3:], None)

    assert recv() == 0 and recv(role=pmd.ROLE_CLIENT) == 0 and recv(cfg=None, pmd_on=0) == 0
    assert recv(role=2) == -1 and recv(role=-1) == -1
    assert recv(cfg=None) == -1
    assert recv(cfg=pmd._Cfg(0, 15, 8, 0, pmd.F_RAW)) == -1 and recv(cfg=pmd._Cfg(0, 15, 8, 0, pmd.F_RAW), pmd_on=0) == -1
    assert recv(cfg=pmd._Cfg(0, 16, 8, 0, 0)) != 0 and recv(cfg=pmd._Cfg(0, 7, 8, 0, 0)) != 0
    assert recv(n=1) == -1                                            # NULL required pointers
    dummy = (ctypes.c_uint64 * 4)()
    some = [ctypes.cast(dummy, ctypes.c_void_p)] * NP
    # d_zstate, d_msg, d_msg_off, d_msg_cap, d_work: required with the extension only
    with_pmd = {4, 17, 18, 19, 21}
    for k in range(NP):
        p = list(some)
        p[k] = None
        assert recv(n=1, ptrs=p) == -1, k
        if k not in with_pmd:
            assert recv(n=1, ptrs=p, pmd_on=0, cfg=None) == -1, k
    p = list(some)
    p[4] = ctypes.c_void_p(ctypes.addressof(dummy) + 8)                # d_zstate not 16-byte aligned
    if (ctypes.addressof(dummy) + 8) % 16:
        assert recv(n=1, ptrs=p) == -1
    a = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for n in (0, 1, 63, 64, 65, 256, 257, 1 << 16):
        assert L.bpmd_receive_pieces_work_bytes(n) == a(64 * n) + a(32 * n)
    zb = L.bpmd_receive_pieces_zstate_bytes()
    assert zb % 16 == 0 and zb > (1 << 15)
    from tests.model import zstream_host as H
    assert zb == H.lib().zs_host_state_bytes()


def test_sanitized_run_of_the_plan():
    """tests/cpp/receive_pieces_plan_main.cpp under -fsanitize=address,undefined"""
    build = os.path.join(CPP, "_build")
    os.makedirs(build, exist_ok=True)
    src, out = os.path.join(CPP, "receive_pieces_plan_main.cpp"), os.path.join(build, "receive_pieces_plan_main")
    hdrs = [os.path.join(CSRC, h) for h in ("receive_pieces_plan.h", "frame_parse.h", "receive_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, [src] + hdrs)):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
