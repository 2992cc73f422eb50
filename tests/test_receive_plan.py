"""The receive side's plan (beast_amd/csrc/receive_plan.h) on the CPU: the
header compiles with plain g++ into a shim (tests/cpp/receive_plan_shim.cpp)
and is compared with the Python model (tests/receive_model.py) over the full
cross product of what one entry can look like after the frame pass and the
inflater.  tests/cpp/receive_plan_main.cpp runs the same header under the
address and undefined-behaviour sanitizers on heap blocks of exactly the
announced sizes."""
import ctypes
import itertools
import os
import subprocess

import pytest

from tests import frame_parse_model as FM
from tests import receive_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beast_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

EVENTS = (FM.EV_NEED_MORE, FM.EV_MESSAGE, FM.EV_PING, FM.EV_PONG, FM.EV_CLOSE)
STATUS = (0, FM.ERR["bad_reserved_bits"])
ZST = (0, 1, 6, 13)   # ok, need_buffers, invalid_stored_length, invalid_distance
CAPS = (0, 1, 2, 100, 4096, M.U32)


def msg_maxes(cap):
    return sorted({0, 1, max(cap - 1, 0), cap, cap + 1, M.U32, 1 << 32, 1 << 63})


def lengths(cap, msg_max):
    """around msg_max and around the slot, inside 32 bits"""
    s = {0, 1, cap}
    for c in (msg_max, cap):
        s |= {c - 1, c, c + 1}
    return sorted(x for x in s if 0 <= x <= M.U32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("receive_plan")
    lib = d / "librp.so"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC,
                    os.path.join(CPP, "receive_plan_shim.cpp"), "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    u64, u32, i32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p
    L.rp_effective_cap.argtypes = [u32, u64]
    L.rp_effective_cap.restype = u32
    L.rp_select.argtypes = [u32, i32, u32, u32, u32, u32, u64, vp]
    L.rp_select.restype = None
    L.rp_merge.argtypes = [u32, i32, u32, u32, u32, u32, u64, i32, u32, vp]
    L.rp_merge.restype = i32
    L.rp_constants.argtypes = [vp]
    L.rp_constants.restype = None
    return L


def test_constants(shim):
    o = (ctypes.c_uint32 * 9)()
    shim.rp_constants(o)
    assert list(o) == [FM.EV_MESSAGE, 1, M.NEED_BUFFERS, M.BAD_FRAME_PAYLOAD, M.BUFFER_OVERFLOW, M.MESSAGE_TOO_BIG,
                       M.SRC_NONE, M.SRC_GATHERED, M.SRC_INFLATED]


def test_effective_capacity_at_the_integer_edges(shim):
    for cap in CAPS + (M.U32 - 1,):
        for mm in msg_maxes(cap) + [M.U32 - 1, M.U32 - 2, (1 << 64) - 1]:
            want = M.effective_cap(cap, mm)
            assert 0 <= want <= cap and (mm == 0 or want <= mm + 1)
            assert shim.rp_effective_cap(cap, mm) == want, (cap, mm)


def test_select_matches_model(shim):
    o = (ctypes.c_uint32 * 3)()
    n = 0
    for cap in CAPS:
        for mm in msg_maxes(cap):
            for ev, st, comp, op in itertools.product(EVENTS, STATUS, (0, 1), (1, 2)):
                for out_len in lengths(cap, mm):
                    shim.rp_select(ev, st, comp, op, out_len, cap, mm, o)
                    want = M.select(ev, st, comp, op, out_len, cap, mm)
                    assert tuple(o) == want, (ev, st, comp, op, out_len, cap, mm)
                    if not (ev == FM.EV_MESSAGE and st == 0 and comp):
                        assert want == (0, 0, 0)
                    n += 1
    assert n >= 6 * 5 * 40 * 4


def test_merge_matches_model(shim):
    o = (ctypes.c_uint32 * 2)()
    n, seen = 0, set()
    for cap in CAPS:
        for mm in msg_maxes(cap):
            lens = lengths(cap, mm)
            for ev, st, comp, op, zst in itertools.product(EVENTS, STATUS, (0, 1), (1, 2), ZST):
                for ln in lens:
                    # ln stands for the gathered length and, independently shifted, the inflated one
                    for z_len in (ln, lens[(lens.index(ln) + 1) % len(lens)]):
                        got = shim.rp_merge(ev, st, comp, op, ln, cap, mm, zst, z_len, o)
                        want = M.merge(ev, st, comp, op, ln, cap, mm, zst, z_len)
                        assert (got, o[0], o[1]) == want, (ev, st, comp, op, ln, cap, mm, zst, z_len)
                        seen.add(got)
                        n += 1
    assert n >= 50000
    assert seen == {0, 6, 13, STATUS[1], M.BUFFER_OVERFLOW, M.MESSAGE_TOO_BIG}


def test_merge_rule_spelled_out(shim):
    """the rule of include/beast_pmd.h on hand-picked entries: (msg_cap,
    msg_max, zst, z_len) -> status of a complete compressed binary message"""
    o = (ctypes.c_uint32 * 2)()
    cases = [
        ((100, 0, 0, 100), 0),
        ((100, 0, 1, 100), M.BUFFER_OVERFLOW),         # no limit: the slot was too small
        ((100, 100, 1, 100), M.MESSAGE_TOO_BIG),       # the slot is the limit: over the slot is over the limit
        ((100, 101, 1, 100), M.BUFFER_OVERFLOW),       # the slot is smaller than the limit
        ((100, 99, 0, 100), M.MESSAGE_TOO_BIG),        # produced msg_max + 1 bytes and fitted
        ((100, 99, 0, 99), 0),
        ((100, 50, 1, 51), M.MESSAGE_TOO_BIG),
        ((100, 50, 6, 51), 6),                         # a zlib error is kept whatever the length
        ((100, 50, 13, 10), 13),
        ((M.U32, 1 << 32, 1, M.U32), M.BUFFER_OVERFLOW),
        ((M.U32, M.U32, 1, M.U32), M.MESSAGE_TOO_BIG),
        ((M.U32, 1 << 63, 0, M.U32), 0),
    ]
    for (cap, mm, zst, z_len), want in cases:
        assert shim.rp_merge(FM.EV_MESSAGE, 0, 1, 2, 7, cap, mm, zst, z_len, o) == want, (cap, mm, zst, z_len)
        assert M.merge(FM.EV_MESSAGE, 0, 1, 2, 7, cap, mm, zst, z_len)[0] == want
        assert (o[0], o[1]) == (M.SRC_NONE, z_len)
    # text: the check reads the slot that holds the message, and only after status 0
    assert shim.rp_merge(FM.EV_MESSAGE, 0, 1, 1, 7, 100, 0, 0, 40, o) == 0 and tuple(o) == (M.SRC_INFLATED, 40)
    assert shim.rp_merge(FM.EV_MESSAGE, 0, 0, 1, 7, 100, 0, 0, 40, o) == 0 and tuple(o) == (M.SRC_GATHERED, 7)
    assert shim.rp_merge(FM.EV_MESSAGE, 0, 1, 1, 7, 100, 0, 6, 40, o) == 6 and tuple(o) == (M.SRC_NONE, 40)
    assert shim.rp_merge(FM.EV_PING, 0, 1, 1, 7, 100, 0, 0, 40, o) == 0 and tuple(o) == (M.SRC_NONE, 0)


def test_entry_points_validate_before_device_use():
    """bpmd_receive_batch: bad arguments are refused and n == 0 is a no-op;
    none of it touches a device."""
    from beast_amd import pmd
    L = pmd._recv_lib()
    cfg = pmd._Cfg(0, 15, 8, 0, 0)

    def recv(n=0, role=pmd.ROLE_SERVER, pmd_on=1, cfg=cfg, ptrs=None):
        p = ptrs or [None] * 21
        return L.bpmd_receive_batch(ctypes.byref(cfg) if cfg else None, role, pmd_on, 0, p[0], p[1], p[2], n, *p[3:],
                                    None)

    assert recv() == 0 and recv(role=pmd.ROLE_CLIENT) == 0 and recv(pmd_on=0, cfg=None) == 0
    assert recv(role=2) == -1 and recv(role=-1) == -1
    assert recv(cfg=None) == -1
    assert recv(cfg=pmd._Cfg(0, 15, 8, 0, pmd.F_RAW)) == -1
    assert recv(cfg=pmd._Cfg(0, 7, 8, 0, 0)) == -2 and recv(cfg=pmd._Cfg(0, 16, 8, 0, 0)) == -2
    assert recv(n=1) == -1 and recv(n=1, pmd_on=0, cfg=None) == -1          # NULL required pointers
    dummy = (ctypes.c_uint64 * 4)()
    some = [ctypes.cast(dummy, ctypes.c_void_p)] * 21
    for k in range(16, 21):   # pmd_on: each of d_msg, d_msg_off, d_msg_cap, d_msg_len, d_work is required
        p = list(some)
        p[k] = None
        assert recv(n=1, ptrs=p) == -1, k
    p = list(some)
    p[4] = None               # d_out, with permessage-deflate off
    assert recv(n=1, pmd_on=0, cfg=None, ptrs=p) == -1
    # three 32-bit arrays and a byte array, each from a 256-byte boundary
    for n in (0, 1, 63, 64, 65, 256, 257, 1 << 16):
        a = lambda x: (x + 255) // 256 * 256  # noqa: E731
        assert L.bpmd_receive_work_bytes(n) == 3 * a(4 * n) + a(n)


def test_sanitized_run_of_the_plan():
    """tests/cpp/receive_plan_main.cpp under -fsanitize=address,undefined"""
    build = os.path.join(CPP, "_build")
    os.makedirs(build, exist_ok=True)
    src, out = os.path.join(CPP, "receive_plan_main.cpp"), os.path.join(build, "receive_plan_main")
    hdr = os.path.join(CSRC, "receive_plan.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
