"""The connection rules of the chained takeover receive
(beast_amd/csrc/receive_takeover_plan.h) on the CPU: the header compiles with
plain g++ into a shim (tests/cpp/receive_takeover_plan_shim.cpp) and is
compared with the Python model (tests/receive_takeover_model.py) over the
cross product of positions, capacities, limits and window sizes at which a
rule changes its answer.  The model itself is checked against the oracle's
inflater kept across a connection's messages, and
tests/cpp/receive_takeover_plan_main.cpp runs the header under the address and
undefined-behaviour sanitizers on heap blocks of exactly one slot each."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import oracle as O
from tests import frame_parse_model as FM
from tests import receive_model as M
from tests import receive_takeover_model as TM
from tests import takeover_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beast_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
WBITS = (8, 9, 15)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("receive_takeover_plan")
    lib = d / "librtp.so"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC,
                    os.path.join(CPP, "receive_takeover_plan_shim.cpp"), "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    u64, u32, i32, ci, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p
    L.rtp_room.argtypes = [u32, u32, u32]
    L.rtp_room.restype = u32
    L.rtp_effective_cap.argtypes = [u32, u64, u32, u32]
    L.rtp_effective_cap.restype = u32
    L.rtp_place.argtypes = [u32, u32, u32, u32, ci, vp]
    L.rtp_place.restype = None
    L.rtp_advance.argtypes = [u32, ci, i32, u32]
    L.rtp_advance.restype = u32
    return L


def _slots(W):
    return (2 * W + 1, 2 * W + 100, 2 * W + 4096, 3 * W + 7)


def _msg_caps(slot, W):
    r = slot - 2 * W
    return sorted({0, 1, r - 1, r, r + 1, slot, M.U32})


def _msg_maxes(cap):
    return sorted({0, 1, max(cap - 1, 0), cap, cap + 1, M.U32, 1 << 32})


def _positions(slot, W, cap):
    s = {0, 1, W - 1, W, W + 1, 2 * W, 2 * W + 1, slot - cap - 1, slot - cap, slot - cap + 1, slot}
    return sorted(p for p in s if 0 <= p <= slot)


def test_room_and_capacity(shim):
    for wbits in WBITS:
        W = 1 << wbits
        for slot in _slots(W):
            for mc in _msg_caps(slot, W):
                want = TM.room(mc, slot, W)
                assert want <= mc and W + want <= slot - W
                assert shim.rtp_room(mc, slot, W) == want, (mc, slot, W)
                for mm in _msg_maxes(want):
                    assert shim.rtp_effective_cap(mc, mm, slot, W) == M.effective_cap(want, mm), (mc, mm, slot, W)


def test_place_matches_model_and_never_overlaps(shim):
    o = (ctypes.c_uint32 * 3)()
    n = slides = 0
    for wbits in WBITS:
        W = 1 << wbits
        for slot in _slots(W):
            for mc in _msg_caps(slot, W):
                cap = TM.room(mc, slot, W)
                for mm in _msg_maxes(cap):
                    eff = M.effective_cap(cap, mm)
                    for pos in _positions(slot, W, eff):
                        for z in (0, 1):
                            shim.rtp_place(pos, eff if z else 0, slot, W, z, o)
                            want = TM.place(pos, eff if z else 0, slot, W, bool(z))
                            assert tuple(o) == want, (pos, eff, slot, W, z)
                            slide, new_pos, hist = want
                            if not z:
                                assert want == (0, pos, 0)
                                continue
                            assert slide == int(pos + eff > slot)      # TakeoverInflater's rule
                            assert hist == min(new_pos, W) and new_pos + eff <= slot
                            if slide:   # a whole window moves, and source and destination lie apart
                                assert new_pos == W and pos - W >= W
                                slides += 1
                            n += 1
    assert n >= 3000 and slides >= 500, (n, slides)   # the loops ran, and met both answers


def test_advance_matches_model(shim):
    for pos in (0, 1, 511, 512, 70000):
        for z_len in (0, 1, 100, 65536):
            for z in (0, 1):
                for zst in range(0, 17):
                    want = TM.advance(pos, bool(z), zst, z_len)
                    assert want == (pos + z_len if z and zst == 0 else pos)
                    assert shim.rtp_advance(pos, z, zst, z_len) == want, (pos, z, zst, z_len)


def _through_model(pls, ops, wbits, slot, msg_cap, msg_max=0):
    """one connection's payloads, one frame each, through TM.receive call by call"""
    st, out = FM.State(), bytearray(max(map(len, pls)) + 1)
    buf, pos, res, slid = bytearray(b"\xee" * slot), 0, [], 0
    for p, op in zip(pls, ops):
        e = TM.receive(FM.frame(p, op, rsv=4), FM.CLIENT, msg_max, len(out), msg_cap, st, out, pos, buf, wbits)
        assert e.stop.event == FM.EV_MESSAGE and e.msg_off == (TM.place(pos, e.eff_cap, slot, 1 << wbits, True)[1])
        assert bytes(buf[e.msg_off:e.msg_off + e.msg_len]) == e.inflated
        pos = e.pos
        slid += e.slid
        res.append(e)
    return res, slid


@pytest.mark.parametrize("wbits", [9, 15])
def test_model_equals_the_oracle_inflater_kept_across_messages(wbits):
    """The model hands the oracle a window, not a history of calls: on real
    streams (CPython's and the oracle's deflater, kept across the messages,
    half of the later messages at least need what came before) statuses and
    bytes equal O.pmd_inflate_stream's, through slides."""
    rng = random.Random(100 + wbits)
    W = 1 << wbits
    max_msg = 700 if wbits == 9 else 9000
    slot = TC.takeover_slot(W, max_msg)
    need = total = slides = 0
    for c in range(6):
        lens = [rng.choice((0, 1, 300, max_msg // 2, max_msg, max_msg)) for _ in range(14 if wbits == 9 else 36)]
        msgs = TC.connection_messages(c, lens, wbits, seed=5)
        pls = TC.zlib_stream(msgs, 6, wbits) if c % 2 else O.pmd_deflate_stream(msgs, 6, wbits, 4)
        want = O.pmd_inflate_stream(pls, cap=max_msg, wbits=wbits)
        assert [w for w in want] == [(0, m) for m in msgs]
        need += sum(1 for p in pls[1:] if O.pmd_inflate(p, cap=max_msg, wbits=wbits)[0] != 0)
        total += len(pls) - 1
        got, slid = _through_model(pls, [2] * len(pls), wbits, slot, max_msg)
        assert [(e.status, e.inflated) for e in got] == want
        assert got[-1].pos == sum(lens) if not slid else got[-1].pos < slot
        slides += slid
    assert 2 * need >= total, (need, total)
    assert slides >= 3, slides


def test_model_reports_a_distance_past_the_window():
    """streams of a 32 KiB encoder window through a 512-byte decoder window:
    up to and including a connection's first failure the model equals the
    oracle's kept inflater, and failures occur"""
    failed = 0
    for c in range(4):
        msgs = TC.connection_messages(c, [3000] * 5, 15, seed=9)
        pls = O.pmd_deflate_stream(msgs, 6, 15, 4)
        want = O.pmd_inflate_stream(pls, cap=3000, wbits=9)
        got, _ = _through_model(pls, [2] * 5, 9, TC.takeover_slot(512, 3000), 3000)
        for e, (st, outb) in zip(got, want):
            assert (e.zst, e.inflated) == (st, outb)
            if st:
                assert e.pos == e.msg_off      # the position stays
                failed += 1
                break
    assert failed >= 2


def test_entry_points_validate_before_device_use():
    """bpmd_receive_takeover_batch: bad arguments are refused and n == 0 is a
    no-op; none of it touches a device."""
    from beast_amd import pmd
    L = pmd._recv_tk_lib()
    cfg = pmd._Cfg(0, 9, 8, 0, 0)

    def recv(n=0, role=pmd.ROLE_SERVER, cfg=cfg, slot=1025, ptrs=None):
        p = ptrs or [None] * 23
        return L.bpmd_receive_takeover_batch(ctypes.byref(cfg) if cfg else None, role, 0, p[0], p[1], p[2], n, *p[3:18],
                                             slot, *p[18:], None)

    assert recv() == 0 and recv(role=pmd.ROLE_CLIENT) == 0
    assert recv(role=2) == -1 and recv(role=-1) == -1
    assert recv(cfg=None) == -1
    assert recv(cfg=pmd._Cfg(0, 9, 8, 0, pmd.F_RAW)) == -1
    assert recv(cfg=pmd._Cfg(0, 7, 8, 0, 0)) == -2 and recv(cfg=pmd._Cfg(0, 16, 8, 0, 0)) == -2
    assert recv(slot=1024) == -1 and recv(slot=0) == -1                       # slot_bytes <= 2 * W
    assert recv(cfg=pmd._Cfg(0, 15, 8, 0, 0), slot=65536) == -1 and recv(cfg=pmd._Cfg(0, 15, 8, 0, 0), slot=65537) == 0
    assert recv(n=1) == -1                                                     # NULL required pointers
    dummy = (ctypes.c_uint64 * 4)()
    some = [ctypes.cast(dummy, ctypes.c_void_p)] * 23
    for k in list(range(0, 3)) + list(range(4, 23)):   # every pointer but d_state (index 3) is required
        p = list(some)
        p[k] = None
        assert recv(n=1, ptrs=p) == -1, k
    # bpmd_receive_batch's workspace, then a 32-bit and a 64-bit array, each from a 256-byte boundary
    for n in (0, 1, 63, 64, 65, 256, 257, 1 << 16):
        a = lambda x: (x + 255) // 256 * 256  # noqa: E731
        assert L.bpmd_receive_takeover_work_bytes(n) == pmd._recv_lib().bpmd_receive_work_bytes(n) + a(4 * n) + a(8 * n)


def test_sanitized_run_of_the_plan():
    """tests/cpp/receive_takeover_plan_main.cpp under -fsanitize=address,undefined"""
    build = os.path.join(CPP, "_build")
    os.makedirs(build, exist_ok=True)
    src, out = os.path.join(CPP, "receive_takeover_plan_main.cpp"), os.path.join(build, "receive_takeover_plan_main")
    hdrs = [os.path.join(CSRC, h) for h in ("receive_takeover_plan.h", "receive_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, [src] + hdrs)):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
