"""The connection rules of the chained takeover send
(beast_amd/csrc/send_takeover_plan.h) on the CPU: the header compiles with
plain g++ into a shim (tests/cpp/send_takeover_plan_shim.cpp) and is compared
with the Python model (tests/send_takeover_model.py) over the cross product of
positions, lengths, options and opcodes at which a rule changes its answer.
The model's payload sequences are checked against the oracle's inflater kept
across a connection's messages, with uncompressed messages in between, and
tests/cpp/send_takeover_plan_main.cpp runs the header under the address and
undefined-behaviour sanitizers on heap blocks of exactly one slot each."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import oracle as O
from tests import send_model as SM
from tests import send_takeover_model as TM
from tests import takeover_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beast_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
K = TM.K
U32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("send_takeover_plan")
    lib = d / "libstp.so"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC,
                    os.path.join(CPP, "send_takeover_plan_shim.cpp"), "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    u64, u32, i32, ci, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p
    L.stp_keep.restype = u32
    L.stp_room.argtypes, L.stp_room.restype = [u32, u32], u32
    L.stp_deflates.argtypes, L.stp_deflates.restype = [u32, ci, u64, u64], ci
    L.stp_provisional.argtypes, L.stp_provisional.restype = [u32, ci, u64, u32], i32
    L.stp_place.argtypes, L.stp_place.restype = [u32, u32, u32, ci, vp], None
    L.stp_merge.argtypes, L.stp_merge.restype = [i32, ci, i32], i32
    L.stp_advance.argtypes, L.stp_advance.restype = [u32, u32, ci, i32], u32
    L.stp_chunk_bound.argtypes, L.stp_chunk_bound.restype = [u32, u32], u64
    return L


SLOTS = (2 * K + 1, 2 * K + 100, 2 * K + 4097, 2 * K + 9008, 3 * K + 7)


def _max_lens(slot):
    r = slot - 2 * K
    return sorted({1, max(r - 1, 1), r, r + 1, slot, U32})


def _lengths(L):
    return sorted({0, 1, 4095, 4096, 4097, max(L - 1, 0), L, L + 1})


def _positions(slot, n):
    s = {0, 1, K - 1, K, K + 1, 2 * K, 2 * K + 1, slot - n - 1, slot - n, slot - n + 1, slot}
    return sorted(p for p in s if 0 <= p <= slot)


def test_keep_and_room(shim):
    from beast_amd import pmd
    assert shim.stp_keep() == K == TC.DEFLATE_HIST == pmd.TakeoverDeflater.HIST
    for slot in SLOTS + (0, 1, 2 * K):
        for ml in (0, 1, 100, slot, U32):
            want = TM.room(ml, slot)
            assert want <= ml and (slot <= 2 * K or K + want <= slot - K)
            assert shim.stp_room(ml, slot) == want, (ml, slot)


def test_plan_matches_model_and_no_slide_overlaps(shim):
    o = (ctypes.c_uint32 * 4)()
    n = slides = refused = plain = 0
    for slot in SLOTS:
        for ml in _max_lens(slot):
            L = TM.room(ml, slot)
            for ln in _lengths(L):
                for op in (0, 1, 2, 3, 8):
                    for opt in (0, 1):
                        for thr in (0, ln, ln + 1):
                            d = TM.deflates(op, opt, ln, thr)
                            assert d == (op in (1, 2) and bool(opt) and ln >= thr)
                            assert shim.stp_deflates(op, opt, ln, thr) == int(d), (op, opt, ln, thr)
                            st = TM.provisional(op, d, ln, L)
                            assert st == (SM.BAD_OPCODE if op not in (0, 1, 2) else TM.MESSAGE_TOO_BIG if d and ln > L
                                          else 0)
                            assert shim.stp_provisional(op, int(d), ln, L) == st, (op, d, ln, L)
                            enters = bool(d and st == 0)
                            refused += st != 0
                            plain += (not d) and st == 0 and op != 0
                            for pos in _positions(slot, ln):
                                want = TM.place(pos, ln, slot, K, enters)
                                shim.stp_place(pos, ln, slot, int(enters), o)
                                assert tuple(o) == want, (pos, ln, slot, enters)
                                slide, new_pos, z_len, hist = want
                                if not enters:   # the connection is left alone and the deflater gets nothing
                                    assert want == (0, pos, 0, 0)
                                else:
                                    assert slide == int(pos + ln > slot)       # TakeoverDeflater's rule
                                    assert z_len == ln and hist == min(new_pos, K) and new_pos + ln <= slot
                                    if slide:   # K whole bytes move, and source and destination lie apart
                                        assert new_pos == K and pos - K >= K
                                        slides += 1
                                for zst in (0, SM.NEED_BUFFERS):
                                    m = TM.provisional(op, d, ln, L) or (zst if enters else 0)
                                    assert shim.stp_merge(st, int(enters), zst) == m
                                    for final in (m, SM.BUFFER_OVERFLOW) if m == 0 else (m,):
                                        adv = TM.advance(new_pos, ln, enters, final)
                                        assert adv == (new_pos + ln if enters and final == 0 else new_pos)
                                        assert shim.stp_advance(new_pos, ln, int(enters), final) == adv
                                n += 1
    assert n >= 20000 and slides >= 300 and refused >= 1000 and plain >= 1000, (n, slides, refused, plain)


def test_chunk_bound_covers_every_batch(shim):
    rng = random.Random(3)
    for slot in SLOTS:
        for ml in _max_lens(slot):
            L = TM.room(ml, slot)
            for n in (1, 2, 7, 1000):
                b = TM.chunk_bound(n, L)
                assert shim.stp_chunk_bound(n, L) == b == n * -(-L // 4096)
                for lens in ([L] * n, [rng.randrange(L + 1) for _ in range(n)], [x for x in _lengths(L) if x <= L]):
                    assert sum(TM.chunk_count(x) for x in lens[:n]) <= b
    assert shim.stp_chunk_bound(U32, U32) == U32 * (1 << 20)   # 64-bit


def _connection(c, wbits, rounds, max_msg, rng):
    """One connection's (message, op, opt): a third of the messages sent
    uncompressed, and twice a text that goes out uncompressed first and
    compressed right after: a deflater that kept the former in its history
    would point into bytes the peer never saw."""
    lens = [rng.choice((0, 1, 300, max_msg // 2, max_msg, max_msg)) for _ in range(rounds)]
    msgs = TC.connection_messages(c, lens, wbits, seed=11)
    out = [(m, 1 + k % 2, 0 if rng.randrange(3) == 0 else 1) for k, m in enumerate(msgs)]
    for at, seed in ((rounds, 2 * c), (rounds // 2, 2 * c + 1)):
        twice = TC.json_message(200, 900 + seed)
        out[at:at] = [(twice, 1, 0), (twice, 1, 1)]
    return out


def _run(conn, wbits, slot, max_msg, leak):
    buf, pos, pls, want, slid = bytearray(b"\xee" * slot), 0, [], [], 0
    for m, op, opt in conn:
        e = TM.send(pos, buf, m, op, opt, 0, max_msg, slot, 1 << 20, None, level=6, wbits=wbits, leak=leak)
        assert e.status == 0 and e.compressed == opt
        if e.compressed:
            pls.append(e.payload)
            want.append(m)
            assert e.wire == SM.wire(e.payload, op, True, None, 4096, True)
        else:
            assert e.wire == SM.wire(m, op, False, None, 4096, True) and e.payload == b""
            assert leak or (e.pos == pos and not e.slid)
        pos = e.pos
        slid += e.slid
    return pls, want, slid


@pytest.mark.parametrize("wbits", [9, 15])
def test_model_payloads_inflate_to_the_compressed_messages(wbits):
    """Per connection, with uncompressed messages interleaved and through
    slides, the oracle's inflater kept across the messages decodes the
    model's payloads to the compressed messages; with the uncompressed
    messages let into the history it does not."""
    rng = random.Random(40 + wbits)
    max_msg = 3000
    slot = TC.takeover_slot(K, max_msg)
    slides = plain = wrong = 0
    for c in range(6):
        conn = _connection(c, wbits, 24, max_msg, rng)
        pls, want, slid = _run(conn, wbits, slot, max_msg, leak=False)
        got = O.pmd_inflate_stream(pls, cap=max_msg, wbits=wbits)
        assert got == [(0, m) for m in want], c
        slides += slid
        plain += len(conn) - len(pls)
        bad, _, _ = _run(conn, wbits, slot, max_msg, leak=True)
        wrong += O.pmd_inflate_stream(bad, cap=max_msg, wbits=wbits) != [(0, m) for m in want]
    assert slides >= 6 and plain >= 24, (slides, plain)
    assert wrong == 6, wrong


def test_entry_points_validate_before_device_use():
    """bpmd_send_takeover_batch: bad arguments are refused and n == 0 is a
    no-op; none of it touches a device."""
    from beast_amd import pmd
    L = pmd._send_tk_lib()
    cfg = pmd._Cfg(6, 15, 4, 0, 0)
    slot0 = 2 * K + 1

    def send(n=0, role=pmd.ROLE_SERVER, cfg=cfg, frame_max=4096, max_len=100, slot=slot0, ptrs=None):
        p = ptrs or [None] * 21
        return L.bpmd_send_takeover_batch(ctypes.byref(cfg) if cfg else None, p[0], p[1], p[2], n, role, 0, 1,
                                          frame_max, max_len, *p[3:7], slot, *p[7:15], 1 << 20, *p[15:], None)

    assert send() == 0 and send(role=pmd.ROLE_CLIENT) == 0
    assert send(frame_max=0) == -1
    assert send(role=2) == -1 and send(role=-1) == -1
    assert send(cfg=None) == -1
    assert send(cfg=pmd._Cfg(6, 15, 4, 0, pmd.F_EXACT)) == -1 and send(cfg=pmd._Cfg(6, 15, 4, 0, pmd.F_RAW)) == -1
    assert send(cfg=pmd._Cfg(10, 15, 4, 0, 0)) == -1 and send(cfg=pmd._Cfg(6, 16, 4, 0, 0)) == -1   # bpmd_deflate_batch's
    assert send(slot=2 * K) == -1 and send(slot=0) == -1 and send(slot=slot0) == 0
    assert send(max_len=0) == -1
    # chunk_bound = n * ceil(L / 4096) must fit 32 bits
    big = 2 * K + (1 << 24)
    assert send(n=1 << 20, max_len=U32, slot=big) == -1               # 2^20 * 2^12 chunks
    assert send(n=(1 << 20) - 1, max_len=U32, slot=big) == -1         # in range, so on to the NULL pointers
    assert send(n=1) == -1                                            # NULL required pointers
    dummy = (ctypes.c_uint64 * 4)()
    some = [ctypes.cast(dummy, ctypes.c_void_p)] * 21
    optional = {3, 4, 12, 13}   # d_op, d_opt, and in server role d_keys, d_key_base
    for k in range(21):
        if k in optional:
            continue
        p = list(some)
        p[k] = None
        assert send(n=1, ptrs=p) == -1, k
    for k in (12, 13):          # client role without keys
        p = list(some)
        p[k] = None
        assert send(n=1, role=pmd.ROLE_CLIENT, ptrs=p) == -1, k
    a = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for n in (0, 1, 63, 64, 65, 256, 257, 1 << 16):
        assert L.bpmd_send_takeover_work_bytes(n) == 3 * a(4 * n) + a(8 * n)


def test_sanitized_run_of_the_plan():
    """tests/cpp/send_takeover_plan_main.cpp under -fsanitize=address,undefined"""
    build = os.path.join(CPP, "_build")
    os.makedirs(build, exist_ok=True)
    src, out = os.path.join(CPP, "send_takeover_plan_main.cpp"), os.path.join(build, "send_takeover_plan_main")
    hdrs = [os.path.join(CSRC, h) for h in ("send_takeover_plan.h", "send_plan.h", "lz_core.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, [src] + hdrs)):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
