"""The receive side's header step (beast_amd/csrc/frame_parse.h) on the CPU:
the header compiles with plain g++ into a shim, and the shim is compared with
the Python restatement of parse_fh / read_close (tests/frame_parse_model.py)
on the known answers of tests/golden/frame_parse_kat.json and on generated
headers; the model itself is checked against the oracle's framer by round
trip.  tests/cpp/frame_parse_main.cpp fuzzes the same header under the address
and undefined-behaviour sanitizers, on buffers of exactly `avail` bytes."""
import ctypes
import json
import os
import random
import subprocess

import pytest

from oracle import oracle as O
from tests import frame_parse_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beast_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
KAT = os.path.join(ROOT, "tests", "golden", "frame_parse_kat.json")
EVENTS = {"need_more": M.EV_NEED_MORE, "message": M.EV_MESSAGE, "ping": M.EV_PING, "pong": M.EV_PONG,
          "close": M.EV_CLOSE}

SHIM = r"""
#include <string.h>
#include "frame_parse.h"
using namespace bpmd::fp;
extern "C" int32_t fp_parse(const uint8_t* p, uint64_t avail, uint32_t role, int pmd_on, uint64_t msg_max,
                            uint64_t out_room, const uint8_t* st16, uint64_t* o)
{
    RdState st;
    memcpy(&st, st16, 16);
    Header h;
    memset(&h, 0, sizeof h);
    const int32_t r = parse_fh(p, avail, role, pmd_on != 0, msg_max, out_room, st, h);
    const uint64_t v[7] = {h.hdr_len, h.len, h.fin, h.rsv1, h.op, h.masked, h.key};
    for (int i = 0; i < 7; ++i) o[i] = v[i];
    return r;
}
extern "C" int fp_close_code_valid(uint32_t v) { return close_code_valid((uint16_t)v); }
extern "C" int32_t fp_read_close(const uint8_t* p, uint32_t n, uint32_t* code)
{
    uint16_t c = 0;
    const int32_t r = read_close([&](uint32_t i) { return (uint32_t)p[i]; }, n, c);
    *code = c;
    return r;
}
extern "C" void fp_walk(const uint8_t* p, uint32_t wl, uint32_t role, int pmd_on, uint64_t msg_max, uint32_t cap,
                        uint8_t* st16, uint8_t* out, uint8_t* ctl, uint64_t* o)
{
    RdState st;
    memcpy(&st, st16, 16);
    Stop s;
    walk(
        p, wl, role, pmd_on != 0, msg_max, cap, st,
        [&](uint64_t at, const uint8_t* src, uint32_t len, uint32_t key) {
            for (uint32_t i = 0; i < len; ++i) out[at + i] = src[i] ^ (uint8_t)(key >> (8 * (i & 3)));
        },
        [&](const uint8_t* src, uint32_t len, uint32_t key) {
            for (uint32_t i = 0; i < len; ++i) ctl[i] = src[i] ^ (uint8_t)(key >> (8 * (i & 3)));
        },
        s);
    memcpy(st16, &st, 16);
    const uint64_t v[8] = {s.event, (uint64_t)s.status, s.consumed, s.msg_len, s.msg_op, s.msg_deflated, s.ctl_len,
                           s.close_code};
    for (int i = 0; i < 8; ++i) o[i] = v[i];
}
extern "C" unsigned fp_state_size() { return sizeof(RdState); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_parse")
    src, lib = d / "shim.cpp", d / "libfp.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC, str(src),
                    "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    u64, u32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p
    L.fp_parse.argtypes = [vp, u64, u32, ctypes.c_int, u64, u64, vp, vp]
    L.fp_parse.restype = ctypes.c_int32
    L.fp_read_close.argtypes = [vp, u32, vp]
    L.fp_read_close.restype = ctypes.c_int32
    L.fp_walk.argtypes = [vp, u32, u32, ctypes.c_int, u64, u32, vp, vp, vp, vp]
    L.fp_walk.restype = None
    assert L.fp_state_size() == 16
    return L


def c_parse(L, b, role, pmd_on, msg_max, out_room, st):
    buf = (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")
    o = (ctypes.c_uint64 * 7)()
    r = L.fp_parse(buf, len(b), role, int(pmd_on), msg_max, out_room, st.pack(), o)
    if r != M.FRAME:
        return r, None
    return r, M.Header(o[0], o[1], bool(o[2]), bool(o[3]), o[4], bool(o[5]), o[6])


def c_walk(L, b, role, pmd_on, msg_max, cap, state16, out):
    """fp_walk on one entry; state16 / out (bytearrays) are updated in place"""
    buf = (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")
    st = (ctypes.c_uint8 * 16).from_buffer(state16)
    ob = (ctypes.c_uint8 * max(len(out), 1)).from_buffer_copy(bytes(out) or b"\0")
    ctl = (ctypes.c_uint8 * 128)()
    o = (ctypes.c_uint64 * 8)()
    L.fp_walk(buf, len(b), role, int(pmd_on), msg_max, cap, st, ob, ctl, o)
    out[:] = bytes(ob)[:len(out)]
    status = o[1] if o[1] < (1 << 31) else o[1] - (1 << 64)
    return M.Stop(o[0], status, o[2], o[3], o[4], o[5], bytes(ctl)[:o[6]], o[7], bytes(state16))


def load_kats():
    with open(KAT) as f:
        return json.load(f)["cases"]


def run_kat(case, walk_fn):
    """[Stop per call] of one known-answer case through walk_fn(bytes, state, out) -> Stop"""
    rest, stops = b"", []
    state, out = case_state(), bytearray(case.get("out_cap", 4096))
    for part in case["parts"]:
        buf = rest + bytes.fromhex(part)
        s = walk_fn(buf, state, out)
        rest = buf[s.consumed:]
        stops.append(s)
    return stops


def case_state():
    return {"model": M.State(), "c": bytearray(16)}


def test_kats_model_and_shim(shim):
    cases = load_kats()
    assert len(cases) >= 40
    chopped = [c for c in cases if c["name"] == "chopped frame header"][0]
    assert chopped["parts"] == ["817e01", "01" + "2a" * 257]
    for c in cases:
        role, pmd_on = c["role"], c["pmd_on"]
        msg_max, cap = c.get("msg_max", 16 << 20), c.get("out_cap", 4096)
        mo = run_kat(c, lambda b, st, out: M.walk(b, role, pmd_on, msg_max, cap, st["model"], out))
        co = run_kat(c, lambda b, st, out: c_walk(shim, b, role, pmd_on, msg_max, cap, st["c"], out))
        assert len(mo) == len(c["expect"])
        for k, e in enumerate(c["expect"]):
            want = (EVENTS[e["event"]], 0 if e["status"] == "ok" else M.ERR[e["status"]], e["consumed"])
            assert (mo[k].event, mo[k].status, mo[k].consumed) == want, (c["name"], k, "model")
            assert co[k] == mo[k], (c["name"], k, "shim")
            for f in ("close_code", "compressed", "op"):
                if f in e:
                    assert getattr(mo[k], f) == e[f], (c["name"], k, f)


def test_close_codes_every_value(shim):
    for v in range(65536):
        assert bool(shim.fp_close_code_valid(v)) == M.close_code_valid(v), v


def test_read_close_matches_model(shim):
    rng = random.Random(3)
    reasons = [b"", b"bye", "é".encode(), "語".encode()[:2], b"\xff", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"a" * 123,
               ("\U0001f600" * 30).encode(), ("\U0001f600" * 31).encode()[:123]]
    reasons += [rng.randbytes(rng.randrange(1, 124)) for _ in range(300)]
    for code in (0, 999, 1000, 1005, 1015, 2999, 3000, 4999, 65535):
        for r in reasons:
            p = code.to_bytes(2, "big") + r
            for q in (p, p[:1], b""):
                buf = (ctypes.c_uint8 * max(len(q), 1)).from_buffer_copy(q or b"\0")
                got_code = ctypes.c_uint32()
                st = shim.fp_read_close(buf, len(q), ctypes.byref(got_code))
                assert (st, got_code.value) == M.read_close(q), q.hex()


LENS = [(7, 0), (7, 1), (7, 125), (16, 0), (16, 125), (16, 126), (16, 65535), (64, 0), (64, 65535), (64, 65536),
        (64, 70001), (64, (1 << 63) - 1), (64, 1 << 63), (64, (1 << 64) - 1)]


def header(b0, form, n, key):
    m = 0x80 if key is not None else 0
    b = bytes([b0]) + (bytes([m | n]) if form == 7 else bytes([m | 126]) + n.to_bytes(2, "big") if form == 16
                       else bytes([m | 127]) + n.to_bytes(8, "big"))
    return b + (key.to_bytes(4, "little") if key is not None else b"")


def states(rng):
    yield M.State()
    yield M.State(rng.choice([0, 1, 100, 4000, (1 << 64) - 100]), True, rng.choice([1, 2]), rng.random() < 0.5)


def test_headers_match_model(shim):
    """Every opcode x FIN x RSV combination x length form at its boundaries x
    masked or not, under both roles, pmd on and off, a message in progress or
    not, and every avail from 0 to header + 2; then mutated headers."""
    rng = random.Random(11)
    n = 0
    kinds = set()
    for b0 in range(256):
        for form, ln in LENS:
            for masked in (False, True):
                h = header(b0, form, ln, rng.getrandbits(32) if masked else None) + rng.randbytes(2)
                role, pmd_on = rng.randrange(2), rng.random() < 0.5
                msg_max = rng.choice([0, 100, 16 << 20, 1 << 62])
                room = rng.choice([0, 125, 4096, 1 << 20, (1 << 32) - 1])
                for k, st in enumerate(states(rng)):
                    for avail in (range(len(h) + 1) if k == 0 else (len(h), rng.randrange(len(h) + 1))):
                        got = c_parse(shim, h[:avail], role, pmd_on, msg_max, room, st)
                        assert got == M.parse_fh(h[:avail], role, pmd_on, msg_max, room, st), \
                            (h.hex(), avail, role, pmd_on, msg_max, room, st)
                        kinds.add(got[0])
                        n += 1
    # the role each header wants, so the later checks are reached as well
    for _ in range(6000):
        form, ln = rng.choice(LENS)
        masked = rng.random() < 0.5
        h = bytearray(header(rng.choice([0x00, 0x01, 0x02, 0x80, 0x81, 0x82, 0xC1, 0x41, 0x88, 0x89, 0x8A]), form, ln,
                             rng.getrandbits(32) if masked else None))
        if rng.random() < 0.5:
            h[rng.randrange(len(h))] = rng.randrange(256)
        role, pmd_on = (0 if h[1] & 0x80 else 1), rng.random() < 0.5
        msg_max, room = rng.choice([0, 100, 70000, 16 << 20]), rng.choice([0, 125, 4096, 70001, (1 << 32) - 1])
        for st in states(rng):
            for avail in (len(h), rng.randrange(len(h) + 1)):
                got = c_parse(shim, bytes(h[:avail]), role, pmd_on, msg_max, room, st)
                assert got == M.parse_fh(bytes(h[:avail]), role, pmd_on, msg_max, room, st), (h.hex(), avail, st)
                kinds.add(got[0])
                n += 1
    assert n >= 20000
    assert kinds >= {M.NEED_MORE, M.FRAME} | {M.ERR[e] for e in (
        "buffer_overflow", "message_too_big", "bad_opcode", "bad_data_frame", "bad_continuation", "bad_reserved_bits",
        "bad_control_fragment", "bad_control_size", "bad_unmasked_frame", "bad_masked_frame", "bad_size")}


def test_model_round_trips_the_oracle_framer(shim):
    """O.frame_write's frames, walked by the model and by the shim, give back
    the payload, opcode and RSV1 and consume every byte."""
    rng = random.Random(12)
    for ln in (0, 1, 5, 125, 126, 127, 300, 4096, 65535, 65536, 70001):
        for frame_max in (1, 5, 125, 126, 4096, 65536):
            if frame_max == 1 and ln > 300:
                continue
            payload, op, rsv1 = rng.randbytes(ln), rng.choice([1, 2]), rng.random() < 0.5
            for masked in (False, True):
                nf = max(1, -(-ln // frame_max))
                keys = [rng.getrandbits(32) for _ in range(nf)] if masked else None
                wire = O.frame_write(payload, op, rsv1, keys=keys, frame_max=frame_max)
                role = M.SERVER if masked else M.CLIENT
                out = bytearray(ln)
                s = M.walk(wire, role, True, 0, ln, M.State(), out)
                assert (s.event, s.status, s.consumed, s.out_len, s.op, s.compressed) == \
                    (M.EV_MESSAGE, 0, len(wire), ln, op, int(rsv1)), (ln, frame_max, masked)
                assert bytes(out) == payload and s.state == bytes(16)
                out2, st2 = bytearray(ln), bytearray(16)
                assert c_walk(shim, wire, role, True, 0, ln, st2, out2) == s
                assert bytes(out2) == payload


def test_entry_point_validates_before_device_use():
    """bpmd_unframe_batch: a bad role and a NULL required pointer are refused,
    n == 0 is a no-op; none of it touches a device."""
    from beast_amd import pmd
    L = pmd.lib()
    nulls = [None] * 14
    assert L.bpmd_unframe_batch(2, 1, 0, None, None, None, 0, *nulls) == -1
    assert L.bpmd_unframe_batch(-1, 1, 0, None, None, None, 1, *nulls) == -1
    for role in (pmd.ROLE_SERVER, pmd.ROLE_CLIENT):
        assert L.bpmd_unframe_batch(role, 1, 0, None, None, None, 0, *nulls) == 0
        assert L.bpmd_unframe_batch(role, 1, 0, None, None, None, 1, *nulls) == -1
    assert set(pmd.WS_ERRORS) == set(M.ERR_NAME) and all(pmd.WS_ERRORS[k] == M.ERR_NAME[k] for k in M.ERR_NAME)
    assert pmd.WS_BAD_CLOSE_PAYLOAD == M.ERR["bad_close_payload"] and pmd.WS_BUFFER_OVERFLOW == M.ERR["buffer_overflow"]


def test_sanitized_fuzz_of_the_header_step():
    """tests/cpp/frame_parse_main.cpp under -fsanitize=address,undefined: the
    header step and the walk on heap buffers of exactly `avail` bytes."""
    build = os.path.join(CPP, "_build")
    os.makedirs(build, exist_ok=True)
    src, out = os.path.join(CPP, "frame_parse_main.cpp"), os.path.join(build, "frame_parse_main")
    hdr = os.path.join(CSRC, "frame_parse.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
