"""The send side's plan (beast_amd/csrc/send_plan.h) on the CPU: the header
compiles with plain g++ into a shim (tests/cpp/send_plan_shim.cpp) and is
compared with the Python model (tests/send_model.py), which stands on the
oracle's framer; the model's control writer is pinned by RFC 6455 5.7's
examples and by the receive side's model parsing every frame back.
tests/cpp/send_plan_main.cpp runs the same header under the address and
undefined-behaviour sanitizers on heap blocks of exactly the announced sizes."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import oracle as O
from tests import frame_parse_model as FM
from tests import send_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beast_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

FRAME_MAX = (1, 2, 125, 126, 127, 4096, 65535, 65536, 70000)


def lengths(frame_max):
    """0-130, 65530-65540 and around every multiple of frame_max up to there"""
    s = set(range(0, 131)) | set(range(65530, 65541))
    top = 65540
    mults = range(frame_max, top + frame_max + 1, frame_max)
    if len(mults) > 40:   # small frame sizes: the first, some in the middle, the last
        mults = list(mults[:6]) + list(mults[len(mults) // 2:len(mults) // 2 + 3]) + list(mults[-3:])
    for m in mults:
        s |= {m - 1, m, m + 1}
    return sorted(s)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("send_plan")
    lib = d / "libsp.so"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC,
                    os.path.join(CPP, "send_plan_shim.cpp"), "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    u64, u32, vp, ci = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int
    L.sp_compress.argtypes = [ci, ci, u64, u64]
    L.sp_deflate_bound.argtypes = [u64]
    L.sp_deflate_bound.restype = u64
    L.sp_split.argtypes = [u64, u32, ci, ci, vp]
    L.sp_split.restype = None
    L.sp_wire_size.argtypes = [u64, u32, ci, ci, ci]
    L.sp_wire_size.restype = u64
    L.sp_frame.argtypes = [u64, u32, ci, ci, ci, u64, vp]
    L.sp_frame.restype = None
    L.sp_header.argtypes = [u64, ci, ci, ci, u32, ci, u32, vp]
    L.sp_header.restype = u32
    L.sp_message.argtypes = [vp, u64, u32, ci, vp, u32, ci, vp]
    L.sp_message.restype = u64
    L.sp_frame_bound.argtypes = [u64, u32, ci, ci]
    L.sp_frame_bound.restype = u64
    L.sp_wire_bound.argtypes = [u64, u32, ci, ci, ci]
    L.sp_wire_bound.restype = u64
    L.sp_most.argtypes = [u64, u32, ci, ci, ci, vp]
    L.sp_most.restype = None
    L.sp_control.argtypes = [u32, vp, u32, u32, ci, u32, vp, vp]
    L.sp_control.restype = ctypes.c_int32
    L.sp_constants.argtypes = [vp]
    L.sp_constants.restype = None
    return L


def c_message(L, payload, op, comp, keys, frame_max, frag):
    size = M.wire_size(len(payload), frame_max, keys is not None, comp, frag)
    out = (ctypes.c_uint8 * (size + 1))()
    out[size] = 0xA5
    src = (ctypes.c_uint8 * max(len(payload), 1)).from_buffer_copy(payload or b"\0")
    kp = (ctypes.c_uint32 * max(len(keys), 1))(*keys) if keys is not None else None
    got = L.sp_message(src, len(payload), op, int(comp), kp, frame_max, int(frag), out)
    assert got == size and out[size] == 0xA5
    return bytes(out)[:size]


def test_constants_and_upper_bound(shim):
    o = (ctypes.c_uint32 * 8)()
    shim.sp_constants(o)
    assert list(o) == [M.CTL_SLOT, M.CTL_WIRE, 125, 123, M.NEED_BUFFERS, M.BUFFER_OVERFLOW, M.BAD_OPCODE,
                       M.BAD_CONTROL_SIZE]
    assert M.BUFFER_OVERFLOW == FM.ERR["buffer_overflow"] and M.BAD_OPCODE == FM.ERR["bad_opcode"]
    assert M.BAD_CONTROL_SIZE == FM.ERR["bad_control_size"]
    for n in list(range(0, 300)) + [4095, 4096, 65535, 65536, 1 << 20, (1 << 32) - 1]:
        assert shim.sp_deflate_bound(n) == O.upper_bound(n) == M.upper_bound(n), n


def test_decision(shim):
    """begin_msg's rule at threshold - 1, threshold, threshold + 1 with opt and
    pmd_on off and on (the cases of the reference's write.cpp:659-807)."""
    for threshold in (0, 1, 2, 125, 126, 4096, 65536, (1 << 32) - 1, 1 << 40):
        for n in {max(threshold - 1, 0), threshold, threshold + 1, 0}:
            for pmd_on in (False, True):
                for opt in (False, True):
                    want = pmd_on and opt and n >= threshold
                    assert M.compress(pmd_on, opt, n, threshold) == want
                    assert bool(shim.sp_compress(int(pmd_on), int(opt), n, threshold)) == want, \
                        (threshold, n, pmd_on, opt)
    assert M.compress(True, True, 0, 0) and not M.compress(True, True, 0, 1)


def test_split_sizes_and_offsets_match_model(shim):
    """Frame count, wire size and every frame's closed-form offsets against the
    model's serial walk, over the length grid, both roles, both frag values,
    compressed and not."""
    n = 0
    o3 = (ctypes.c_uint64 * 3)()
    for fm in FRAME_MAX:
        for ln in lengths(fm):
            for masked in (False, True):
                for frag in (False, True):
                    for comp in (False, True):
                        walk = M.frame_offsets(ln, fm, masked, comp, frag)
                        shim.sp_split(ln, fm, int(comp), int(frag), o3)
                        assert o3[0] == len(walk) == M.frame_count(ln, fm, comp, frag), (fm, ln, masked, frag, comp)
                        assert shim.sp_wire_size(ln, fm, int(masked), int(comp), int(frag)) == \
                            M.wire_size(ln, fm, masked, comp, frag), (fm, ln, masked, frag, comp)
                        if not comp and not frag:
                            assert len(walk) == 1
                        # every frame of short walks; the ends and a sample of long ones
                        fs = range(len(walk)) if len(walk) <= 8 else \
                            sorted({0, 1, len(walk) // 2, len(walk) - 2, len(walk) - 1})
                        for f in fs:
                            shim.sp_frame(ln, fm, int(masked), int(comp), int(frag), f, o3)
                            assert tuple(o3) == walk[f], (fm, ln, masked, frag, comp, f)
                        n += 1
    assert n >= 9 * 140 * 8


def test_header_bytes_match_the_oracle(shim):
    rng = random.Random(5)
    out = (ctypes.c_uint8 * 14)()
    for ln in (0, 1, 125, 126, 127, 65535, 65536, 70000, (1 << 32) - 1):
        for first in (False, True):
            for fin in (False, True):
                for rsv1 in (False, True):
                    for key in (None, rng.getrandbits(32), 0, 0xFFFFFFFF):
                        op = rng.choice([1, 2])
                        hl = shim.sp_header(ln, int(first), int(fin), int(rsv1), op, int(key is not None), key or 0,
                                            out)
                        want = FM.frame(b"", op if first else 0, fin, 4 if (rsv1 and first) else 0, key)
                        # FM.frame writes the length of its (empty) payload: patch in ln's field
                        b0 = want[0:1]
                        m = 0x80 if key is not None else 0
                        field = bytes([m | ln]) if ln <= 125 else bytes([m | 126]) + ln.to_bytes(2, "big") \
                            if ln <= 65535 else bytes([m | 127]) + ln.to_bytes(8, "big")
                        want = b0 + field + (key.to_bytes(4, "little") if key is not None else b"")
                        assert bytes(out)[:hl] == want, (ln, first, fin, rsv1, key)


def test_messages_match_the_oracle_framer(shim):
    """Whole messages written by the closed form (last frame first) equal
    O.frame_write at the model's frame size, and the receive model reads them
    back."""
    rng = random.Random(6)
    n = 0
    for fm in FRAME_MAX:
        lens = [ln for ln in lengths(fm) if ln <= 131 or ln % 7 == 0 or abs(ln - 65535) <= 5 or ln % fm <= 1
                or ln % fm == fm - 1]
        if fm <= 2:
            lens = [ln for ln in lens if ln <= 300]
        for ln in lens:
            payload = rng.randbytes(ln)
            for masked in (False, True):
                frag, comp, op = rng.random() < 0.5, rng.random() < 0.5, rng.choice([1, 2])
                for frag, comp in ((frag, comp), (not frag, not comp)):
                    nf = M.frame_count(ln, fm, comp, frag)
                    keys = [rng.getrandbits(32) for _ in range(nf)] if masked else None
                    want = M.wire(payload, op, comp, keys, fm, frag)
                    assert c_message(shim, payload, op, comp, keys, fm, frag) == want, (fm, ln, masked, frag, comp)
                    n += 1
            # parsed back by the receive side's model
            out = bytearray(ln)
            s = FM.walk(want, FM.SERVER if masked else FM.CLIENT, True, 0, ln, FM.State(), out)
            assert (s.event, s.status, s.consumed, s.out_len, s.op, s.compressed) == \
                (FM.EV_MESSAGE, 0, len(want), ln, op, int(comp))
            assert bytes(out) == payload
    assert n >= 2000


def test_bounds_cover_every_decision_and_deflate_result(shim):
    """Both host bounds >= the actual frames and wire bytes for every payload
    length up to upper_bound(len): by the shim's loop over all of them (its
    split and wire_size are the ones checked against the model above), and by
    the model itself for the short lengths."""
    o2 = (ctypes.c_uint64 * 2)()
    for fm in FRAME_MAX:
        lens = [ln for ln in lengths(fm) if ln <= 130 or ln >= 65530 or ln % fm == 0]
        if fm <= 2:
            lens = [ln for ln in lens if ln <= 130 or ln in (65535, 65536, 65540)]
        for ln in lens:
            for masked in (False, True):
                for frag in (False, True):
                    for may in (False, True):
                        shim.sp_most(ln, fm, int(masked), int(may), int(frag), o2)
                        fb = shim.sp_frame_bound(ln, fm, int(may), int(frag))
                        wb = shim.sp_wire_bound(ln, fm, int(masked), int(may), int(frag))
                        assert fb >= o2[0] and wb >= o2[1], (fm, ln, masked, frag, may)
                        # tight: some decision and deflate result reaches them
                        assert (fb, wb) == tuple(o2), (fm, ln, masked, frag, may)
    for fm in (1, 2, 125, 126, 127, 4096):
        for ln in range(0, 131, 3):
            for masked in (False, True):
                for frag in (False, True):
                    fb = shim.sp_frame_bound(ln, fm, 1, int(frag))
                    wb = shim.sp_wire_bound(ln, fm, int(masked), 1, int(frag))
                    for z in range(M.upper_bound(ln) + 1):
                        assert fb >= M.frame_count(z, fm, True, frag) and wb >= M.wire_size(z, fm, masked, True, frag)
                    assert fb >= M.frame_count(ln, fm, False, frag) and wb >= M.wire_size(ln, fm, masked, False, frag)
                    assert shim.sp_frame_bound(ln, fm, 0, int(frag)) == M.frame_count(ln, fm, False, frag)
                    assert shim.sp_wire_bound(ln, fm, int(masked), 0, int(frag)) == \
                        M.wire_size(ln, fm, masked, False, frag)


def test_torch_bounds_equal_the_header(shim):
    """pmd.send_bounds (sizing on the device, no host loop) restates the two bounds"""
    import torch

    from beast_amd import pmd
    for fm in FRAME_MAX:
        lens = [ln for ln in lengths(fm) if ln <= 130 or ln >= 65530 or ln % fm <= 1]
        t = torch.tensor(lens, dtype=torch.int32)
        for masked in (False, True):
            for frag in (False, True):
                for may in (False, True):
                    fb, wb = pmd.send_bounds(t, fm, masked, may, frag)
                    assert fb.tolist() == [shim.sp_frame_bound(ln, fm, int(may), int(frag)) for ln in lens]
                    assert wb.tolist() == [shim.sp_wire_bound(ln, fm, int(masked), int(may), int(frag))
                                           for ln in lens]
        mix = torch.tensor([i % 2 for i in range(len(lens))], dtype=torch.uint8)
        fb, wb = pmd.send_bounds(t, fm, True, mix, True)
        assert wb.tolist() == [shim.sp_wire_bound(ln, fm, 1, i % 2, 1) for i, ln in enumerate(lens)]


def c_control(L, op, slot, code, key):
    buf = (ctypes.c_uint8 * max(len(slot), 1)).from_buffer_copy(bytes(slot) or b"\0")
    out = (ctypes.c_uint8 * M.CTL_WIRE)(*([0xA5] * M.CTL_WIRE))
    size = ctypes.c_uint32()
    st = L.sp_control(op, buf, len(slot), code, int(key is not None), key or 0, out, ctypes.byref(size))
    assert all(b == 0xA5 for b in bytes(out)[size.value:])
    return st, bytes(out)[:size.value]


def test_control_model_is_pinned_by_the_rfc():
    """RFC 6455 5.7: an unmasked ping and a masked pong carrying "Hello" """
    assert M.control(M.OP_PING, b"Hello") == (0, bytes.fromhex("890548656c6c6f"))
    assert M.control(M.OP_PONG, b"Hello", key=int.from_bytes(bytes.fromhex("37fa213d"), "little")) == \
        (0, bytes.fromhex("8a8537fa213d7f9f4d5158"))
    assert M.control(M.OP_CLOSE, b"", 1000) == (0, bytes.fromhex("880203e8"))
    assert M.control(M.OP_CLOSE, b"ignored", 0) == (0, bytes.fromhex("8800"))


def test_control_frames_match_model_and_parse_back(shim):
    rng = random.Random(8)
    n = 0
    cases = [(op, ln, 0) for op in (M.OP_PING, M.OP_PONG) for ln in range(0, 129)]
    cases += [(M.OP_CLOSE, ln, code) for code in (0, 1000, 1001, 4999) for ln in (0, 1, 2, 122, 123, 124, 125, 128)]
    cases += [(op, ln, code) for op in (0, 1, 2, 3, 7, 11, 15) for ln in (0, 5) for code in (0, 1000)]
    for op, ln, code in cases:
        slot = bytes(rng.choice(b"abcdefghij klmnop") for _ in range(ln))
        for key in (None, rng.getrandbits(32)):
            want = M.control(op, slot, code, key)
            assert c_control(shim, op, slot, code, key) == want, (op, ln, code, key)
            if want[0]:
                assert want[1] == b""
                assert want[0] == (M.BAD_CONTROL_SIZE if op in (8, 9, 10) else M.BAD_OPCODE)
                continue
            s = FM.walk(want[1], FM.SERVER if key is not None else FM.CLIENT, True, 0, 0, FM.State(), bytearray())
            ev = {8: FM.EV_CLOSE, 9: FM.EV_PING, 10: FM.EV_PONG}[op]
            assert (s.event, s.status, s.consumed) == (ev, 0, len(want[1])), (op, ln, code, key)
            if op == 8:
                assert s.close_code == code and s.ctl == (code.to_bytes(2, "big") + slot if code else b"")
            else:
                assert s.ctl == slot
            n += 1
    assert n >= 2 * (2 * 126 + 4 * 5)


def test_entry_points_validate_before_device_use():
    """bpmd_send_batch / bpmd_control_batch: bad arguments are refused and
    n == 0 is a no-op; none of it touches a device."""
    from beast_amd import pmd
    L = pmd._send_lib()
    cfg = pmd._Cfg(6, 15, 4, 0, 0)

    def send(n=0, role=pmd.ROLE_SERVER, pmd_on=1, frame_max=4096, cfg=cfg, ptrs=None, keys=(None, None)):
        p = ptrs or [None] * 15
        return L.bpmd_send_batch(ctypes.byref(cfg) if cfg else None, p[0], p[1], p[2], n, role, pmd_on, 0, 1, frame_max,
                                 p[3], p[4], p[5], p[6], p[7], p[8], keys[0], keys[1], p[9], 0, p[10], p[11], p[12],
                                 p[13], p[14], None)

    assert send() == 0 and send(role=pmd.ROLE_CLIENT) == 0 and send(pmd_on=0, cfg=None) == 0
    assert send(frame_max=0) == -1
    assert send(role=2) == -1 and send(role=-1) == -1
    assert send(cfg=None) == -1                          # the deflater's cfg check
    assert send(cfg=pmd._Cfg(10, 15, 4, 0, 0)) == -1
    assert send(cfg=pmd._Cfg(6, 7, 4, 0, 0)) == -1
    assert send(n=1) == -1                               # NULL required pointers
    assert send(n=1, pmd_on=0, cfg=None) == -1
    # everything there but the keys, client role: refused before the device is looked for
    dummy = (ctypes.c_uint64 * 4)()
    some = [ctypes.cast(dummy, ctypes.c_void_p)] * 15
    assert send(n=1, role=pmd.ROLE_CLIENT, ptrs=some) == -1
    assert send(n=1, role=pmd.ROLE_CLIENT, ptrs=some, keys=(some[0], None)) == -1
    assert L.bpmd_control_batch(None, None, None, None, None, 0, None, None, None, None) == 0
    assert L.bpmd_control_batch(None, None, None, None, None, 1, None, None, None, None) == -1
    assert L.bpmd_send_frame_bound(100, 0, 1, 1) == 0 and L.bpmd_send_wire_bound(100, 0, 1, 1, 1) == 0
    assert pmd.send_frame_bound(0, 4096) == 1 and pmd.send_wire_bound(0, 4096, masked=True) == \
        M.wire_size(M.upper_bound(0), 4096, True, True, True)
    for ln in (0, 1, 125, 126, 4096, 65536, 70000):
        for fm in (1, 126, 4096, 70000):
            for frag in (False, True):
                assert pmd.send_frame_bound(ln, fm, False, frag) == M.frame_count(ln, fm, False, frag)
                assert pmd.send_wire_bound(ln, fm, True, False, frag) == M.wire_size(ln, fm, True, False, frag)
    assert pmd.CTL_WIRE == M.CTL_WIRE and pmd.CTL_SLOT == M.CTL_SLOT


def test_sanitized_run_of_the_plan():
    """tests/cpp/send_plan_main.cpp under -fsanitize=address,undefined"""
    build = os.path.join(CPP, "_build")
    os.makedirs(build, exist_ok=True)
    src, out = os.path.join(CPP, "send_plan_main.cpp"), os.path.join(build, "send_plan_main")
    hdrs = [os.path.join(CSRC, "send_plan.h"), os.path.join(CSRC, "frame_parse.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
