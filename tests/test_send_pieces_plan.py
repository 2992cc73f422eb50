"""The piece rules of the chained send (beast_amd/csrc/send_pieces_plan.h) on
the CPU: the header compiles with plain g++ into a shim
(tests/cpp/send_pieces_plan_shim.cpp) and is compared with the Python model
(tests/send_pieces_model.py) over the cross product of states, opcodes,
options, lengths, positions and statuses at which a rule changes its answer.
The model's piece payloads, markers kept behind the non-final ones, are
checked against the oracle's inflater -- kept across a takeover connection's
messages, reset after each message under no_context_takeover -- with
uncompressed messages in between, and tests/cpp/send_pieces_plan_main.cpp runs
the header under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import oracle as O
from tests import send_model as SM
from tests import send_pieces_model as PM
from tests import send_takeover_model as TM
from tests import takeover_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beast_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
K = TM.K
U32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("send_pieces_plan")
    lib = d / "libspp.so"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC,
                    os.path.join(CPP, "send_pieces_plan_shim.cpp"), "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    u64, u32, i32, ci, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p
    L.spp_state_bytes.restype = u32
    L.spp_keep.restype = u32
    L.spp_begin.argtypes, L.spp_begin.restype = [vp, u32, ci, u64, u64, vp], None
    L.spp_provisional.argtypes, L.spp_provisional.restype = [u32, ci, u64, u32], i32
    L.spp_status.argtypes, L.spp_status.restype = [i32, ci, i32, ci, u64, u64], i32
    L.spp_payload_len.argtypes, L.spp_payload_len.restype = [ci, ci, u64, u64], u64
    L.spp_frame_first.argtypes, L.spp_frame_first.restype = [u64, ci], ci
    L.spp_frame_fin.argtypes, L.spp_frame_fin.restype = [u64, u64, ci], ci
    L.spp_commit.argtypes, L.spp_commit.restype = [vp, u32, u32, ci, vp, ci, i32, ci, ci, vp], None
    L.spp_piece_frame_bound.argtypes, L.spp_piece_frame_bound.restype = [u64, u32, ci, ci, ci], u64
    L.spp_piece_wire_bound.argtypes, L.spp_piece_wire_bound.restype = [u64, u32, ci, ci, ci, ci], u64
    L.spp_header.argtypes, L.spp_header.restype = [u64, u64, u64, ci, ci, ci, u32, ci, u32, vp], u32
    return L


def _state(cont, comp, sop):
    return (ctypes.c_uint8 * 4)(cont, comp, sop, 0)


def test_state_is_four_bytes_and_keep_is_the_takeover_keep(shim):
    from beast_amd import pmd
    assert shim.spp_state_bytes() == 4 == pmd.WR_STATE_BYTES
    assert shim.spp_keep() == K == pmd.PieceSender.HIST


SLOT = 2 * K + 4097
THR = 301


def _lengths(L):
    return sorted({0, 1, THR - 1, THR, 4095, 4096, 4097, L - 1, L, L + 1})


def _positions(slot, n):
    s = {0, K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, slot - n - 1, slot - n, slot - n + 1, slot - 1, slot}
    return sorted(p for p in s if 0 <= p <= slot)


def test_plan_matches_model(shim):
    """begin, provisional, place, status, payload length, commit"""
    o2, o5 = (ctypes.c_uint32 * 2)(), (ctypes.c_uint32 * 5)()
    L = TM.room(U32, SLOT)
    assert L == 4097
    n = cont_kept = resets = refused = 0
    z = 57    # the deflater's length: the marker's room is z_cap - z, whatever z is
    for cont in (0, 1):
        for comp in (0, 1):
            for sop in ((1, 2) if cont else (0,)):
                if not cont and comp:
                    continue    # all zero is the only state with no message open
                st0 = (cont, comp, sop)
                for op in (0, 1, 2, 3):
                    for opt in (0, 1):
                        for ln in _lengths(L):
                            b = PM.begin(st0, op, opt, ln, THR)
                            if op not in (1, 2):
                                assert b == (0, op)
                            elif cont:
                                assert b == (comp, sop)      # whatever opt, op and the length say
                                cont_kept += 1
                            else:
                                assert b == (int(bool(opt) and ln >= THR), op)
                            shim.spp_begin(_state(*st0), op, opt, ln, THR, o2)
                            assert tuple(o2) == b, (st0, op, opt, ln)
                            prov = PM.provisional(op, b[0], ln, L)
                            assert prov == (SM.BAD_OPCODE if op == 3 else TM.MESSAGE_TOO_BIG if b[0] and ln > L else 0)
                            assert shim.spp_provisional(op, b[0], ln, L) == prov
                            enters = bool(b[0] and prov == 0)
                            for fin in (0, 1):
                                for zst in (0, SM.NEED_BUFFERS):
                                    for z_cap in (z + 3, z + 4):
                                        st = PM.status(prov, enters, zst, fin, z, z_cap)
                                        want = prov or (zst if enters else 0)
                                        if not want and enters and not fin and z_cap < z + 4:
                                            want = SM.NEED_BUFFERS
                                        assert st == want
                                        assert shim.spp_status(prov, int(enters), zst, fin, z, z_cap) == st
                                pl = PM.payload_len(b[0], fin, ln, z)
                                assert pl == ((z if fin else z + 4) if b[0] else ln)
                                assert shim.spp_payload_len(b[0], fin, ln, z) == pl
                                for pos in _positions(SLOT, ln):
                                    slide, new_pos, z_in, hist = TM.place(pos, ln, SLOT, K, enters)
                                    for final in (0, SM.NEED_BUFFERS, SM.BUFFER_OVERFLOW) if prov == 0 else (prov,):
                                        for nt in (0, 1):
                                            got = PM.commit(st0, new_pos, ln, enters, b, op == 0, final, fin, nt)
                                            if final or op == 0:
                                                assert got == (new_pos, st0)
                                                refused += final != 0
                                            else:
                                                reset = fin and b[0] and nt
                                                resets += bool(reset)
                                                assert got == (0 if reset else new_pos + ln if enters else new_pos,
                                                               (0 if fin else 1, b[0], b[1]))
                                            bb = (ctypes.c_uint32 * 2)(*b)
                                            shim.spp_commit(_state(*st0), new_pos, ln, int(enters), bb, int(op == 0),
                                                            final, fin, nt, o5)
                                            assert (o5[0], (o5[1], o5[2], o5[3])) == got and o5[4] == 0
                                            n += 1
    assert n >= 20000 and cont_kept >= 100 and resets >= 300 and refused >= 3000, (n, cont_kept, resets, refused)


def test_frame_flags_and_headers(shim):
    """opcode and RSV1 on a message's first frame only, FIN on its last only,
    and the header bytes equal the model's patched oracle frames"""
    out = (ctypes.c_uint8 * 16)()
    for frames in (1, 2, 3):
        for f in range(frames):
            for cont in (0, 1):
                assert shim.spp_frame_first(f, cont) == int(f == 0 and not cont)
            for fin in (0, 1):
                assert shim.spp_frame_fin(f, frames, fin) == int(f + 1 == frames and bool(fin))
    rng = random.Random(5)
    for frame_max in (7, 125, 126, 4096):
        for n in (0, 1, frame_max - 1, frame_max, frame_max + 1, 2 * frame_max + 3):
            body = bytes(rng.randrange(256) for _ in range(n))
            for comp in (0, 1):
                for cont in (0, 1):
                    for fin in (0, 1):
                        for masked in (0, 1):
                            nf = SM.frame_count(n, frame_max, bool(comp), True)
                            keys = [rng.getrandbits(32) for _ in range(nf)] if masked else None
                            w = PM.wire_piece(body, 2, bool(comp), not cont, bool(fin), keys, frame_max, True)
                            offs = SM.frame_offsets(n, frame_max, bool(masked), bool(comp), True)
                            assert len(offs) == nf
                            for f, (_, at, ln) in enumerate(offs):
                                hl = shim.spp_header(ln, f, nf, cont, fin, comp, 2, masked, keys[f] if masked else 0, out)
                                assert bytes(out[:hl]) == w[at:at + hl], (frame_max, n, comp, cont, fin, masked, f)
                                b0 = w[at]
                                assert b0 & 15 == (2 if f == 0 and not cont else 0)
                                assert bool(b0 & 0x40) == bool(f == 0 and not cont and comp)
                                assert bool(b0 & 0x80) == bool(f + 1 == nf and fin)


def test_bounds_match_model_and_cover_every_piece(shim):
    from beast_amd import pmd
    L = pmd._send_pc_lib()
    for frame_max in (7, 125, 126, 4096):
        for ln in (0, 1, 100, 125, 126, 4095, 4096, 4097, 65535, 65536, 70000):
            for masked in (0, 1):
                for may in (0, 1):
                    for frag in (0, 1):
                        for fin in (0, 1):
                            fb = PM.piece_frame_bound(ln, frame_max, may, frag, fin)
                            wb = PM.piece_wire_bound(ln, frame_max, masked, may, frag, fin)
                            assert shim.spp_piece_frame_bound(ln, frame_max, may, frag, fin) == fb
                            assert shim.spp_piece_wire_bound(ln, frame_max, masked, may, frag, fin) == wb
                            assert pmd.send_piece_bounds(ln, frame_max, bool(masked), bool(may), bool(frag),
                                                         bool(fin)) == (fb, wb)
                            if fin:    # a final piece is bounded like a message
                                assert fb == L.bpmd_send_frame_bound(ln, frame_max, may, frag)
                                assert wb == L.bpmd_send_wire_bound(ln, frame_max, masked, may, frag)
                            # any payload the deflater may leave, and the marker
                            for z in (0, 1, SM.upper_bound(ln)):
                                pl = PM.payload_len(may, fin, ln, z)
                                assert SM.frame_count(pl, frame_max, bool(may), bool(frag)) <= fb
                                assert SM.wire_size(pl, frame_max, bool(masked), bool(may), bool(frag)) <= wb
    assert L.bpmd_send_piece_frame_bound(10, 0, 1, 1, 0) == 0 and L.bpmd_send_piece_wire_bound(10, 0, 0, 1, 1, 0) == 0


def _cut(rng, msg, most, empty_final):
    """msg in pieces of at most `most` bytes at random cuts, empty ones among them"""
    pieces, at = [], 0
    while at < len(msg):
        ln = rng.choice((0, 1, rng.randrange(most + 1), most)) if pieces or rng.randrange(3) else rng.randrange(most + 1)
        pieces.append(msg[at:at + ln])
        at += ln
    if empty_final or not pieces:
        pieces.append(b"")       # write_some(true, {}) after the data
    return pieces


def _connection(c, rng, rounds, max_piece):
    """[(message, op, opt, pieces)]: JSON and random messages of up to three
    pieces' length, a third of them sent uncompressed"""
    out = []
    for k in range(rounds):
        ln = rng.choice((0, 1, 300, max_piece, 2 * max_piece + 17, 3 * max_piece))
        m = TC.json_message(ln, 100 * c + k) if k % 3 else TC.random_message(ln, 100 * c + k)
        out.append((m, 1 + k % 2, 0 if rng.randrange(3) == 0 else 1, _cut(rng, m, max_piece, rng.randrange(2))))
    return out


@pytest.mark.parametrize("wbits,no_takeover", [(15, 0), (15, 1), (9, 0), (9, 1)])
def test_model_payloads_are_valid_messages(wbits, no_takeover):
    """Per connection: a message's piece payloads concatenated, markers behind
    the non-final ones, inflate to the message -- through one inflater kept
    across the messages with takeover, a fresh one per message under
    no_context_takeover -- with uncompressed messages in between and through
    slides in the middle of messages.  Without the markers they do not."""
    rng = random.Random(60 + wbits + no_takeover)
    max_piece = 3000
    slot = TC.takeover_slot(K, max_piece)
    slides = plain = markers = empties = bad = 0
    for c in range(4):
        conn = _connection(c, rng, 10, max_piece)
        buf, pos, state = bytearray(b"\xee" * slot), 0, PM.ZERO
        payloads, stripped, want = [], [], []
        for m, op, opt, pieces in conn:
            got, bare, comp = b"", b"", None
            for j, p in enumerate(pieces):
                fin = j + 1 == len(pieces)
                cont = state[0]
                assert cont == int(j > 0)
                # a continuation piece: opt and the opcode given no longer matter
                e = PM.send(pos, state, buf, p, op if not cont else 3 - op, opt if not cont else 1 - opt, fin,
                            no_takeover, 0, max_piece, slot, 1 << 20, None, level=6, wbits=wbits)
                assert e.status == 0 and e.compressed == opt
                comp = e.compressed
                body = e.payload if comp else p
                assert e.wire == PM.wire_piece(body, op, bool(comp), not cont, fin, None, 4096, True)
                assert e.marked == int(bool(comp) and not fin)
                if comp:
                    assert fin or e.payload.endswith(PM.MARKER)
                    got += e.payload
                    bare += e.payload[:len(e.payload) - 4 * e.marked]
                    markers += e.marked
                    empties += len(p) == 0
                else:
                    assert e.pos == pos and not e.slid and e.payload == b""
                slides += e.slid
                pos, state = e.pos, e.state
            assert state == (0, comp, op)
            if comp:
                assert pos == 0 or not no_takeover
                payloads.append(got)
                stripped.append(bare)
                want.append(m)
            else:
                plain += 1
        cap = 3 * max_piece
        if no_takeover:
            assert [O.pmd_inflate(p, cap=cap, wbits=wbits) for p in payloads] == [(0, m) for m in want], c
            bad += [O.pmd_inflate(p, cap=cap, wbits=wbits) for p in stripped] != [(0, m) for m in want]
        else:
            assert O.pmd_inflate_stream(payloads, cap=cap, wbits=wbits) == [(0, m) for m in want], c
            bad += O.pmd_inflate_stream(stripped, cap=cap, wbits=wbits) != [(0, m) for m in want]
    assert markers >= 20 and empties >= 4 and plain >= 6, (markers, empties, plain)
    assert no_takeover or slides >= 4, slides
    assert bad == 4, bad


def test_threshold_is_decided_at_the_first_piece_only():
    """a short first piece, long ones behind it: the message stays
    uncompressed; a long first piece, short ones behind it: compressed"""
    slot = 2 * K + 4097
    buf, pos, state = bytearray(slot), 0, PM.ZERO
    for first, rest, comp in ((b"a" * 10, b"b" * 4000, 0), (b"a" * 400, b"b" * 3, 1)):
        for j, p in enumerate((first, rest, rest, b"")):
            e = PM.send(pos, state, buf, p, 1, 1, j == 3, 0, 400, 1 << 16, slot, 1 << 20, None)
            assert (e.status, e.compressed) == (0, comp)
            assert bool(e.wire[0] & 0x40) == bool(comp and j == 0)
            pos, state = e.pos, e.state
        assert pos == (0 if not comp else 406) and state == (0, comp, 1)


def test_entry_points_validate_before_device_use():
    """bpmd_send_pieces_batch: bad arguments are refused and n == 0 is a
    no-op; none of it touches a device."""
    from beast_amd import pmd
    L = pmd._send_pc_lib()
    cfg = pmd._Cfg(6, 15, 4, 0, 0)
    slot0 = 2 * K + 1
    NP = 24    # pointer arguments besides cfg and stream

    def send(n=0, role=pmd.ROLE_SERVER, cfg=cfg, frame_max=4096, max_len=100, slot=slot0, ptrs=None):
        p = ptrs or [None] * NP
        return L.bpmd_send_pieces_batch(ctypes.byref(cfg) if cfg else None, p[0], p[1], p[2], n, role, 0, 1, frame_max,
                                        max_len, *p[3:10], slot, *p[10:18], 1 << 20, *p[18:], None)

    assert send() == 0 and send(role=pmd.ROLE_CLIENT) == 0
    assert send(frame_max=0) == -1
    assert send(role=2) == -1 and send(role=-1) == -1
    assert send(cfg=None) == -1
    assert send(cfg=pmd._Cfg(6, 15, 4, 0, pmd.F_EXACT)) == -1 and send(cfg=pmd._Cfg(6, 15, 4, 0, pmd.F_RAW)) == -1
    assert send(cfg=pmd._Cfg(10, 15, 4, 0, 0)) == -1 and send(cfg=pmd._Cfg(6, 16, 4, 0, 0)) == -1
    assert send(slot=2 * K) == -1 and send(slot=0) == -1 and send(slot=slot0) == 0
    assert send(max_len=0) == -1
    big = 2 * K + (1 << 24)
    assert send(n=1 << 20, max_len=U32, slot=big) == -1
    assert send(n=1) == -1                                            # NULL required pointers
    dummy = (ctypes.c_uint64 * 4)()
    some = [ctypes.cast(dummy, ctypes.c_void_p)] * NP
    # d_op, d_opt, d_fin, d_no_takeover, and in server role d_keys, d_key_base
    optional = {3, 4, 5, 6, 15, 16}
    for k in range(NP):
        if k in optional:
            continue
        p = list(some)
        p[k] = None
        assert send(n=1, ptrs=p) == -1, k      # k == 7 is d_state
    for k in (15, 16):          # client role without keys
        p = list(some)
        p[k] = None
        assert send(n=1, role=pmd.ROLE_CLIENT, ptrs=p) == -1, k
    a = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for n in (0, 1, 63, 64, 65, 256, 257, 1 << 16):
        assert L.bpmd_send_pieces_work_bytes(n) == 3 * a(4 * n) + a(8 * n) + 2 * a(n)
    assert pmd.wr_state(3, device="cpu").tolist() == [[0, 0, 0, 0]] * 3


def test_sanitized_run_of_the_plan():
    """tests/cpp/send_pieces_plan_main.cpp under -fsanitize=address,undefined"""
    build = os.path.join(CPP, "_build")
    os.makedirs(build, exist_ok=True)
    src, out = os.path.join(CPP, "send_pieces_plan_main.cpp"), os.path.join(build, "send_pieces_plan_main")
    hdrs = [os.path.join(CSRC, h) for h in ("send_pieces_plan.h", "send_takeover_plan.h", "send_plan.h", "lz_core.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, [src] + hdrs)):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
