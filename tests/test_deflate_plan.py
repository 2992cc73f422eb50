"""The chunk-parallel deflater's rules (beast_amd/csrc/deflate_plan.h) on the
CPU.  The header compiles with plain g++ into a shim
(tests/cpp/deflate_plan_shim.cpp) that holds a byte-serial host stitch
(tests/cpp/deflate_plan_stitch.h): which chunk gets a marker, where each byte
goes, the room each step asks for and the tail are the header's, the loops
that move the bytes are the test's.

Here Python builds chunk blocks as the chunk kernel leaves them in their slots
and, independently, the payload as a string of bits: blocks concatenated, a
stored block or a marker aligned where DEFLATE aligns it, `000` and the pad at
the end.  Every sequence of 1, 2 and 3 chunks over {stored, Huffman} x 0 to 8
data bytes goes through the stitch at every capacity from 0 to two bytes past
its payload.  A Huffman block is a fixed-Huffman block of the literals 65 (8
bits) and 200 (9 bits) with BFINAL 0, so its length is known to the bit; the
sequences reach every start phase 0 to 7, both tail sizes, and a marker before
and after both kinds.  tests/cpp/deflate_plan_main.cpp runs the same stitch
under the address and undefined-behaviour sanitizers on heap blocks of exactly
`cap` bytes."""
import ctypes
import itertools
import os
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beast_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
U32 = (1 << 32) - 1
OK, NEED_BUFFERS = 0, 1
STRIDE = 32   # bytes per test slot: the longest block here is 1 + 4 + 8 bytes
STORED, HUFF = "S", "H"
KEY = 0xA1B2C3D4

u8p, u32p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_plan")
    lib = d / "libdp.so"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC,
                    os.path.join(CPP, "deflate_plan_shim.cpp"), "-o", str(lib)], check=True)
    L = ctypes.CDLL(str(lib))
    u64, u32, ci = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    L.dp_chunk.restype = L.dp_slot.restype = u32
    L.dp_chunk_count.argtypes, L.dp_chunk_count.restype = [u32, ci], u32
    L.dp_chunk_bound.argtypes, L.dp_chunk_bound.restype = [u32, u32], u64
    L.dp_word.argtypes, L.dp_word.restype = [ci, ci, u32], u32
    L.dp_read_word.argtypes, L.dp_read_word.restype = [u32, u32p], None
    L.dp_marker_before.argtypes, L.dp_marker_before.restype = [u32, ci], ci
    L.dp_layout.argtypes, L.dp_layout.restype = [u32, u32, u64, u64p], None
    L.dp_one_launch_setup.argtypes, L.dp_one_launch_setup.restype = [ci, u64, u32], ci
    L.dp_stitch.argtypes = [ctypes.c_char_p, u64, u32p, u32, u32, u32, u8p, u32, u32p]
    L.dp_stitch.restype = None
    L.dp_sweep.argtypes, L.dp_sweep.restype = [ctypes.c_char_p, u64, u32p, u32, u32, u32, ctypes.c_char_p, u32p], None
    return L


def test_header_needs_no_hip():
    """deflate_plan.h compiles with plain g++, warnings on, and includes nothing of HIP or of the library."""
    header = os.path.join(CSRC, "deflate_plan.h")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include",
                        header, os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    deps = subprocess.run(["g++", "-std=c++17", "-MM", "-x", "c++", header], capture_output=True, text=True, check=True)
    names = {os.path.basename(p) for p in deps.stdout.replace("\\\n", " ").split()}
    assert "pmd_internal.h" not in names and "pmd_common.h" not in names, names
    assert not [n for n in names if n.startswith("hip")], names
    # the host model stays an independent restatement
    with open(os.path.join(ROOT, "tests", "model", "deflate_model.cpp")) as f:
        assert "deflate_plan.h" not in f.read()


# ------------------------------------------------------------ blocks and model

def _bits_lsb(value, n):
    """n bits of value, the low bit first (how DEFLATE packs everything but Huffman codes)"""
    return "".join(str((value >> i) & 1) for i in range(n))


def _fixed_code(sym):
    """RFC 1951 3.2.6, the code's high bit first (how DEFLATE packs Huffman codes)"""
    if sym < 144:
        return format(0x30 + sym, "08b")
    if sym < 256:
        return format(0x190 + sym - 144, "09b")
    return format(sym - 256, "07b")   # 256..279: here only the end of block


def _pack(bits):
    """a bit string to bytes, the first bit in the low bit of byte 0"""
    bits = bits + "0" * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8][::-1], 2) for i in range(0, len(bits), 8))


def _data(kind, n, seed):
    if kind == HUFF:   # literals of 8 and 9 bits, the mix moved by the seed
        return bytes(65 if (seed >> i) & 1 else 200 for i in range(n))
    return bytes((37 * seed + 11 * i + 1) & 0xFF for i in range(n))


def _huff_bits(data):
    """a fixed-Huffman block, BFINAL 0: header, the literals, the end of block"""
    return "0" + _bits_lsb(1, 2) + "".join(_fixed_code(b) for b in data) + _fixed_code(256)


def _stored_body(data):
    return len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + data


def _aligned(bits):
    return bits + "0" * (-len(bits) % 8)


def _bytes_bits(b):
    return "".join(_bits_lsb(x, 8) for x in b)


class Seq:
    """One message: its chunks' slots and words as the chunk kernel leaves
    them, and the model of what the stitch must make of them."""

    def __init__(self, shim, spec, overflow_at=None):
        self.spec = spec
        self.datas = [_data(kind, n, 5 * c + n) for c, (kind, n) in enumerate(spec)]
        slots, words = b"", []
        bits, rooms = "", []   # the payload so far; the room every step asked for
        for c, ((kind, _), data) in enumerate(zip(spec, self.datas)):
            if kind == STORED:
                # in the slot: 000 and the pad from bit 0 take byte 0
                slot = b"\x00" + _stored_body(data)
                words.append(shim.dp_word(0, 1, 8 * len(slot)))
            else:
                slot = _pack(_huff_bits(data))
                words.append(shim.dp_word(0, 0, len(_huff_bits(data))))
            assert len(slot) <= STRIDE
            slots += slot.ljust(STRIDE, b"\xEE")
            # a marker before every Huffman-coded chunk but the first, and before a stored chunk 1
            if c >= 1 and (kind == HUFF or c == 1):
                bits = _aligned(bits + "000") + _bytes_bits(b"\x00\x00\xff\xff")
                rooms.append(len(bits) // 8 + 1)
            if kind == STORED:
                bits = _aligned(bits + "000") + _bytes_bits(_stored_body(data))
            else:
                bits += _huff_bits(data)
            rooms.append(-(-len(bits) // 8) + 1)   # its last byte, and one for the tail
        if overflow_at is not None:
            words[overflow_at] = shim.dp_word(1, 0, 0)
        self.out_bits = len(bits)
        self.payload = _pack(_aligned(bits + "000"))
        rooms.append(len(self.payload))
        self.need = max(rooms)
        self.last_huff_ends = len(bits) % 8 if spec[-1][0] == HUFF else 0
        self.slots, self.nk = slots, len(spec)
        self.words = (ctypes.c_uint32 * self.nk)(*words)

    def stitch(self, shim, cap, key=0):
        room = cap + 16
        out, res = (ctypes.c_uint8 * room)(), (ctypes.c_uint32 * 4)()
        shim.dp_stitch(self.slots, STRIDE, self.words, self.nk, key, cap, out, room, res)
        status, out_len, out_bits, touched = res
        assert touched == 0 and out_len <= cap
        return status, bytes(out[:out_len]), out_bits

    def sweep(self, shim, max_cap, key=0, full=None):
        res = (ctypes.c_uint32 * (4 * (max_cap + 1)))()
        shim.dp_sweep(self.slots, STRIDE, self.words, self.nk, key, max_cap, full or self.payload, res)
        return [tuple(res[4 * c:4 * c + 4]) for c in range(max_cap + 1)]


OPTIONS = [(kind, n) for kind in (STORED, HUFF) for n in range(9)]


def _specs(counts=(1, 2, 3)):
    for k in counts:
        yield from itertools.product(OPTIONS, repeat=k)


def test_every_sequence_at_every_capacity(shim):
    n = 0
    phases, tails, marked = set(), set(), set()
    for spec in _specs():
        s = Seq(shim, spec)
        L = len(s.payload)
        # the model's payload is DEFLATE: with the stripped tail put back it inflates to the data
        assert zlib.decompressobj(-15).decompress(s.payload + b"\x00\x00\xff\xff") == b"".join(s.datas), spec
        # the smallest accepted capacity: the payload's size, plus one byte when the
        # last block is Huffman-coded and ends 1 to 5 bits into a byte
        assert s.need == L + (1 if 1 <= s.last_huff_ends <= 5 else 0), spec
        got = s.sweep(shim, L + 2)
        for cap, (status, out_len, out_bits, flags) in enumerate(got):
            assert flags == 0, (spec, cap, flags)   # nothing at or past cap written; the payload is the full one
            if cap >= s.need:
                assert (status, out_len, out_bits) == (OK, L, s.out_bits), (spec, cap)
            else:
                assert (status, out_len, out_bits) == (NEED_BUFFERS, 0, 0), (spec, cap)
        assert [g[0] for g in got] == sorted((g[0] for g in got), reverse=True)   # monotone in cap
        status, payload, out_bits = s.stitch(shim, s.need)
        assert (status, payload, out_bits) == (OK, s.payload, s.out_bits), spec
        n += 1
        tails.add(L - s.out_bits // 8)
        phases.add(s.out_bits % 8)
        marked.update((a[0], b[0]) for a, b in zip(spec, spec[1:]))
    assert n == 18 + 18 ** 2 + 18 ** 3 == 6174
    assert phases == set(range(8)) and tails == {1, 2} and len(marked) == 4


def test_masked_output_is_the_payload_xor_the_key(shim):
    n = 0
    for spec in _specs((2, 3)):
        s = Seq(shim, spec)
        want = bytes(b ^ ((KEY >> (8 * (p & 3))) & 0xFF) for p, b in enumerate(s.payload))
        status, got, out_bits = s.stitch(shim, s.need, KEY)
        assert (status, got, out_bits) == (OK, want, s.out_bits), spec
        n += spec[1][0] == STORED
    assert n >= 18 * 9   # a stored chunk 1 and its marker


def test_masked_capacity_sweep(shim):
    """the key changes no decision: a subset of the sequences at every cap"""
    for spec in _specs((2,)):
        s = Seq(shim, spec)
        want = bytes(b ^ ((KEY >> (8 * (p & 3))) & 0xFF) for p, b in enumerate(s.payload))
        for cap, (status, out_len, _, flags) in enumerate(s.sweep(shim, len(want) + 2, KEY, want)):
            assert flags == 0 and (status, out_len) == ((OK, len(want)) if cap >= s.need else (NEED_BUFFERS, 0))


def test_an_overflowed_chunk_refuses_the_message(shim):
    for spec in itertools.chain(_specs((1, 2)), itertools.product(OPTIONS[::4], repeat=3)):
        for at in range(len(spec)):
            s = Seq(shim, spec, overflow_at=at)
            assert s.stitch(shim, len(s.payload) + 64) == (NEED_BUFFERS, b"", 0), (spec, at)


# ------------------------------------------------------------------- tables

def test_constants_and_the_word(shim):
    assert shim.dp_chunk() == 4096 and shim.dp_slot() == 4736 and shim.dp_slot() % 16 == 0
    assert shim.dp_slot() >= 4096 + 512 + 64 + 11 + 2   # bpmd_deflate_upper_bound(4096) + 2
    o = (ctypes.c_uint32 * 3)()
    for overflow, stored, nbits in [(0, 0, 0), (0, 0, 10), (0, 1, 40), (0, 1, 8 * 4736), (0, 0, 8 * 4736 - 1), (1, 0, 0),
                                    (1, 1, 77)]:
        w = shim.dp_word(overflow, stored, nbits)
        shim.dp_read_word(w, o)
        assert w == (0xFFFFFFFF if overflow else (0x80000000 if stored else 0) | nbits)
        assert o[0] == overflow and (overflow or (o[1], o[2]) == (stored, nbits))
    for c in range(5):
        assert shim.dp_marker_before(c, 0) == int(c >= 1) and shim.dp_marker_before(c, 1) == int(c == 1)


def test_chunk_count(shim):
    want = {0: (0, 0), 1: (0, 1), 4096: (0, 1), 4097: (2, 2), 8192: (2, 2), 8193: (3, 3)}
    for ln, (plain, hist) in want.items():
        assert (shim.dp_chunk_count(ln, 0), shim.dp_chunk_count(ln, 1)) == (plain, hist), ln


def test_chunk_bound_is_64_bit(shim):
    for x in (0, 1, 4096, U32):
        assert shim.dp_chunk_bound(0, x) == 0
    assert shim.dp_chunk_bound(1, 1) == 1
    assert shim.dp_chunk_bound(65536, 65536) == 65536 * 16 == 1 << 20
    assert shim.dp_chunk_bound(1 << 20, 1 << 24) == 1 << 32          # passes 2^32
    assert shim.dp_chunk_bound(U32, U32) == U32 * (1 << 20)
    for n, L in [(1, 4096), (1, 4097), (7, 9000), (1000, 1)]:
        assert shim.dp_chunk_bound(n, L) == n * -(-L // 4096) == n * shim.dp_chunk_count(L, 1)


def test_a_bound_past_32_bits_is_refused():
    """bpmd_send_takeover_batch, the caller with a bound: n * ceil(L / 4096) = 2^32 is an invalid
    argument, before anything touches a device.  Every pointer is set, so the bound is the only
    reason left to refuse; one chunk fewer passes the check (it would go on to the device)."""
    from beast_amd import pmd
    lib = pmd._send_tk_lib()
    cfg = pmd._Cfg(6, 15, 4, 0, 0)
    dummy = (ctypes.c_uint64 * 4)()
    none = [ctypes.cast(dummy, ctypes.c_void_p)] * 21
    slot = 2 * 4096 + (1 << 24)

    def send(n):
        return lib.bpmd_send_takeover_batch(ctypes.byref(cfg), none[0], none[1], none[2], n, pmd.ROLE_SERVER, 0, 1, 4096,
                                            U32, *none[3:7], slot, *none[7:15], 1 << 20, *none[15:], None)

    assert send(1 << 20) == -1 and send(0) == 0


def test_layout(shim):
    assert shim.dp_size_t_bytes() == 8
    o = (ctypes.c_uint64 * 6)()
    a = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for n, total in [(1, 0), (1, 1), (3, 17), (1, U32)]:
        for scan in (0, 1, 767):
            shim.dp_layout(n, total, scan, o)
            first, items, bits, slots, scan_at, size = o
            assert all(x % 256 == 0 for x in o), tuple(o)
            # first | items | bits | slots | scan, each where the one before it ends
            assert first == 0 and items == a(4 * (n + 1)) and bits == items + a(4 * total)
            assert slots == bits + a(4 * total) and scan_at == slots + a(4736 * total) and size == scan_at + a(scan)
            assert size >= 4 * (n + 1) + 8 * total + 4736 * total + scan   # no 32-bit wrap
    shim.dp_layout(3, 17, 767, o)
    assert tuple(o) == (0, 256, 512, 768, 768 + 80640, 768 + 80640 + 768)


def test_chunk_count_sources(shim):
    READ_BACK, EXACT, BOUND = 0, 1, 2
    assert shim.dp_default_kind_is_read_back() == 1
    for n in (0, 1, 2, 1000):
        for chunks in (0, 1, 5, 1 << 33):
            assert shim.dp_one_launch_setup(READ_BACK, chunks, n) == 0
            assert shim.dp_one_launch_setup(BOUND, chunks, n) == 0
            assert shim.dp_one_launch_setup(EXACT, chunks, n) == int(n == 1)


def test_sanitized_run_of_the_plan():
    """tests/cpp/deflate_plan_main.cpp under -fsanitize=address,undefined"""
    build = os.path.join(CPP, "_build")
    os.makedirs(build, exist_ok=True)
    src, out = os.path.join(CPP, "deflate_plan_main.cpp"), os.path.join(build, "deflate_plan_main")
    deps = [src, os.path.join(CPP, "deflate_plan_stitch.h"), os.path.join(CSRC, "deflate_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, deps)):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
