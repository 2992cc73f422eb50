"""Scripts for the per-stream deflater (the bpmd_deflate_stream_* ABI of
include/beast_pmd.h), a driver that runs one against any library exporting
that ABI, and the checks over a recorded run.  Shared by
tests/test_deflate_scripts.py (the oracle backend alone, no device) and
tests/test_gpu_deflate_stream.py (libbeast_pmd.so beside the oracle backend).

A script is a list of steps:
    ("write", bytes, flush)      flush: a key of FLUSH
    ("params", level, strategy)  or ("params", level, strategy, room) with that much output room
    ("tune", good, lazy, nice, chain)
    ("prime", bits, value)
    ("pending",)
    ("reset",)

Output room (the `room` argument of run()):
    None          roomy: every call gets upper_bound(all input so far) + 64
    ("tight", k)  every call gets k bytes
    ("split", j)  a flushing write gets j bytes, then roomy calls (the
                  reference's own harness, test/beast/zlib/deflate_stream.cpp:352-405)
With less than roomy output a flushing write is repeated while it returns
with avail_out == 0, as zlib's protocol asks, until a call leaves room or
nothing is left to hand out (avail_in == 0 and pending() reports no bytes).
The repeats carry the same flush when the room is at least 7 bytes.  Below
that the same flush does not end on the reference either (zlib's manual asks
for avail_out > 6 for this reason): a repeat that finds room after handing out
what was pending appends another flush marker -- 5 bytes for sync / full /
trees, 10 bits for partial -- so with 3 bytes pending and 5 of room every
repeat hands out 3, adds 5 and keeps 3.  Those repeats therefore carry
Flush::none, which only hands out what is pending.  Flush::finish is always
repeated as finish, until end_of_stream.  The number of calls per step is
capped; a run over the cap raises instead of looping.

The decoder in every check is the oracle's inflater (oracle.Inflater) at the
stream's own windowBits."""
import ctypes
import functools

from beast_amd import synth
from oracle import oracle as O

FLUSH = O.FLUSH
OK, NEED_BUFFERS, END_OF_STREAM, STREAM_ERROR = 0, 1, 2, 4
FLUSH_POINTS = ("partial", "sync", "full", "trees", "finish")
MARKER = b"\x00\x00\xff\xff"

# the reference's get_config rows (deflate_stream.hpp:571-590) as
# (good_length, max_lazy, nice_length, max_chain); level 0's row of zeros is
# left out: tune() values come from rows 1-9 only
LEVEL_ROWS = {1: (4, 4, 8, 4), 2: (4, 5, 16, 8), 3: (4, 6, 32, 32), 4: (4, 4, 16, 16), 5: (8, 16, 32, 32),
              6: (8, 16, 128, 128), 7: (8, 32, 128, 256), 8: (32, 128, 258, 1024), 9: (32, 258, 258, 4096)}


class ZParams(ctypes.Structure):
    _fields_ = [("next_in", ctypes.c_void_p), ("avail_in", ctypes.c_size_t), ("total_in", ctypes.c_size_t),
                ("next_out", ctypes.c_void_p), ("avail_out", ctypes.c_size_t), ("total_out", ctypes.c_size_t),
                ("data_type", ctypes.c_int)]


def bind(L):
    """argtypes of the per-stream deflate ABI on a loaded library."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    zp = ctypes.POINTER(ZParams)
    L.bpmd_deflate_upper_bound.argtypes = [ctypes.c_size_t]
    L.bpmd_deflate_upper_bound.restype = ctypes.c_size_t
    L.bpmd_deflate_stream_create.argtypes = [ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.bpmd_deflate_stream_reset.argtypes = [vp]
    L.bpmd_deflate_stream_write.argtypes = [vp, zp, ci]
    L.bpmd_deflate_stream_params.argtypes = [vp, zp, ci, ci]
    L.bpmd_deflate_stream_tune.argtypes = [vp, ci, ci, ci, ci]
    L.bpmd_deflate_stream_pending.argtypes = [vp, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ci)]
    L.bpmd_deflate_stream_prime.argtypes = [vp, ci, ci]
    L.bpmd_stream_destroy.argtypes = [vp]
    return L


@functools.lru_cache(maxsize=None)
def oracle_backend():
    """tests/cpp/oracle_backend.c over liboracle.so (tests/test_facade.py's recipe)."""
    from tests.test_facade import _build_oracle_backend
    return bind(ctypes.CDLL(_build_oracle_backend()))


@functools.lru_cache(maxsize=None)
def gpu_library():
    from beast_amd import pmd
    L = bind(pmd.lib())
    L.bpmd_stream_batching.argtypes = [ctypes.c_int, ctypes.c_int]
    if hasattr(L, "bpmd_stream_batching_get"):   # not in a BPMD_LIB built from an earlier commit
        L.bpmd_stream_batching_get.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    return L


def batching(L):
    """The stream batcher's setting in force: (max_calls, max_delay_us)."""
    if not hasattr(L, "bpmd_stream_batching_get"):
        return 256, 0   # the default such a library starts with
    m, d = ctypes.c_int(), ctypes.c_int()
    assert L.bpmd_stream_batching_get(ctypes.byref(m), ctypes.byref(d)) == 0
    return m.value, d.value


class Step:
    """One step of a run: the last call's return code, avail_in and total_in
    after it, the bytes the step produced, pending() after it, and for a
    write every call as (rc, bytes produced, avail_out after, pending after)."""
    __slots__ = ("op", "flush", "data", "rc", "avail_in", "total_in", "out", "pend", "calls")

    def __init__(self, op):
        self.op, self.flush, self.data = op, None, b""
        self.rc, self.avail_in, self.total_in, self.out, self.pend, self.calls = 0, 0, 0, b"", (0, 0), []

    def key(self):
        return (self.op, self.flush, self.rc, self.avail_in, self.total_in)


class CallCapExceeded(AssertionError):
    pass


def run(L, script, level=6, wbits=15, mem=8, strategy=0, room=None):
    """The script on a fresh stream of library L; returns the list of Steps."""
    h = ctypes.c_void_p()
    r = L.bpmd_deflate_stream_create(level, wbits, mem, strategy, ctypes.byref(h))
    assert r == 0, r
    zs = ZParams(None, 0, 0, None, 0, 0, 2)
    fed = 0
    steps = []

    def pending():
        v, b = ctypes.c_uint(0), ctypes.c_int(0)
        assert L.bpmd_deflate_stream_pending(h, ctypes.byref(v), ctypes.byref(b)) == 0
        return (v.value, b.value)

    def call(fn, want, *args):
        buf = ctypes.create_string_buffer(want)
        zs.next_out, zs.avail_out = ctypes.addressof(buf), want
        before = zs.total_out
        rc = fn(h, ctypes.byref(zs), *args)
        n = zs.total_out - before
        assert n <= want and zs.avail_out == want - n, (n, want, zs.avail_out)
        return rc, buf.raw[:n]

    try:
        for st in script:
            s = Step(st[0])
            roomy = L.bpmd_deflate_upper_bound(fed + (len(st[1]) if st[0] == "write" else 0)) + 64
            if st[0] == "write":
                _, data, flush = st
                s.flush, s.data = flush, bytes(data)
                fed += len(data)
                src = ctypes.create_string_buffer(s.data, len(s.data)) if data else None
                zs.next_in, zs.avail_in = (ctypes.addressof(src) if data else None), len(data)
                cap = 64 + 4 * roomy // (room[1] if room else roomy)
                out = []
                while True:
                    if len(s.calls) >= cap:
                        raise CallCapExceeded(f"{len(s.calls)} calls for {flush} of {len(data)} bytes, room {room}")
                    want = roomy
                    if room and (room[0] == "tight" or (not s.calls and flush != "none")):
                        want = room[1]
                    again = "none" if s.calls and flush != "finish" and want < 7 else flush
                    rc, got = call(L.bpmd_deflate_stream_write, want, FLUSH[again])
                    out.append(got)
                    p = pending()
                    s.calls.append((rc, len(got), zs.avail_out, p))
                    s.rc = rc
                    if rc not in (OK, NEED_BUFFERS) or (rc == NEED_BUFFERS and zs.avail_out):
                        break
                    if flush == "finish":
                        continue
                    if zs.avail_out or (zs.avail_in == 0 and p[0] == 0):
                        break
                s.out = b"".join(out)
            elif st[0] == "params":
                zs.next_in, zs.avail_in = None, 0
                s.rc, s.out = call(L.bpmd_deflate_stream_params, st[3] if len(st) > 3 else roomy, st[1], st[2])
            elif st[0] == "tune":
                s.rc = L.bpmd_deflate_stream_tune(h, *st[1:])
            elif st[0] == "prime":
                s.rc = L.bpmd_deflate_stream_prime(h, st[1], st[2])
            elif st[0] == "pending":
                pass
            elif st[0] == "reset":
                s.rc = L.bpmd_deflate_stream_reset(h)
                zs.total_in = zs.total_out = 0
                fed = 0
            else:
                raise ValueError(st[0])
            s.avail_in, s.total_in, s.pend = zs.avail_in, zs.total_in, pending()
            steps.append(s)
    finally:
        L.bpmd_stream_destroy(h)
    return steps


def output(steps):
    return b"".join(s.out for s in steps)


# ------------------------------------------------------------------- decoding

def inflate(data, expect_len, wbits, finished=False):
    """(status name, bytes) of the oracle's inflate_stream over data: write()
    with Flush::sync until a call makes no progress or returns an error or
    end_of_stream.  finished: the stream ends in its final block, and two
    zero bytes follow it: Beast's decoder wants lenbits_ (up to 9) bits in
    hand before it decodes a symbol (inflate_stream.ipp:374), so it sees a
    final end-of-block code of 7 bits only with something after it."""
    if not data:
        return "ok", b""
    if finished:
        data += b"\0\0"
    zi = O.Inflater(wbits)
    src = ctypes.create_string_buffer(data, len(data))
    cap = expect_len + 64
    buf = ctypes.create_string_buffer(cap)
    zs = O.ZParams(ctypes.addressof(src), len(data), 0, ctypes.addressof(buf), cap, 0, 2)
    st = 0
    for _ in range(64):
        before = (zs.total_in, zs.total_out)
        st = zi.write(zs, "sync")
        if st == NEED_BUFFERS and before == (zs.total_in, zs.total_out):
            st = OK   # nothing more to do with these bytes
            break
        if st not in (OK, NEED_BUFFERS) or before == (zs.total_in, zs.total_out) or zs.avail_out == 0:
            break
    return O.ERRORS.get(st, st), buf.raw[:zs.total_out]


def primed_bits_present(out, primes):
    """Every prime()'s bits [(position, bits, value)] that have reached the
    output hold the primed value."""
    v, nbits = int.from_bytes(out, "little"), 8 * len(out)
    for pos, bits, value in primes:
        have = max(0, min(bits, nbits - pos))
        assert (v >> pos) & ((1 << have) - 1) == value & ((1 << have) - 1), (pos, bits, value)


# --------------------------------------------------------------------- checks

def check_call_parity(got, ref):
    """A: per step the return code, avail_in (0) and total_in equal the
    reference run's; pending() equals it exactly after every prime() that
    starts from a byte boundary both sides are on by construction (the
    stream's start, a reset, or a sync / full / trees / finish point)."""
    assert len(got) == len(ref)
    aligned = True
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.key() == r.key(), (i, g.key(), r.key())
        if g.op != "write" or g.rc in (OK, END_OF_STREAM):
            assert g.avail_in == 0, (i, g.op, g.avail_in)
        if g.op == "prime":
            if aligned:
                assert g.pend == r.pend, (i, "pending after prime", g.pend, r.pend)
        elif g.op == "reset":
            aligned = True
        elif g.op == "write" and g.rc in (OK, END_OF_STREAM):
            aligned = g.flush in ("sync", "full", "trees", "finish") if g.flush != "none" else aligned and not g.data
        elif g.op == "params" and g.out:
            aligned = False


def check_decodable(steps, script, wbits, only_end=False):
    """B: after every partial / sync / full / trees / finish step that did
    something, all output so far decodes to exactly all input so far (ok, or
    end_of_stream after finish); after none and block to a prefix of it.
    prime()'s bits are in the output where pending() put them and decode
    with it: the scripts prime whole empty blocks (PRIMES).  Cutting the bits
    out and shifting the rest instead cannot work for a bit count that is no
    multiple of 8: whatever is padded to a byte boundary after them -- the
    empty stored block of sync / full / trees, a stored block of level 0 or
    of incompressible input -- is padded for the unshifted stream, on the
    reference as much as here."""
    primes, prev = [], (0, 0)
    last = max((i for i, s in enumerate(steps) if s.op == "write"), default=-1)
    fed, out = b"", b""
    finished = False
    for i, s in enumerate(steps):
        if s.op == "reset":
            fed, out, primes, finished = b"", b"", [], False
        elif s.op == "prime" and s.rc == OK and script[i][1]:
            primes.append((8 * (len(out) + prev[0]) + prev[1], script[i][1], script[i][2]))
        prev = s.pend
        out += s.out
        if s.op != "write":
            continue
        if finished:
            assert not s.out, (i, "output after end_of_stream")
            continue
        fed += s.data[:len(s.data) - s.avail_in]
        if s.rc == END_OF_STREAM:
            finished = True
        if only_end and i != last:
            continue
        if s.rc not in (OK, END_OF_STREAM) or (s.rc == OK and s.flush == "finish"):
            continue
        primed_bits_present(out, primes)
        status, back = inflate(out, len(fed), wbits, s.flush == "finish")
        where = (i, s.flush, len(s.data), status, len(back), len(fed))
        if s.flush in FLUSH_POINTS and (s.calls[-1][2] or s.flush == "finish"):
            assert status == ("end_of_stream" if s.flush == "finish" else "ok"), where
            assert back == fed, where
        else:   # none, block, or a flush cut short by the room (see the module docstring)
            assert status == "ok" and fed.startswith(back), where


def framing(steps):
    """C's facts per flushing write that did something: (step, flush, output
    so far ends with 00 00 FF FF, pending bytes, pending bits where the flush
    kind fixes them)."""
    out, facts = b"", []
    for i, s in enumerate(steps):
        out = b"" if s.op == "reset" else out + s.out
        if s.op == "write" and s.flush != "none" and s.rc in (OK, END_OF_STREAM):
            # after block and partial the bit count is the encoder's own parse mod 8: not comparable
            bits = s.pend[1] if s.flush in ("sync", "full", "trees", "finish") else None
            facts.append((i, s.flush, out.endswith(MARKER), s.pend[0], bits))
    return facts


def check_framing(got, ref):
    """C: compared with the reference run, not stated per flush kind.  After
    block, partial and finish the output ends in the encoder's own last
    block, and the reference's can happen to be an empty stored block (level
    0 at windowBits 9 and 10, where deflate_stored closes a block every
    2^wbits - 262 bytes and the flush then finds nothing left; after finish
    it is 01 00 00 FF FF): there the marker is only required not to appear
    where the reference has none.  What is pending is compared as elsewhere."""
    fg, fr = framing(got), framing(ref)
    assert len(fg) == len(fr)
    for g, r in zip(fg, fr):
        if g[1] in ("block", "partial", "finish"):
            assert g[:2] == r[:2] and g[3:] == r[3:] and (r[2] or not g[2]), (g, r)
        else:
            assert g == r, (g, r)


def restart_after(steps, at, wbits):
    """(status, bytes) of a fresh inflater over what the stream produced
    after step `at`, and the input written after it."""
    tail = b"".join(s.out for s in steps[at + 1:])
    fed = b"".join(s.data for s in steps[at + 1:] if s.op == "write" and s.rc in (OK, END_OF_STREAM))
    return inflate(tail, len(fed), wbits, True), fed


def check_restart(lib, script, cfg):
    """D: after every Flush::full point a fresh inflater decodes the rest of
    the stream to the input written after it.  Non-vacuity: the same script
    with sync in place of full does not restart (a fresh inflater fails or
    comes up short) and its second segment is smaller than its first, so the
    history across the flush really is used."""
    wbits = cfg.get("wbits", 15)
    steps = run(lib, script, **cfg)
    fulls = [i for i, st in enumerate(script) if st[0] == "write" and st[2] == "full" and steps[i].rc == OK]
    assert fulls
    for at in fulls:
        (status, back), fed = restart_after(steps, at, wbits)
        assert status == "end_of_stream" and back == fed, (at, status, len(back), len(fed))
    return steps


def check_sync_does_not_restart(lib, script, cfg):
    """D's non-vacuity half; the script's first two steps are writes of the
    same compressible segment."""
    wbits = cfg.get("wbits", 15)
    as_sync = [("write", st[1], "sync") if st[0] == "write" and st[2] == "full" else st for st in script]
    steps = run(lib, as_sync, **cfg)
    assert script[0][1] == script[1][1] and script[0][2] == script[1][2] == "full"
    (status, back), fed = restart_after(steps, 0, wbits)
    assert status not in ("ok", "end_of_stream") or len(back) < len(fed), (status, len(back), len(fed))
    assert len(steps[1].out) < len(steps[0].out), (len(steps[0].out), len(steps[1].out))
    return steps


def check_tight(steps, script, wbits, k, strict=False):
    """E: the concatenated output passes B at the end; every call returns
    ok, need_buffers or end_of_stream; a finish that returns ok has no room
    left and reports the number P of pending bytes, and exactly P more bytes
    come out before the single end_of_stream.  (P > 0 except where the call
    itself handed out the last byte into the last byte of room: it still
    returns ok, on the reference as here, and the next call is the
    end_of_stream.)

    strict (the GPU stream, which compresses everything in a flush's first
    call): that holds for every ok return of finish, and below 7 bytes of
    room, where the repeats of the other flushes are Flush::none calls that
    only hand out what is pending, every call of such a step reports exactly
    the bytes that the step's later calls hand out.  Without strict (the
    reference, which may return from a flush in the middle of its parse with
    more blocks to come) the finish rule is asked only of calls after which
    pending() just counts down (finish_drains)."""
    check_decodable(steps, script, wbits, only_end=True)
    ends = 0
    for i, s in enumerate(steps):
        if s.op != "write":
            continue
        rcs = [c[0] for c in s.calls]
        assert set(rcs) <= {OK, NEED_BUFFERS, END_OF_STREAM}, (i, rcs)
        assert all(c[1] <= k for c in s.calls), i
        later = [sum(c[1] for c in s.calls[j + 1:]) for j in range(len(s.calls))]
        if s.flush != "finish":
            assert END_OF_STREAM not in rcs, i
            if strict and k < 7 and s.flush != "none":
                for j, (rc, _, avail_out, pend) in enumerate(s.calls):
                    assert rc != OK or pend[0] == later[j], (i, j, pend, later[j])
            continue
        ends += rcs.count(END_OF_STREAM)
        assert rcs[-1] == END_OF_STREAM and rcs.count(END_OF_STREAM) == 1, (i, rcs)
        for j, (rc, _, avail_out, pend) in enumerate(s.calls[:-1]):
            assert rc == OK and avail_out == 0, (i, j, rc, avail_out)
            if strict or finish_drains(s, j):
                assert pend[0] > 0 or j == len(s.calls) - 2, (i, j, pend)
                assert later[j] == pend[0], (i, j, pend, later[j])
        if strict:
            assert s.calls[-1][3][0] == 0, (i, s.calls[-1])
    assert ends == 1


def finish_drains(s, j):
    """The finish call j of step s left only pending bytes behind: every
    later call hands out min(room, pending before it) and nothing is added.
    (On the reference a finish can also return ok with no room left in the
    middle of its parse -- finish_started / need_more, deflate_stream.ipp:446-452 --
    with more blocks still to come; P then says nothing about them.  The
    per-stream GPU deflater compresses everything in the first call, so there
    every ok return is of this kind.)"""
    p = s.calls[j][3][0]
    for rc, n, _, pend in s.calls[j + 1:]:
        if n > p or pend[0] != p - n:
            return False
        p = pend[0]
    return True


# -------------------------------------------------------------------- configs

LEVELS = (0, 1, 3, 4, 6, 9)
WBITS = (9, 10, 15)


def config(level, wbits, strategy=0, n=0):
    """create()'s arguments; memLevel alternates 1 / 8 / 9 (on the GPU it is
    only validated).  Level 0 with Strategy::rle never gets memLevel 1: the
    reference's deflate_rle then closes a block every 127 symbols, level 0
    forces it stored, and up to 127 x 258 bytes go into a pending buffer of
    512 -- the oracle backend, which restates that code, corrupts its heap.
    (Strategy::huffman closes blocks of 127 literals, which fit.)"""
    mem = (1, 8, 9)[(level + wbits + strategy + n) % 3]
    return dict(level=level, wbits=wbits, mem=8 if level == 0 and strategy == 3 and mem == 1 else mem,
                strategy=strategy)


# ------------------------------------------------------------------- segments

LENGTHS = (0, 1, 2, 3, 258, 259, 4095, 4096, 4097, 8193, 20000)
KINDS = ("json", "corpus1", "random", "binary", "zeros")
PERIODS = (251, 300, 700, 2047, 2048, 2049, 4095, 4096, 4097, 5000)


@functools.lru_cache(maxsize=None)
def segment(kind, n, seed=0):
    if n == 0:
        return b""
    d, _, _ = synth.make_batch(kind, [n], seed=0x5C217 + 977 * seed + n)
    return bytes(d[:n])


@functools.lru_cache(maxsize=None)
def periodic(period, n, seed=0):
    """A JSON-like block tiled with the given period: the cheapest match of
    every position past the first block is at distance exactly `period`."""
    base = bytearray(segment("json", period, seed + 11))
    # no shorter period: a counter in every 64 bytes of the block
    for i in range(0, period - 4, 64):
        base[i:i + 4] = b"%04d" % (i // 64 + 1)
    return (bytes(base) * (n // period + 1))[:n]


def pool(seed):
    """11 segments: every length of LENGTHS once, kinds rotating with the seed."""
    return [segment(KINDS[(i + seed) % 5], n, seed) for i, n in enumerate(LENGTHS)]


# -------------------------------------------------------------------- scripts

def repeating(flush, seed):
    """Up to 15 flushes of one kind and a finish: the pool's segments in an
    order that depends on the seed, one of them fed by two Flush::none
    writes first, an empty write (a duplicate flush: need_buffers) and an
    empty finish (end_of_stream again) included."""
    segs = pool(seed)
    order = [(3 * i + seed) % len(segs) for i in range(len(segs))]
    script = []
    for n, j in enumerate(order[:-1]):
        s = segs[j]
        if n == 2 and len(s) > 2:
            script += [("write", s[:len(s) // 3], "none"), ("write", s[len(s) // 3:len(s) // 3 + 1], "none")]
            s = s[len(s) // 3 + 1:]
        script.append(("write", s, flush))
        if n == 4:
            script.append(("write", b"", flush))
    script.append(("write", segs[order[-1]], "finish"))
    script.append(("write", b"", "finish"))
    return script


def mixed(seed):
    """Every flush kind in one stream, then what the reference's own test
    asks after finish (test/beast/zlib/deflate_stream.cpp:472-496): another
    finish is end_of_stream, any other flush stream_error, more input
    need_buffers."""
    segs = pool(seed + 1)
    kinds = ("sync", "none", "partial", "block", "full", "trees", "none", "sync", "block", "partial", "trees")
    script = [("write", segs[(5 * i + seed) % len(segs)], f) for i, f in enumerate(kinds)]
    script += [("pending",), ("write", b"", "sync"), ("write", segs[4], "finish"), ("pending",),
               ("write", b"", "finish"), ("write", b"", "sync"), ("write", b"x", "finish"), ("write", b"x", "none")]
    return script


def full_restart(seed, n=1500):
    """The same compressible segment written twice with Flush::full, a third
    one, then finish (check D and its non-vacuity half)."""
    s = segment("json", n, seed + 3)
    return [("write", s, "full"), ("write", s, "full"), ("write", segment("corpus1", 700, seed), "full"),
            ("write", s[:n // 2], "finish")]


def history_window(period, flush="sync", n=6000, parts=3):
    """A periodic text in `parts` writes, cut at places that are no multiple
    of the period, with `flush` between them: the matches of every write
    after the first start in the history."""
    data = periodic(period, n)
    cuts = [0] + [n * (i + 1) // parts + 17 * (i + 1) for i in range(parts - 1)] + [n]
    script = [("write", data[a:b], flush) for a, b in zip(cuts, cuts[1:])]
    return script + [("write", b"", "finish")]


def split_pattern(data, i):
    """The reference harness's split: Flush::none with the first i bytes,
    Flush::full with the rest (run with room ("split", j)), then finish."""
    return [("write", data[:i], "none"), ("write", data[i:], "full"), ("write", b"", "finish")]


HELLO = b"Hello, world!"


def corpus56():
    return segment("corpus1", 56, 5)


def params_script(seed, buffered):
    """Level 6 -> 0 -> 9 -> 1 and strategy normal -> huffman -> rle -> fixed ->
    normal between segments, with input buffered by a Flush::none write at
    each switch or not; an invalid level in the middle."""
    segs = [segment("json", 3000, seed), segment("corpus1", 4097, seed), segment("json", 2500, seed + 1),
            segment("binary", 1000, seed), segment("json", 5000, seed + 2)]
    script = [("write", segs[0], "sync")]
    for k, (lvl, strat) in enumerate([(0, 0), (9, 2), (1, 3), (1, 4), (6, 0)]):
        s = segs[k % len(segs)]
        if buffered:
            script.append(("write", s[:len(s) // 2], "none"))
            s = s[len(s) // 2:]
        # the first buffered switch gets no room for output: doParams' doWrite is need_buffers,
        # cleared as nothing is pending (deflate_stream.ipp:339), and the level changes with the
        # input still inside, which the next flush then compresses at level 0
        script.append(("params", lvl, strat, 0) if buffered and k == 0 else ("params", lvl, strat))
        if k == 2:
            script.append(("params", 10, 0))
            script.append(("params", -2, 0))
        if k == 0 and not buffered:
            # doParams' own doWrite(Flush::block) (deflate_stream.ipp:334-341) is the
            # previous flush now: a sync without input is no duplicate of the one before
            script.append(("write", b"", "sync"))
        script.append(("write", s, ("sync", "partial", "full", "block", "sync")[k]))
    script.append(("write", segs[1][:800], "finish"))
    return script


def level0_cost(steps, script):
    """[(bytes produced, bytes written)] of the flushed writes made at level 0."""
    level, res = None, []
    for st, s in zip(script, steps):
        if st[0] == "params" and s.rc == OK:
            level = st[1]
        elif st[0] == "write" and st[2] != "none" and level == 0 and s.rc == OK:
            res.append((len(s.out), len(s.data)))
    return res


# prime() inserts bits that the inflater will read as part of the stream, so
# the scripts prime whole empty blocks, in pieces of every bit count the
# issue asks for (0, 1, 5, 8, 13, 16):
#   static   one empty static block (BFINAL 0, BTYPE 01, end-of-block 0000000): 10 bits, value 2
#   static3  three of them, 30 bits, as 1 + 13 + 16
#   stored   an empty stored block from a byte boundary: 00 | 00 00 | FF FF as 8 + 16 + 16
_S3 = 2 | 2 << 10 | 2 << 20
PRIMES = {
    "none": [(0, 0)],
    "static": [(5, 2), (5, 0)],
    "static3": [(1, _S3 & 1), (13, (_S3 >> 1) & 0x1FFF), (16, _S3 >> 14)],
    "stored": [(8, 0), (16, 0), (16, 0xFFFF)],
}


def prime_script(kind, seed, between):
    """prime() before the first write and, with `between`, after the first
    and second flush too: the static blocks at any bit position (after partial
    and block), the stored one only from a byte boundary (after sync and
    full).  The second segment is two chunks, the third does not compress."""
    primes = [("prime", bits, value) for bits, value in PRIMES[kind]] + [("pending",)]
    a, b, c = segment("json", 2000, seed), segment("json", 4097, seed + 1), segment("random", 900, seed)
    f1, f2 = ("sync", "full") if kind == "stored" else ("partial", "block")
    script = primes + [("write", a, f1)]
    if between:
        script += primes
    script += [("write", b, f2)]
    if between:
        script += primes
    return script + [("write", c, "sync"), ("write", a[:500], "finish")]


def prime_only():
    """pending() after prime alone; on the reference (0, 5), (2, 2), (4, 2)."""
    return [("prime", 5, 0x15), ("prime", 13, 0x1ABC), ("prime", 16, 0xBEEF), ("pending",)]


def tight_scripts(seed):
    """A subset of the flush matrix for small rooms: one script per flush
    kind and a mixed one, segments of at most 4097 bytes."""
    lens = (700, 0, 1, 259, 4097, 3)
    segs = [segment(KINDS[(i + seed) % 5], n, seed) for i, n in enumerate(lens)]
    scripts = []
    for flush in ("partial", "sync", "full", "trees", "block"):
        scripts.append([("write", s, flush) for s in segs] + [("write", segs[0][:300], "finish")])
    kinds = ("none", "sync", "partial", "block", "full", "trees")
    scripts.append([("write", s, f) for s, f in zip(segs, kinds)] + [("write", b"", "finish")])
    return scripts


def check_tune(L, runner, level=6):
    """tune(): runner(script, **cfg) runs a script and returns its Steps
    (after whatever checks the caller makes of every run).  Rows of the
    reference's level table only."""
    own, low, high = LEVEL_ROWS[level], LEVEL_ROWS[1], LEVEL_ROWS[9]
    a, b = segment("json", 20000, 41), segment("json", 8193, 42)
    cfg = dict(level=level, wbits=15, mem=8, strategy=0)
    plain = output(runner([("write", a, "sync"), ("write", b, "finish")], **cfg))
    # a. before the first write: undone by the lazy init (deflate_stream.ipp:688, 697-710)
    assert output(runner([("tune",) + low, ("write", a, "sync"), ("write", b, "finish")], **cfg)) == plain
    # b. the level's own row after the first write: the same bytes
    assert output(runner([("write", a, "sync"), ("tune",) + own, ("write", b, "finish")], **cfg)) == plain
    # c. the level-1 and level-9 rows: still decodable (the runner's check B), the level-1 row no smaller
    t1 = output(runner([("write", a, "sync"), ("tune",) + low, ("write", b, "sync"), ("write", a, "finish")], **cfg))
    t9 = output(runner([("write", a, "sync"), ("tune",) + high, ("write", b, "sync"), ("write", a, "finish")], **cfg))
    t0 = output(runner([("write", a, "sync"), ("write", b, "sync"), ("write", a, "finish")], **cfg))
    assert len(t1) >= len(t9), (len(t1), len(t9))
    assert t1 != t0, "tune() to another row changed nothing"
    # d. params() to another level reloads that level's row (deflate_stream.ipp:342-349)
    other = 4 if level != 4 else 5
    tuned = runner([("write", a, "sync"), ("tune",) + low, ("params", other, 0), ("write", b, "finish")], **cfg)
    never = runner([("write", a, "sync"), ("params", other, 0), ("write", b, "finish")], **cfg)
    assert output(tuned) == output(never)
    # e. reset() drops it
    again = runner([("write", a, "sync"), ("tune",) + low, ("reset",), ("write", b, "finish")], **cfg)
    assert again[-1].out == output(runner([("write", b, "finish")], **cfg))
    # f. prime() initialises the stream (deflate_stream.ipp:556-580 via maybe_init), so a tune after it is kept
    # (the primed bits are the empty stored block that a first write(Flush::sync) emits)
    primes = [("prime", bits, value) for bits, value in PRIMES["stored"]]
    kept = output(runner(primes + [("tune",) + low, ("write", a, "finish")], **cfg))
    untuned = output(runner(primes + [("write", a, "finish")], **cfg))
    late = output(runner([("write", b"", "sync"), ("tune",) + low, ("write", a, "finish")], **cfg))
    assert kept != untuned, "a tune() after prime() was dropped"
    assert kept == late, "the tune kept after prime() is not the one set"
