"""Shared driver and cases for the per-stream inflater (zlib::inflate_stream
behind bpmd_inflate_stream_*): every write() is compared with the oracle's
restatement of Beast's inflate_stream (oracle/bzo_inflate.c =
inflate_stream.ipp:74-535 + bitstream.hpp + window.hpp) field by field --
status, next_in / avail_in / total_in, next_out / avail_out / total_out,
data_type, and the bytes in the caller's buffer (also after an error, which
returns without advancing z_params, inflate_stream.ipp:120-125).

Used by tests/test_gpu_zstream.py (the kernel, through the C ABI, a launch
per call), tests/test_gpu_stream_batch.py (calls sharing a launch: plans of a
fixed call count run in lockstep, run_lockstep), tests/test_gpu_zstream_guard.py
(the kernels launched directly, inside guarded rooms) and
tests/test_zstream_host.py (the kernel's own source built for the host,
behind the library's own call protocol)."""
import ctypes
import json
import os
import random

from beast_amd import synth
from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE, BLOCK, PARTIAL, SYNC, FULL, FINISH, TREES = range(7)
FLUSH_NAMES = {NONE: "none", BLOCK: "block", PARTIAL: "partial", SYNC: "sync", FULL: "full", FINISH: "finish",
               TREES: "trees"}
EB = b"\x00\x00\xff\xff"


class ZParams(ctypes.Structure):
    _fields_ = [("next_in", ctypes.c_void_p), ("avail_in", ctypes.c_size_t), ("total_in", ctypes.c_size_t),
                ("next_out", ctypes.c_void_p), ("avail_out", ctypes.c_size_t), ("total_out", ctypes.c_size_t),
                ("data_type", ctypes.c_int)]


class OracleInflater:
    def __init__(self, wbits=15):
        self.z = O.Inflater(wbits)

    def write(self, zs, flush):
        return self.z.write(zs, FLUSH_NAMES[flush])


def drive(inf, stream: bytes, calls, stop=True, before=None):
    """calls: [(cut, avail_out, flush)].  Each call offers input from where
    the inflater's next_in stands to max(cut, that).  Returns one record per
    call: (status, total_in, avail_in, total_out, avail_out, data_type,
    in position, out position, the whole output buffer).  stop=True ends
    after the first error or end_of_stream; stop=False makes every call in the
    list whatever the status (a connection that keeps calling an inflater in
    BAD or DONE mode).  before(), if given, runs ahead of every write()."""
    src = ctypes.create_string_buffer(stream, max(1, len(stream)))
    base = ctypes.addressof(src)
    pos = 0
    recs = []
    for cut, room, flush in calls:
        cut = max(cut, pos)
        buf = ctypes.create_string_buffer(max(1, room))
        zs = ZParams(base + pos if cut > pos else None, cut - pos, 0, ctypes.addressof(buf), room, 0, 12345)
        if before:
            before()
        st = inf.write(zs, flush)
        assert st >= 0, f"C ABI error {st}"
        in_at = (zs.next_in - base) if zs.next_in else pos
        out_at = (zs.next_out - ctypes.addressof(buf)) if zs.next_out else 0
        recs.append((st, zs.total_in, zs.avail_in, zs.total_out, zs.avail_out, zs.data_type, in_at, out_at,
                     buf.raw))
        pos += zs.total_in
        if stop and st >= 2:
            break
    return recs


FIELDS = ("status", "total_in", "avail_in", "total_out", "avail_out", "data_type", "next_in", "next_out", "bytes")


def assert_records_equal(got, want, calls, label=""):
    """Every call of `got` equal to the oracle's `want` over all of FIELDS."""
    for i in range(min(len(got), len(want))):
        for f, a, b in zip(FIELDS, got[i], want[i]):
            assert a == b, (label, "call", i, f, a if f != "bytes" else len(a), b if f != "bytes" else len(b),
                            calls[i], O.ERRORS[got[i][0]], O.ERRORS[want[i][0]])
    assert len(got) == len(want), (label, len(got), len(want))


def compare(make, stream, calls, wbits=15, label="", stop=True):
    """make(wbits) -> inflater under test.  Asserts every call equal to the
    oracle's; returns the oracle's records.  stop: see drive()."""
    want = drive(OracleInflater(wbits), stream, calls, stop=stop)
    inf = make(wbits)
    try:
        got = drive(inf, stream, calls, stop=stop)
    finally:
        close = getattr(inf, "close", None)
        if close:
            close()
    assert_records_equal(got, want, calls, label)
    return want


def calls_after(recs, pred):
    """How many of the records follow the first one whose status satisfies
    pred (the calls a connection made to an inflater already in that state)."""
    for i, r in enumerate(recs):
        if pred(r[0]):
            return len(recs) - i - 1
    return 0


def is_error(st):
    return st > 2   # zlib::error: 1 need_buffers and 2 end_of_stream are not failures


def connection_stream(msgs, level=6, wbits=15, mem=4, takeover=True):
    """What one connection's inflater receives: each payload followed by the
    00 00 FF FF that inflate_with_eb feeds (impl_base.hpp:179-190)."""
    if takeover:
        pays = O.pmd_deflate_stream(msgs, level, wbits, mem)
    else:
        pays = [O.pmd_deflate(m, level, wbits, mem) for m in msgs]
    return b"".join(p + EB for p in pays)


def msgs_of(kind, sizes, seed):
    data, off, lens = synth.make_batch(kind, sizes, seed=seed)
    return [bytes(data[int(off[i]):int(off[i]) + int(lens[i])]) for i in range(len(sizes))]


def random_calls(rng, total, n_calls, rooms, flushes=(SYNC,)):
    cuts = sorted(rng.randrange(0, total + 1) for _ in range(n_calls - 1)) + [total]
    calls = [(c, rng.choice(rooms), rng.choice(flushes)) for c in cuts]
    # drain: keep calling with everything offered until nothing more comes out
    calls += [(total, 1 << 16, SYNC)] * 8
    return calls


def kat_vectors():
    with open(os.path.join(GOLD, "inflate_kat.json")) as f:
        return json.load(f)


# ------------------------------------------------------- websocket read path

class WsReader:
    """websocket::stream's sync read_some inflate branch
    (read.hpp:1284-1385) over one inflater: rd_buf filled from the socket up
    to its capacity, avail_in clamped to the frame's rd_remain, rd_buf and
    rd_remain advanced by exactly total_in, then inflate_with_eb
    (impl_base.hpp:179-190) with rd_eb_consumed until a call produces
    nothing; any error stops the read (check_stop_now).  Messages are given
    as their frames' payloads (headers parsed elsewhere)."""

    def __init__(self, inf, rd_buf_cap=1536):
        self.inf = inf
        self.cap = rd_buf_cap
        self.calls = []   # (status, total_in, total_out, data_type) of every write()

    def begin(self, frames):
        self.frames = list(frames)
        self.sock = bytearray()
        self.rd_buf = bytearray()
        self.rd_remain = 0
        self.fin = False
        self.rd_eb_consumed = 0   # rd_deflated(rsv1), impl_base.hpp:68-77
        self.rd_done = False
        for p in self.frames:
            self.sock += p
        self._next_frame()

    def _next_frame(self):
        p = self.frames.pop(0)
        self.rd_remain = len(p)
        self.fin = not self.frames

    def _write(self, data: bytes, room: int):
        src = ctypes.create_string_buffer(data, max(1, len(data)))
        buf = ctypes.create_string_buffer(max(1, room))
        zs = ZParams(ctypes.addressof(src) if data else None, len(data), 0, ctypes.addressof(buf), room, 0, 0)
        st = self.inf.write(zs, SYNC)
        self.calls.append((st, zs.total_in, zs.total_out, zs.data_type))
        return st, zs, buf.raw[:zs.total_out]

    def read_some(self, size):
        """One read_some into a `size`-byte buffer: (bytes, status)."""
        while self.rd_remain == 0 and not self.fin:
            self._next_frame()
        out = bytearray()
        did_read = False
        room = size
        while room > 0:
            if self.rd_remain > 0:
                if self.rd_buf:
                    data = bytes(self.rd_buf[:min(self.rd_remain, len(self.rd_buf))])
                elif not did_read:
                    k = min(self.cap - len(self.rd_buf), len(self.sock))
                    self.rd_buf += self.sock[:k]
                    del self.sock[:k]
                    data = bytes(self.rd_buf[:min(self.rd_remain, len(self.rd_buf))])
                    did_read = True
                else:
                    break
                st, zs, got = self._write(data, room)
                if st:
                    return bytes(out), st
                self.rd_remain -= zs.total_in
                del self.rd_buf[:zs.total_in]
            elif self.fin:
                st, zs, got = self._write(EB[self.rd_eb_consumed:], room)
                self.rd_eb_consumed += zs.total_in
                assert self.rd_eb_consumed <= 4
                if st == 1:   # need_buffers cleared
                    st = 0
                if st:
                    return bytes(out), st
                if zs.total_out == 0:
                    self.rd_done = True
                    break
            else:
                break
            out += got
            room -= zs.total_out
        return bytes(out), 0

    def read_message(self, frames, size):
        """do { read_some(size) } while (!is_message_done()) -- the shape of
        read3.cpp:1190-1200; returns (bytes, first error or 0)."""
        self.begin(frames)
        msg = bytearray()
        while True:
            got, st = self.read_some(size)
            msg += got
            if st:
                return bytes(msg), st
            if self.rd_done:
                return bytes(msg), 0


def ws_replay(make, messages, size, rd_buf_cap=1536, wbits=15):
    """Reads every message (a list of frame payloads) through WsReader on the
    inflater under test and on the oracle; asserts the same bytes, errors
    and per-write() z_params; returns the oracle side's messages."""
    a = WsReader(make(wbits), rd_buf_cap)
    b = WsReader(OracleInflater(wbits), rd_buf_cap)
    res = []
    try:
        for i, frames in enumerate(messages):
            ga = a.read_message(frames, size)
            gb = b.read_message(frames, size)
            assert ga == gb, (i, len(ga[0]), ga[1], len(gb[0]), gb[1])
            if a.calls != b.calls:
                k = next((k for k, (x, y) in enumerate(zip(a.calls, b.calls)) if x != y), None)
                raise AssertionError(("message", i, "write", k, a.calls[k] if k is not None else len(a.calls),
                                      b.calls[k] if k is not None else len(b.calls)))
            res.append(gb)
    finally:
        close = getattr(a.inf, "close", None)
        if close:
            close()
    return res


# ------------------------------------------------------------------- cases

def case_connection_random_cuts(make, kind, level, mem):
    rng = random.Random(f"{kind}{level}{mem}")
    msgs = msgs_of(kind, [rng.choice([0, 1, 100, 1024, 4096, 9000]) for _ in range(12)], seed=level * 10 + mem)
    stream = connection_stream(msgs, level=level, mem=mem)
    for trial in range(3):
        calls = random_calls(rng, len(stream), rng.choice([3, 20, 80]), [4096, 1 << 16, 300, 7, 1, 258, 257])
        compare(make, stream, calls, label=f"{kind} L{level} m{mem} t{trial}")


def case_foreign_payloads(make):
    """A connection whose peer is another encoder (CPython's zlib, no context
    takeover): payloads with mid-message none / block / sync / full flushes and
    zlib's strategies (tests/foreign.py), each followed by 00 00 FF FF, under
    random cuts and output rooms."""
    from tests.foreign import foreign_payloads
    rng = random.Random("foreign")
    pays, _, _ = foreign_payloads(21, 24)
    stream = b"".join(p + EB for p in pays)
    for trial in range(3):
        calls = random_calls(rng, len(stream), rng.choice([5, 40, 160]), [4096, 1 << 16, 300, 7, 1, 258])
        compare(make, stream, calls, label=f"foreign t{trial}")


def case_output_room_one_byte(make, n_calls=3000):
    # memLevel 9: blocks of up to 32 Ki symbols; output handed out a byte at a time
    msgs = msgs_of("corpus1", [20000], seed=5)
    stream = connection_stream(msgs, level=9, mem=9)
    calls = [(len(stream), 1, SYNC)] * n_calls + [(len(stream), 1 << 16, SYNC)] * 4
    compare(make, stream, calls, label="room 1")


def case_byte_at_a_time_input(make):
    msgs = msgs_of("json", [3000, 20], seed=6)
    stream = connection_stream(msgs, level=6, mem=4)
    calls = [(k, 1 << 16, SYNC) for k in range(1, len(stream) + 1)] + [(len(stream), 1 << 16, SYNC)] * 3
    compare(make, stream, calls, label="input 1")


def case_flush_mix(make):
    rng = random.Random(11)
    msgs = msgs_of("json", [3000, 50, 8000, 0, 700], seed=3)
    stream = connection_stream(msgs, level=6, mem=4)
    for trial in range(4):
        calls = random_calls(rng, len(stream), 40, [1 << 16, 500, 3],
                             flushes=(SYNC, BLOCK, TREES, NONE, FINISH, PARTIAL, FULL))
        compare(make, stream, calls, label=f"flush mix {trial}")


def case_flush_trees_kat(make):
    k = kat_vectors()["flush_trees"]
    for name in ("fixed", "stored"):
        stream = bytes.fromhex(k[name])
        want = compare(make, stream, [(len(stream), 5, TREES), (len(stream), 5, SYNC)], label=name)
        assert want[1][8][:want[1][3]] == bytes.fromhex(k["expect_out"])


def case_kat_split(make, every_cut=True):
    for v in kat_vectors()["vectors"]:
        d = bytes.fromhex(v["in"])
        if "prefix" in v:
            d = d[:v["prefix"]]
        w = v.get("wbits", 15)
        whole = compare(make, d, [(len(d), 1024, SYNC), (len(d), 1024, SYNC)], wbits=w, label=v["in"][:16])
        assert O.ERRORS[whole[0][0]] == v["expect"]
        cuts = range(1, len(d)) if every_cut else range(1, len(d), max(1, len(d) // 8))
        for cut in cuts:
            compare(make, d, [(cut, 1024, SYNC), (len(d), 1024, SYNC), (len(d), 1024, SYNC)], wbits=w,
                    label=f"{v['in'][:16]}@{cut}")


def case_small_window(make):
    """Stream compressed with a 32 KiB window, inflated with windowBits 9..12:
    whether a long distance is invalid depends on where the calls split."""
    rng = random.Random(7)
    msgs = msgs_of("corpus1", [6000, 6000], seed=9)
    stream = connection_stream(msgs, level=9, wbits=15, mem=8)
    seen_err = False
    for w in (9, 10, 12):
        for trial in range(6):
            calls = random_calls(rng, len(stream), rng.choice([2, 10, 40]), [1 << 16, 2000, 64])
            want = compare(make, stream, calls, wbits=w, label=f"w{w} t{trial}")
            seen_err |= any(r[0] == O.ERROR_CODES["invalid_distance"] for r in want)
    assert seen_err   # the rule was exercised


def case_end_of_stream(make):
    import zlib
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    stream = c.compress(b"hello world " * 300) + c.flush(zlib.Z_FINISH) + b"trailing garbage"
    eos = O.ERROR_CODES["end_of_stream"]
    for cuts in ([len(stream)], [10, 40, len(stream)], list(range(1, len(stream) + 1, 3))):
        calls = [(x, 1 << 16, SYNC) for x in cuts] + [(len(stream), 1 << 16, SYNC)] * 3
        want = compare(make, stream, calls, label=f"eos {len(cuts)}")
        assert want[-1][0] == eos
        # the connection keeps calling: DONE mode answers end_of_stream again,
        # with the trailing bytes offered and with every flush
        more = calls + [(len(stream), room, fl) for room in (1 << 16, 1, 0) for fl in (SYNC, FINISH, BLOCK, TREES)]
        want = compare(make, stream, more, label=f"eos {len(cuts)} then DONE", stop=False)
        assert len(want) == len(more) and calls_after(want, lambda st: st == eos) >= 12
        assert all(r[0] == eos for r in want[-12:])


def case_stored_blocks(make):
    rng = random.Random(12)
    msgs = msgs_of("random", [70000, 5, 3000], seed=12)
    stream = connection_stream(msgs, level=0, mem=4)   # stored blocks
    for trial in range(4):
        calls = random_calls(rng, len(stream), rng.choice([3, 30]), [1 << 17, 4000, 1, 70000],
                             flushes=(SYNC, TREES, BLOCK))
        compare(make, stream, calls, label=f"stored {trial}")


def case_errors(make):
    rng = random.Random(3)
    msgs = msgs_of("json", [4096] * 4, seed=4)
    good = bytearray(connection_stream(msgs, level=6, mem=4))
    after = 0
    for trial in range(12):
        bad = bytearray(good)
        at = rng.randrange(len(bad) // 3, len(bad))
        bad[at] ^= 1 << rng.randrange(8)
        calls = random_calls(rng, len(bad), rng.choice([1, 5, 30]), [4096, 1 << 16, 100])
        calls += [(len(bad), 1 << 16, SYNC)] * 2
        compare(make, bytes(bad), calls, label=f"corrupt {trial}@{at}")
        # the connection keeps calling the dead inflater: every call of the
        # list is made, BAD mode's answers included
        want = compare(make, bytes(bad), calls, label=f"corrupt {trial}@{at} then BAD", stop=False)
        assert len(want) == len(calls)
        after += calls_after(want, is_error)
    # most single-bit flips of this stream still decode (the oracle reports no
    # error for any of the twelve above): flips the oracle does fail on
    for trial, bad in enumerate(failing_flips(good, rng, 8)):
        calls = random_calls(rng, len(bad), rng.choice([1, 5, 30]), [4096, 1 << 16, 100])
        compare(make, bad, calls, label=f"failing {trial}")
        want = compare(make, bad, calls, label=f"failing {trial} then BAD", stop=False)
        assert len(want) == len(calls) and calls_after(want, is_error) >= 1, trial
        after += calls_after(want, is_error)
    assert after >= 8   # calls made after an error were compared


def case_reset_between_streams(make):
    """reset(windowBits) mid-stream: fresh state and window, new size.  A
    clear() in the middle of the second stream (doClear is empty,
    inflate_stream.ipp:49-53) changes nothing in the calls that follow: the
    oracle's side runs without it."""
    msgs = msgs_of("json", [5000, 5000], seed=31)
    s1 = connection_stream(msgs[:1], level=6, mem=4)
    s2 = connection_stream(msgs[1:], level=6, wbits=10, mem=4)
    g = make(15)
    o = OracleInflater(15)
    try:
        drive(g, s1, [(len(s1) // 2, 1 << 16, SYNC)])
        drive(o, s1, [(len(s1) // 2, 1 << 16, SYNC)])
        g.reset(10)
        o.z.reset(10)
        calls = [(len(s2) // 3, 100, SYNC), (len(s2), 1 << 16, SYNC), (len(s2), 1 << 16, SYNC)]
        writes = []

        def clear_before_the_second():
            writes.append(0)
            if len(writes) == 2:
                g.clear()

        assert drive(g, s2, calls, before=clear_before_the_second) == drive(o, s2, calls)
        assert len(writes) >= 2
    finally:
        g.close()


def case_output_over_four_mib(make):
    """5 MiB of zeros (about 5 KiB deflated) written in one call into a room
    of 5 MiB + 4096, so the room handed to the decoder is over 4 MiB; then a
    600-byte message of the same connection into a room of 1 KiB."""
    msgs = [bytes(5 << 20), msgs_of("json", [600], seed=51)[0]]
    pays = O.pmd_deflate_stream(msgs, 6, 15, 4)
    stream = b"".join(p + EB for p in pays)
    n, room = len(pays[0]) + 4, (5 << 20) + 4096
    assert min(room, 1040 * n + 8192) > 4 << 20
    want = compare(make, stream, [(n, room, SYNC), (len(stream), 1024, SYNC)], label="5 MiB of zeros")
    assert [(r[0], r[1], r[3]) for r in want] == [(0, n, 5 << 20), (0, len(stream) - n, 600)]
    assert want[0][8][:5 << 20] == msgs[0] and want[1][8][:600] == msgs[1]


R_INVALID_ARGUMENT, R_DOMAIN_ERROR, STREAM_ERROR = -1, -2, 4   # include/beast_pmd.h


def case_argument_checks(make):
    """The call protocol's argument checks (beast_amd/csrc/inflate_reader.h),
    through the C ABI of the inflater's library (inf.L, inf.h): windowBits 7
    and 16 at create and at reset are BPMD_R_DOMAIN_ERROR, flush -1 and 7
    BPMD_R_INVALID_ARGUMENT, a null next_in with avail_in 1 and a null
    next_out with avail_out 1 BPMD_STREAM_ERROR.  Each refused write leaves
    every z_params field as it was.  Each of them is made before every
    write() of a stream -- on the fresh inflater and in mid-stream -- and
    every write() still equals the oracle's, which never saw them: a known
    answer, and a connection whose second message needs the first one's
    window (a reset that took effect would lose it)."""
    src = ctypes.create_string_buffer(b"\x00" * 16)
    dst = ctypes.create_string_buffer(16)

    def fields(zs):
        return tuple(getattr(zs, f) for f, _ in ZParams._fields_)

    def refused(inf, want, flush, next_in, avail_in, next_out, avail_out):
        zs = ZParams(next_in, avail_in, 11, next_out, avail_out, 22, 12345)
        was = fields(zs)
        assert inf.L.bpmd_inflate_stream_write(inf.h, ctypes.byref(zs), flush) == want
        assert fields(zs) == was and dst.raw == bytes(16)

    def create(inf):
        for w in (7, 16):
            h = ctypes.c_void_p(1)
            assert inf.L.bpmd_inflate_stream_create(w, ctypes.byref(h)) == R_DOMAIN_ERROR and not h.value

    def reset(inf):
        for w in (7, 16):
            assert inf.L.bpmd_inflate_stream_reset(inf.h, w) == R_DOMAIN_ERROR

    def flush(inf):
        for fl in (-1, 7):
            refused(inf, R_INVALID_ARGUMENT, fl, ctypes.addressof(src), 16, ctypes.addressof(dst), 16)

    def null_in(inf):
        refused(inf, STREAM_ERROR, SYNC, None, 1, ctypes.addressof(dst), 16)

    def null_out(inf):
        refused(inf, STREAM_ERROR, SYNC, ctypes.addressof(src), 16, None, 1)

    kat = max((v for v in kat_vectors()["vectors"] if v["expect"] == "ok"), key=lambda v: len(v["in"]))
    k = bytes.fromhex(kat["in"])
    conn = connection_stream(msgs_of("json", [3000, 3000], seed=41), level=6, mem=4)
    streams = [("kat", k, kat.get("wbits", 15), [(len(k) // 2, 1024, SYNC), (len(k), 1024, SYNC), (len(k), 1024, SYNC)]),
               ("connection", conn, 15, [(len(conn) // 3, 1 << 16, SYNC), (2 * len(conn) // 3, 100, SYNC),
                                         (len(conn), 1 << 16, SYNC), (len(conn), 1 << 16, SYNC)])]
    for name, stream, wbits, calls in streams:
        want = drive(OracleInflater(wbits), stream, calls)
        assert len(want) == len(calls) and not any(is_error(r[0]) for r in want)
        for bad in (create, reset, flush, null_in, null_out):
            inf = make(wbits)
            try:
                got = drive(inf, stream, calls, before=lambda: bad(inf))
            finally:
                inf.close()
            assert_records_equal(got, want, calls, label=f"{name} after {bad.__name__}")


def failing_flips(good, rng, count, before=None):
    """`count` copies of the stream with one bit flipped (in its last two
    thirds, or before byte `before`) each of which the oracle's inflater fails
    on: drawn from rng until it does."""
    out = []
    while len(out) < count:
        bad = bytearray(good)
        at = rng.randrange(0, before) if before else rng.randrange(len(bad) // 3, len(bad))
        bad[at] ^= 1 << rng.randrange(8)
        recs = drive(OracleInflater(15), bytes(bad), [(len(bad), 1 << 20, SYNC)] * 2)
        if is_error(recs[-1][0]):
            out.append(bytes(bad))
    return out


def issue3028_message() -> bytes:
    with open(os.path.join(GOLD, "ws_issues.json")) as f:
        return bytes.fromhex(json.load(f)["issue3028"]["message_hex"])


def issue1630_frames():
    """[(opcode, payload)] of the four packets' frames, read3.cpp:619-1009."""
    with open(os.path.join(GOLD, "ws_issues.json")) as f:
        packets = [bytes.fromhex(p) for p in json.load(f)["issue1630"]["packets_hex"]]
    out = []
    for p in packets:
        i = 0
        while i < len(p):
            b0, b1 = p[i], p[i + 1]
            assert b0 & 0x80 and b0 & 0x40 and not b1 & 0x80   # FIN, RSV1 (compressed), unmasked
            n = b1 & 0x7f
            i += 2
            if n == 126:
                n = int.from_bytes(p[i:i + 2], "big")
                i += 2
            elif n == 127:
                n = int.from_bytes(p[i:i + 8], "big")
                i += 8
            out.append((b0 & 0x0f, p[i:i + n]))
            i += n
    return out


# ------------------------------------------------ plans of a fixed call count
# A plan is (stream bytes, windowBits, R calls): what one connection does in R
# rounds of a lockstep run (run_lockstep) or of a direct kernel launch
# (tests/test_gpu_zstream_guard.py).

ROOMS = [4096, 65536, 300, 7, 1, 258, 257, 255, 256]
ALL_FLUSHES = (NONE, BLOCK, PARTIAL, SYNC, FULL, FINISH, TREES)


def fixed_calls(stream, calls, R):
    """The call list cut to exactly R calls: truncated, or padded with drain
    calls that offer the whole stream."""
    calls = list(calls[:R])
    return calls + [(len(stream), 65536, SYNC)] * (R - len(calls))


def offering_calls(stream, wbits, R, offers, rooms, flush=SYNC):
    """R calls that offer exactly offers[i % len] new bytes with a room of
    rooms[i % len] each.  How far a call gets decides where the next one
    starts, so the cuts are taken from the oracle's inflater."""
    inf = OracleInflater(wbits)
    src = ctypes.create_string_buffer(stream, max(1, len(stream)))
    pos, calls = 0, []
    for i in range(R):
        n = min(offers[i % len(offers)], len(stream) - pos)
        room = rooms[i % len(rooms)]
        buf = ctypes.create_string_buffer(max(1, room))
        zs = ZParams(ctypes.addressof(src) + pos if n else None, n, 0, ctypes.addressof(buf), room, 0, 0)
        inf.write(zs, flush)
        calls.append((pos + n, room, flush))
        pos += zs.total_in
    return calls


_ORACLE = {}


def oracle_records(plan):
    """The oracle's records of every call of the plan (stop=False), computed
    once per plan and shared; nothing may change them."""
    stream, wbits, calls = plan
    key = (stream, wbits, tuple(calls))
    if key not in _ORACLE:
        _ORACLE[key] = drive(OracleInflater(wbits), stream, calls, stop=False)
    return _ORACLE[key]


_PLANS = {}


def mixed_plans(R, seed=0, rooms=ROOMS):
    """16 named plans of R calls each whose inflaters are, in any one round,
    in different phases: block headers, stored copies, the fast loop, pending
    matches and literals (rooms of 1 and 7), BAD and DONE.  [(name, plan)]."""
    key = (R, seed, tuple(rooms))
    if key in _PLANS:
        return _PLANS[key]
    import zlib
    from tests.foreign import foreign_payloads
    rng = random.Random(f"mixed {seed}")
    plans = []

    def add(name, stream, calls, wbits=15):
        plans.append((name, (bytes(stream), wbits, fixed_calls(stream, calls, R))))

    def cuts(stream, rooms_=rooms, flushes=(SYNC,)):
        return random_calls(rng, len(stream), max(1, R - 8), rooms_, flushes)

    sizes = [0, 1, 100, 1024, 4096, 9000]
    s = connection_stream(msgs_of("json", [rng.choice(sizes) for _ in range(12)], seed=61 + seed), level=6, mem=4)
    add("json L6 m4 takeover", s, cuts(s))
    s = connection_stream(msgs_of("binary", [rng.choice(sizes) for _ in range(12)], seed=62 + seed), level=1, mem=4)
    add("binary L1", s, cuts(s))
    s = connection_stream(msgs_of("random", [70000, 5, 3000], seed=63 + seed), level=0, mem=4)
    add("stored blocks", s, cuts(s, [1 << 17, 4000, 1, 70000] + list(rooms), (SYNC, TREES, BLOCK)))
    s = connection_stream(msgs_of("corpus1", [9000, 4096, 20000], seed=64 + seed), level=9, mem=9)
    add("corpus1 L9 m9", s, cuts(s))
    pays, _, _ = foreign_payloads(21 + seed, 12)
    s = b"".join(p + EB for p in pays)
    add("foreign encoders", s, cuts(s))
    w15 = connection_stream(msgs_of("corpus1", [6000, 6000], seed=9), level=9, wbits=15, mem=8)
    add("w15 stream at windowBits 9", w15, cuts(w15, [1 << 16, 2000, 64] + list(rooms)), wbits=9)
    add("w15 stream at windowBits 12", w15, cuts(w15, [1 << 16, 2000, 64] + list(rooms)), wbits=12)
    # bit flips the oracle fails on, in the first part of the stream so that
    # BAD mode comes part-way through the R calls and the calls go on
    good = connection_stream(msgs_of("json", [4096] * 4, seed=4), level=6, mem=4)
    for k, bad in enumerate(failing_flips(good, rng, 2, before=len(good) // 2)):
        add(f"bit flip {k}", bad, cuts(bad, [4096, 1 << 16, 100]))
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    s = c.compress(b"hello world " * 300) + c.flush(zlib.Z_FINISH) + b"trailing garbage"
    add("end of stream, trailing bytes", s, [(x, rng.choice(rooms), SYNC) for x in range(1, len(s) + 1, 3)])
    kat = max((bytes.fromhex(v["in"]) for v in kat_vectors()["vectors"] if v["expect"] == "ok"), key=len)
    add("KAT a byte at a time", kat, [(k, 1024, SYNC) for k in range(1, len(kat) + 1)])
    s = connection_stream(msgs_of("json", [3000, 50, 8000, 0, 700], seed=3), level=6, mem=4)
    cut = sorted(rng.randrange(0, len(s) + 1) for _ in range(R))
    add("every Flush value", s, [(cut[i], rng.choice([1 << 16, 500, 3]), ALL_FLUSHES[i % 7]) for i in range(R)])
    s = connection_stream(msgs_of("corpus1", [20000], seed=5), level=9, mem=9)
    add("room 1", s, [(len(s), 1, SYNC)] * R)
    # inflate_batch packs inputs at up256(n + 64) and outputs at up256(cap)
    s = connection_stream(msgs_of("json", [9000] * 6, seed=65 + seed), level=6, mem=4)
    add("packing edges", s, offering_calls(s, 15, R, [0, 1, 191, 192, 193], [255, 256, 257]))
    for k in range(16 - len(plans)):
        s = connection_stream(msgs_of("json", [rng.choice(sizes) for _ in range(12)], seed=70 + 7 * seed + k), level=6,
                              mem=4)
        add(f"json random cuts {k}", s, cuts(s))
    assert len(plans) == 16 and all(len(p[2]) == R for _, p in plans)
    # what the names promise, on the oracle's records
    recs = {name: oracle_records(p) for name, p in plans}
    for k in range(2):
        assert calls_after(recs[f"bit flip {k}"], is_error) >= R // 4, (k, [r[0] for r in recs[f"bit flip {k}"]])
    eos = O.ERROR_CODES["end_of_stream"]
    assert calls_after(recs["end of stream, trailing bytes"], lambda st: st == eos) >= R // 4
    edges = dict(plans)["packing edges"]
    offered = {(c[0] - (recs["packing edges"][i - 1][6] if i else 0), c[1]) for i, c in enumerate(edges[2])}
    assert offered >= {(n, room) for n in (0, 1, 191, 192, 193) for room in (255, 256, 257)}, sorted(offered)
    _PLANS[key] = plans
    return plans


def run_lockstep(make, plans, max_calls, L, timeout=60.0):
    """K connections in lockstep.  plans: K of (stream, windowBits, R calls).
    The oracle's records of every plan come first (main thread).  Then the
    batcher is set to max_calls with a 5 s delay -- a ceiling a leader waits
    out only when fewer than max_calls calls arrive -- and K threads each
    create their inflater (make(wbits)) and make their R calls, all meeting
    at a barrier before every call, so each round's K calls run as
    ceil(K / max_calls) full batches.  Workers record and never assert; an
    exception breaks the barrier for all.  Every call of every stream is then
    compared with the oracle over all of FIELDS.  L: the library
    (bpmd_stream_batching, bpmd_stream_batch_stats).  Returns the stats
    [inflate calls, inflate launches, deflate flushes, deflate launches]."""
    import threading
    K = len(plans)
    want = [oracle_records(p) for p in plans]
    bar = threading.Barrier(K)
    got, errs = [None] * K, []

    def work(i):
        stream, wbits, calls = plans[i]
        inf = None
        try:
            inf = make(wbits)
            got[i] = drive(inf, stream, calls, stop=False, before=lambda: bar.wait(timeout))
        except BaseException as e:   # noqa: BLE001 (reported after the join)
            errs.append((i, repr(e)))
            bar.abort()
        finally:
            close = getattr(inf, "close", None)
            if close:
                close()

    stats = (ctypes.c_ulonglong * 4)()
    assert L.bpmd_stream_batching(max_calls, 5_000_000) == 0
    try:
        assert L.bpmd_stream_batch_stats(stats, 1) == 0
        ts = [threading.Thread(target=work, args=(i,)) for i in range(K)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert L.bpmd_stream_batch_stats(stats, 1) == 0
    finally:
        L.bpmd_stream_batching(256, 0)
    assert not errs, errs
    for i in range(K):
        assert_records_equal(got[i], want[i], plans[i][2], label=f"stream {i}")
    return list(stats)
