"""GPU: the micro-batcher behind the per-stream calls (pmd_stream.hip; SURVEY
8(f) N2).  Concurrent write() calls of different streams run as one launch,
each with exactly its single-call result.  Python threads drive the C ABI
through ctypes (the GIL is released during each call), so their calls
overlap on the device.

* Free-running threads (batches as the timing makes them): every payload and
  round trip equals the same connections run one after another with the
  batcher off, and the oracle's inflater returns the messages from the
  batched payloads.
* Lockstep threads (tests/zstream_cases.py run_lockstep): K connections meet
  at a barrier before every call and the batcher waits for max_calls calls,
  so every launch holds exactly max_calls calls of known content.  Every
  write() of every inflater in such batches -- streams in header, stored,
  fast-loop, pending-match, BAD and DONE states side by side -- equals the
  oracle's call over all nine z_params fields and the output bytes, and the
  launch counts are exact.  The same for deflate flushes (byte-equal to the
  unbatched run, inflated by the oracle, one launch per parameter group).
* Both copy-back paths of inflate_batch and deflate_group: the single block
  copy and, past 4 MiB of room, results first and then each call's output."""
import ctypes
import threading

import pytest

from beast_amd import synth
from oracle import oracle as O
from tests import zstream_cases as Z
from tests.test_gpu_stream import SYNC, ZParams, _lib, ws_deflate_message, ws_inflate_message
from tests.test_gpu_zstream import GpuInflater

pytestmark = pytest.mark.gpu


def _api():
    L = _lib()
    L.bpmd_stream_batching.argtypes = [ctypes.c_int, ctypes.c_int]
    L.bpmd_stream_batch_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    L.bpmd_diag_set_zstream_parallel.argtypes = [ctypes.c_int]
    return L


def _stats(L):
    c = (ctypes.c_ulonglong * 4)()
    assert L.bpmd_stream_batch_stats(c, 1) == 0
    return list(c)


def _msgs(conn, n):
    sizes = [(conn * 7919 + k * 104729) % 30000 for k in range(n)]
    sizes[0] = [0, 1, 700, 4096, 4097][conn % 5]
    raw, off, ln = synth.make_batch("json", sizes, seed=0x5EED0600 + conn)
    return [bytes(raw[int(off[i]):int(off[i]) + int(ln[i])]) for i in range(n)]


def _connection(L, cfg, msgs):
    """One connection: its deflater (level, memLevel; never reset under
    context takeover, reset after each message otherwise) and inflater."""
    level, mem, takeover = cfg
    zo, zi = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.bpmd_deflate_stream_create(level, 15, mem, 0, ctypes.byref(zo)) == 0
    assert L.bpmd_inflate_stream_create(15, ctypes.byref(zi)) == 0
    pays, backs = [], []
    try:
        for m in msgs:
            p = ws_deflate_message(L, zo, m)
            if not takeover:
                assert L.bpmd_deflate_stream_reset(zo) == 0
            pays.append(p)
            backs.append(ws_inflate_message(L, zi, p))
    finally:
        L.bpmd_stream_destroy(zo)
        L.bpmd_stream_destroy(zi)
    return pays, backs


def _run(L, cfgs, msgs_of, threaded):
    res = [None] * len(cfgs)
    errs = []

    def work(i):
        try:
            res[i] = _connection(L, cfgs[i], msgs_of[i])
        except Exception as e:   # noqa: BLE001 (reported below)
            errs.append((i, repr(e)))

    if threaded:
        ts = [threading.Thread(target=work, args=(i,)) for i in range(len(cfgs))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    else:
        for i in range(len(cfgs)):
            work(i)
    assert not errs, errs
    return res


@pytest.mark.parametrize("max_calls,delay_us", [(256, 0), (8, 0), (64, 300)])
def test_batched_streams_equal_single_calls(max_calls, delay_us):
    """24 connections at three levels, two memLevels, with and without context
    takeover: every payload byte and every round trip of the concurrent,
    batched run equals the same connections run one by one unbatched (the
    deflate flushes of different parameters go to separate deflater calls of
    one batch), the oracle's inflater returns the messages from the batched
    payloads, and the batched run makes fewer launches than calls.  (How the
    calls group here is up to the threads' timing; the exact launch counts
    are the lockstep tests' below.)"""
    L = _api()
    cfgs = [((1, 6, 9)[i % 3], (4, 8)[(i // 3) % 2], i % 4 != 0) for i in range(24)]
    msgs_of = [_msgs(i, 4) for i in range(24)]
    try:
        assert L.bpmd_stream_batching(0, 0) == 0
        ref = _run(L, cfgs, msgs_of, threaded=False)
        assert L.bpmd_stream_batching(max_calls, delay_us) == 0
        _stats(L)
        got = _run(L, cfgs, msgs_of, threaded=True)
        ic, il, dc, dl = _stats(L)
    finally:
        L.bpmd_stream_batching(256, 0)
    for i in range(24):
        assert got[i][0] == ref[i][0], i
        assert got[i][1] == msgs_of[i] == ref[i][1], i
        # not only the code under test at both ends: the oracle's inflater
        if cfgs[i][2]:
            back = O.pmd_inflate_stream(got[i][0], cap=30000)
        else:
            back = [O.pmd_inflate(p, cap=30000) for p in got[i][0]]
        assert back == [(0, m) for m in msgs_of[i]], i
    assert ic > 0 and dc > 0 and il < ic and dl <= dc, (ic, il, dc, dl)


def test_batched_inflate_error_stays_with_its_stream():
    """16 inflaters called at once, every fourth fed a corrupt block (BTYPE 3):
    those calls return invalid_block_type without advancing z_params (the
    reference's err()), the others inflate their payloads exactly, in the
    same batches."""
    L = _api()
    zo = ctypes.c_void_p()
    assert L.bpmd_deflate_stream_create(6, 15, 4, 0, ctypes.byref(zo)) == 0
    msg = _msgs(3, 1)[0] or b"x" * 500
    good = ws_deflate_message(L, zo, msg)
    L.bpmd_stream_destroy(zo)
    bad = b"\x07" + b"\x00" * 63   # BFINAL 1, BTYPE 3
    out = [None] * 16

    def work(i):
        zi = ctypes.c_void_p()
        assert L.bpmd_inflate_stream_create(15, ctypes.byref(zi)) == 0
        try:
            if i % 4 == 0:
                src = ctypes.create_string_buffer(bad, len(bad))
                buf = ctypes.create_string_buffer(4096)
                zs = ZParams(ctypes.addressof(src), len(bad), 0, ctypes.cast(buf, ctypes.c_void_p), 4096, 0, 2)
                r = L.bpmd_inflate_stream_write(zi, ctypes.byref(zs), SYNC)
                out[i] = (r, zs.total_in, zs.total_out)
            else:
                out[i] = ws_inflate_message(L, zi, good)
        finally:
            L.bpmd_stream_destroy(zi)

    assert L.bpmd_stream_batching(256, 200) == 0
    try:
        ts = [threading.Thread(target=work, args=(i,)) for i in range(16)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    finally:
        L.bpmd_stream_batching(256, 0)
    for i in range(16):
        if i % 4 == 0:
            assert out[i] == (5, 0, 0), out[i]   # zlib::error::invalid_block_type
        else:
            assert out[i] == msg, i


def test_batching_settings_are_validated():
    L = _api()
    assert L.bpmd_stream_batching(-1, 0) != 0
    assert L.bpmd_stream_batching(5000, 0) != 0
    assert L.bpmd_stream_batching(16, -1) != 0
    assert L.bpmd_stream_batching(0, 0) == 0      # off
    assert L.bpmd_stream_batching(256, 0) == 0    # the default
    assert L.bpmd_stream_batch_stats(None, 0) != 0


# ---------------------------------------------------- lockstep inflate batches
# K threads, a barrier before every call, the batcher waiting (up to 5 s, paid
# only if a thread is late -- and then the launch count is wrong and the test
# fails, as it should: smaller batches would not be what is claimed) for
# max_calls calls: each round is ceil(K / max_calls) full launches.

R_MIXED = 100


def _mixed(R=R_MIXED):
    return [p for _, p in Z.mixed_plans(R)]


def _full_batches(stats, K, R, max_calls, what):
    print(f"{what}: K {K} R {R} max_calls {max_calls}: inflate calls {stats[0]} launches {stats[1]}, "
          f"deflate flushes {stats[2]} launches {stats[3]}")
    assert stats[:2] == [K * R, R * -(-K // max_calls)], stats


@pytest.mark.parametrize("max_calls", [16, 8])
def test_lockstep_mixed_phases_equal_oracle(max_calls):
    """16 inflaters, 100 rounds, one launch (max_calls 16) or two (8) per
    round: json with context takeover, binary L1, stored blocks with rooms of
    1 and 70000, corpus1 L9/m9, foreign encoders, a w15 stream at windowBits
    9 and at 12, two bit-flipped streams that fail part-way and are called on
    in BAD mode, a finished stream with trailing bytes (DONE), a KAT a byte at
    a time, all seven Flush values, a room of 1, and offers of 0 / 1 / 191 /
    192 / 193 bytes with rooms of 255 / 256 / 257 (the arena's 256-byte
    packing edges).  Every call equals the oracle's."""
    L = _api()
    plans = _mixed()
    stats = Z.run_lockstep(GpuInflater, plans, max_calls, L)
    _full_batches(stats, len(plans), R_MIXED, max_calls, "mixed phases")


def test_lockstep_mixed_phases_serial_loops():
    """The same batches with the serial inflate_fast loop in every workgroup."""
    L = _api()
    plans = _mixed()
    L.bpmd_diag_set_zstream_parallel(0)
    try:
        stats = Z.run_lockstep(GpuInflater, plans, 16, L)
    finally:
        L.bpmd_diag_set_zstream_parallel(-1)
    _full_batches(stats, len(plans), R_MIXED, 16, "mixed phases, serial loops")


MIB = 1 << 20


def _big_room_plans():
    """8 plans of 8 calls, each call with 1 MiB of room and at least 1001 new
    bytes (1040 n + 8192 >= 1 MiB: the room handed to the kernel stays 1
    MiB), so a batch has 8 MiB of room: five 200 KB json messages at L6, one
    of them failing early (BAD: nothing more comes out), one stream that ends
    early with trailing bytes (DONE), one whose output is 10 bytes followed by
    empty stored blocks."""
    import random
    import zlib
    rng = random.Random("big rooms")
    R = 8

    def calls(stream):
        step = len(stream) // R
        assert step >= 1001 + 64
        return [(len(stream) if k == R else k * step - rng.randrange(64), MIB, SYNC) for k in range(1, R + 1)]

    msgs = Z.msgs_of("json", [200_000] * 6, seed=0x4D1B)
    streams = [Z.connection_stream([m], level=6, mem=8) for m in msgs[:5]]
    streams.append(Z.failing_flips(Z.connection_stream([msgs[5]], level=6, mem=8), rng, 1, before=2000)[0])
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    streams.append(c.compress(msgs[0][:5000]) + c.flush(zlib.Z_FINISH) + rng.randbytes(12000))
    streams.append(Z.connection_stream([msgs[1][:10]], level=6, mem=8) + b"\x00\x00\x00\xff\xff" * 2000)
    plans = [(s, 15, calls(s)) for s in streams]
    # the oracle's side of what the docstring says
    recs = [Z.oracle_records(p) for p in plans]
    for p, rs in zip(plans, recs):
        pos = 0
        for (cut, room, _), r in zip(p[2], rs):
            assert cut - pos >= 1001 and min(room, 1040 * (cut - pos) + 8192) == MIB
            pos = r[6]
    assert all(sum(r[3] for r in rs) == 200_000 for rs in recs[:5])
    assert Z.calls_after(recs[5], Z.is_error) >= 4 and all(r[3] == 0 for r in recs[5][-4:])
    assert recs[6][1][0] == O.ERROR_CODES["end_of_stream"] and recs[6][-1][3] == 0
    assert [r[3] for r in recs[7]] == [10] + [0] * 7 and all(r[0] == 0 and r[1] > 0 for r in recs[7])
    return plans


def test_lockstep_over_4mib_of_room_then_small_rooms():
    """inflate_batch past its 4 MiB switch: the results come back first, then
    each call's used output (100 KB ones beside one of 10 bytes and calls
    with none).  Then small rooms on the same arena: the single block copy
    after the piecewise one."""
    L = _api()
    big = _big_room_plans()
    stats = Z.run_lockstep(GpuInflater, big, 8, L)
    _full_batches(stats, 8, 8, 8, "over 4 MiB of room")
    small = _mixed(40)
    stats = Z.run_lockstep(GpuInflater, small, 16, L)
    _full_batches(stats, 16, 40, 16, "small rooms after it")


# ---------------------------------------------------- lockstep deflate batches

def _deflate_conn(L, cfg, msgs, before=None):
    """One connection's messages, each one write(whole message, Flush::sync)
    with room upper_bound(n) + 16; the payloads (00 00 FF FF removed)."""
    level, mem, takeover = cfg
    zo = ctypes.c_void_p()
    assert L.bpmd_deflate_stream_create(level, 15, mem, 0, ctypes.byref(zo)) == 0
    pays = []
    try:
        for m in msgs:
            room = O.upper_bound(len(m)) + 16
            src = ctypes.create_string_buffer(m, len(m))
            out = ctypes.create_string_buffer(room)
            zs = ZParams(ctypes.addressof(src), len(m), 0, ctypes.addressof(out), room, 0, 2)
            if before:
                before()
            r = L.bpmd_deflate_stream_write(zo, ctypes.byref(zs), SYNC)
            pays.append((r, zs.avail_in, out.raw[:zs.total_out]))
            if not takeover:
                L.bpmd_deflate_stream_reset(zo)
    finally:
        L.bpmd_stream_destroy(zo)
    return pays


def _deflate_lockstep(L, cfgs, msgs_of, max_calls):
    """The connections unbatched one after another, then in lockstep through
    the batcher: byte-equal payloads, which the oracle inflates to the
    messages; returns the stats and the launches same_params (pmd_stream.hip)
    makes of full batches: per round, the distinct (level, windowBits,
    strategy, history or none) among the streams."""
    K, R = len(cfgs), len(msgs_of[0])
    assert all(len(m) == R and all(len(x) > 0 for x in m) for m in msgs_of)   # an empty message makes no flush
    assert L.bpmd_stream_batching(0, 0) == 0
    try:
        ref = [_deflate_conn(L, cfgs[i], msgs_of[i]) for i in range(K)]
    finally:
        L.bpmd_stream_batching(256, 0)
    bar = threading.Barrier(K)
    got, errs = [None] * K, []

    def work(i):
        try:
            got[i] = _deflate_conn(L, cfgs[i], msgs_of[i], before=lambda: bar.wait(60.0))
        except BaseException as e:   # noqa: BLE001 (reported after the join)
            errs.append((i, repr(e)))
            bar.abort()

    assert L.bpmd_stream_batching(max_calls, 5_000_000) == 0
    try:
        _stats(L)
        ts = [threading.Thread(target=work, args=(i,)) for i in range(K)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        stats = _stats(L)
    finally:
        L.bpmd_stream_batching(256, 0)
    assert not errs, errs
    for i in range(K):
        for r, left, pay in ref[i] + got[i]:
            assert r == 0 and left == 0 and pay.endswith(b"\x00\x00\xff\xff"), (i, r, left)
        assert got[i] == ref[i], i
        pays = [p[2][:-4] for p in got[i]]
        cap = max(len(m) for m in msgs_of[i])
        back = O.pmd_inflate_stream(pays, cap=cap) if cfgs[i][2] else [O.pmd_inflate(p, cap=cap) for p in pays]
        assert back == [(0, m) for m in msgs_of[i]], i
    launches = sum(len({(cfgs[i][0], 15, 0, r > 0 and cfgs[i][2]) for i in range(K)}) for r in range(R))
    return stats, launches


def test_lockstep_deflate_groups():
    """12 deflaters (levels 1, 6, 9, with and without context takeover), 4
    rounds of one sync flush each, all 12 flushes of a round in one batch:
    one launch per parameter group -- 3 in the first round (no stream has
    history), 6 in each later one."""
    L = _api()
    cfgs = [((1, 6, 9)[i % 3], (4, 8)[(i // 6) % 2], (i // 3) % 2 == 0) for i in range(12)]
    sizes = [1, 700, 4096, 4097, 30000]
    msgs_of = []
    for i in range(12):
        ns = [sizes[(i + 2 * r + i // 5) % 5] for r in range(4)]
        raw, off, ln = synth.make_batch("json", ns, seed=0x5EED0700 + i)
        msgs_of.append([bytes(raw[int(off[k]):int(off[k]) + int(ln[k])]) for k in range(4)])
    assert {len(m) for ms in msgs_of for m in ms} == set(sizes)
    stats, launches = _deflate_lockstep(L, cfgs, msgs_of, 12)
    print(f"deflate groups: flushes {stats[2]} launches {stats[3]} (expected {launches})")
    assert launches == 3 + 3 * 6
    assert stats[2:] == [48, launches], stats


def test_lockstep_deflate_over_4mib():
    """deflate_group past its 4 MiB switch (8 x 600 KiB messages, about 614
    KB of output room each): the meta block comes back first, then each
    flush's output."""
    L = _api()
    cfgs = [(6, 8, True)] * 8
    raw, off, ln = synth.make_batch("json", [600 * 1024] * 8, seed=0x5EED0800)
    msgs_of = [[bytes(raw[int(off[k]):int(off[k]) + int(ln[k])])] for k in range(8)]
    assert 8 * ((O.upper_bound(600 * 1024) + 16 + 255) & ~255) > 4 * MIB
    stats, launches = _deflate_lockstep(L, cfgs, msgs_of, 8)
    print(f"deflate over 4 MiB: flushes {stats[2]} launches {stats[3]} (expected {launches})")
    assert launches == 1
    assert stats[2:] == [8, 1], stats
