"""GPU: the per-stream deflater (bpmd_deflate_stream_*, pmd_stream.hip) run
through the scripts of tests/deflate_scripts.py beside the oracle backend
(Beast's deflate_stream restated): every Flush value, params(), tune(),
prime() and pending(), at levels 0-9, windowBits 9 / 10 / 15 and every
strategy, with the stream batcher off ("unbatched": each flush is a
deflate_group of one on the stream's own arena) and on ("batched": the
coalescer's groups on its leader's arena).  The call protocol alone, without
a device, is tests/test_deflate_writer.py.

A  call parity: per step the return code, avail_in and total_in equal the
   oracle backend's on the same script, and pending() after prime().
B  flush-point decodability: after partial / sync / full / trees / finish the
   oracle's inflater, at the stream's windowBits, returns all input so far
   from all output so far; after none / block a prefix of it.
C  framing: "ends with 00 00 FF FF" and "nothing pending" equal the oracle's
   at every flush.
D  restart: what follows a Flush::full decodes from a fresh inflater; what
   follows a Flush::sync does not (so the history is in use).
E  small output rooms.
tests/test_deflate_scripts.py shows that the reference itself passes B-E."""
import pytest

from tests import deflate_scripts as S

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(script, cfg, room=None):
    """The oracle backend's run, computed once per script and configuration."""
    key = (tuple(script), tuple(sorted(cfg.items())), room)
    if key not in _REF:
        _REF[key] = S.run(S.oracle_backend(), script, room=room, **cfg)
    return _REF[key]


@pytest.fixture(params=[(0, 0), (256, 0)], ids=["unbatched", "batched"])
def lib(request):
    L = S.gpu_library()
    before = S.batching(L)
    assert L.bpmd_stream_batching(*request.param) == 0
    try:
        yield L
    finally:
        assert L.bpmd_stream_batching(*before) == 0


def _abc(L, script, cfg):
    steps = S.run(L, script, **cfg)
    ref = _ref(script, cfg)
    S.check_call_parity(steps, ref)
    S.check_decodable(steps, script, cfg["wbits"])
    S.check_framing(steps, ref)
    return steps


@pytest.mark.parametrize("wbits", S.WBITS)
@pytest.mark.parametrize("level", S.LEVELS)
def test_flush_matrix(lib, level, wbits):
    """Each of partial, sync, full, trees and block as the repeating flush
    between segments of every length in S.LENGTHS and every synth kind, and a
    script that mixes them all and goes on calling after finish; every
    strategy.  A, B, C, and D wherever a Flush::full occurs."""
    for strategy in range(5):
        seed = level * 5 + strategy + wbits
        for n, flush in enumerate(("partial", "sync", "full", "trees", "block")):
            _abc(lib, S.repeating(flush, seed + n), S.config(level, wbits, strategy, n))
        S.check_restart(lib, S.repeating("full", seed + 2), S.config(level, wbits, strategy, 2))
        _abc(lib, S.mixed(seed), S.config(level, wbits, strategy, 5))
        S.check_restart(lib, S.full_restart(seed), S.config(level, wbits, strategy))
        S.check_restart(lib, S.mixed(seed), S.config(level, wbits, strategy))


@pytest.mark.parametrize("level", (0, 1, 6, 9))
def test_full_flush_restarts(lib, level):
    """D on its own: a 1500-byte segment written twice and a third one, each
    with Flush::full (clear_hash(), deflate_stream.ipp:474-483): the bytes
    after every full flush decode from a fresh inflater.  Above level 0 the
    same script with sync in place of full does not restart, so the history
    that full has to drop really is in use."""
    script = S.full_restart(level)
    S.check_restart(lib, script, S.config(level, 15, 0))
    _abc(lib, script, S.config(level, 15, 0))
    if level:
        S.check_sync_does_not_restart(lib, script, S.config(level, 15, 0))


@pytest.mark.parametrize("level", (0, 6))
def test_trees_flush_framing(lib, level):
    """C on its own: on the deflate side Flush::trees falls into
    `flush != Flush::block` (deflate_stream.ipp:467-470) and emits the empty
    stored block: 00 00 FF FF, byte aligned, nothing pending, as sync."""
    script = [("write", S.segment("json", 700), "trees"), ("pending",), ("write", S.segment("json", 4097), "trees"),
              ("write", b"", "trees"), ("write", S.segment("binary", 300), "finish")]
    steps = _abc(lib, script, S.config(level, 15, 0))
    assert [f[2:] for f in S.framing(steps)[:2]] == [(True, 0, 0)] * 2


@pytest.mark.parametrize("level", (1, 6, 9))
def test_sync_does_not_restart(lib, level):
    """D's other half: with sync in place of full, the second copy of a
    1500-byte segment is smaller than the first and a fresh inflater cannot
    decode it."""
    S.check_sync_does_not_restart(lib, S.full_restart(level), S.config(level, 15, 0))


@pytest.mark.parametrize("wbits", (9, 10, 15))
@pytest.mark.parametrize("level", (1, 6, 9))
def test_history_against_the_window(lib, level, wbits):
    """Text of period P written in three parts with sync between them: the
    cheapest match of the later parts lies P back, in the history, across the
    flush, the chunk histories of 2048 and 4096 bytes and, at windowBits 9 and
    10, max_dist = 2^wbits - 262.  The inflater runs at the same windowBits,
    so a match from beyond the window is invalid_distance.  At windowBits 15
    and P <= 2048 the history must be in use: the second part is smaller than
    the first and does not decode on its own."""
    for period in S.PERIODS:
        for n in (6000, 13000):
            script = S.history_window(period, n=n)
            steps = _abc(lib, script, S.config(level, wbits, 0, period))
            if wbits == 15 and period <= 2048:
                assert len(steps[1].out) < len(steps[0].out), (period, n, len(steps[0].out), len(steps[1].out))
                (status, back), fed = S.restart_after(steps, 0, wbits)
                assert status not in ("ok", "end_of_stream") or len(back) < len(fed), (period, n, status)


@pytest.mark.parametrize("k", (1, 2, 5, 7, 64))
def test_tight_output(lib, k):
    """E: every call gets k bytes of room; pending() after every call that
    leaves bytes behind is exactly what the later calls hand out."""
    for level in (6, 0):
        for wbits in (9, 15):
            for n, script in enumerate(S.tight_scripts(level + wbits)):
                cfg = S.config(level, wbits, 0, n)
                S.check_tight(S.run(lib, script, room=("tight", k), **cfg), script, wbits, k, strict=True)


@pytest.mark.parametrize("data", (S.HELLO, S.corpus56()), ids=("hello", "corpus56"))
def test_split_pattern(lib, data):
    """The reference harness's pattern (test/beast/zlib/deflate_stream.cpp:352-405):
    Flush::none with the first i bytes, Flush::full with the rest into j bytes
    of room and then the remainder, for every i."""
    cfg = S.config(6, 15)
    for i in range(len(data) + 1):
        script = S.split_pattern(data, i)
        for j in (1, 2, 3, 5, 8, 13):
            steps = S.run(lib, script, room=("split", j), **cfg)
            S.check_decodable(steps, script, 15)
            S.check_call_parity(steps, _ref(script, cfg, ("split", j)))


@pytest.mark.parametrize("buffered", (False, True))
def test_params_mid_stream(lib, buffered):
    """Level 6 -> 0 -> 9 -> 1 and strategy normal -> huffman -> rle -> fixed ->
    normal between segments, with and without input buffered at the switch:
    A against the oracle, B at every later flush; what is written at level 0
    costs at least its own length; an invalid level is stream_error."""
    for seed in range(3):
        script = S.params_script(seed, buffered)
        steps = _abc(lib, script, S.config(6, 15, 0, seed))
        bad = [s.rc for st, s in zip(script, steps) if st[0] == "params" and not 0 <= st[1] <= 9]
        assert bad == [S.STREAM_ERROR] * 2
        cost = S.level0_cost(steps, script)
        assert cost and all(out >= n for out, n in cost), cost


@pytest.mark.parametrize("level", (6, 3))
def test_tune(lib, level):
    """tune() with rows of the level table: undone before the first write,
    a no-op with the level's own row, decodable with the level-1 and level-9
    rows (the level-1 row no smaller), dropped by params() to another level
    and by reset(), kept after prime()."""
    S.check_tune(lib, lambda script, **cfg: _abc(lib, script, cfg), level=level)


@pytest.mark.parametrize("kind", sorted(S.PRIMES))
def test_prime(lib, kind):
    """prime() before the first write and between flushes, in pieces of 0, 1,
    5, 8, 13 and 16 bits that add up to whole empty blocks (S.PRIMES): A
    (pending() included) and B over the stream with the primed bits in it."""
    for between in (False, True):
        for level in (1, 6):
            _abc(lib, S.prime_script(kind, level, between), S.config(level, 15, 0))


def test_prime_only_pending(lib):
    script = S.prime_only()
    steps = S.run(lib, script)
    S.check_call_parity(steps, _ref(script, {}))
    assert [s.pend for s in steps] == [(0, 5), (2, 2), (4, 2), (4, 2)]
