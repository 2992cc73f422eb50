"""The deflate scripts and checks of tests/deflate_scripts.py on the oracle
backend alone (tests/cpp/oracle_backend.c: Beast's deflate_stream restated):
every check that tests/test_gpu_deflate_stream.py makes of the GPU stream
holds for the reference itself, so none asks more than Beast delivers.  Check
A (call parity) is the run compared with a second run of itself: a smoke test
of the driver."""
import pytest

from tests import deflate_scripts as S

LEVELS, WBITS, _cfg = S.LEVELS, S.WBITS, S.config


def _abc(L, script, cfg):
    steps = S.run(L, script, **cfg)
    S.check_call_parity(steps, S.run(L, script, **cfg))
    S.check_decodable(steps, script, cfg["wbits"])
    S.check_framing(steps, steps)
    return steps


@pytest.mark.parametrize("wbits", WBITS)
@pytest.mark.parametrize("level", LEVELS)
def test_flush_matrix(level, wbits):
    L = S.oracle_backend()
    for strategy in range(5):
        seed = level * 5 + strategy + wbits
        for n, flush in enumerate(("partial", "sync", "full", "trees", "block")):
            _abc(L, S.repeating(flush, seed + n), _cfg(level, wbits, strategy, n))
        S.check_restart(L, S.repeating("full", seed + 2), _cfg(level, wbits, strategy, 2))
        _abc(L, S.mixed(seed), _cfg(level, wbits, strategy, 5))
        S.check_restart(L, S.full_restart(seed), _cfg(level, wbits, strategy))
        S.check_restart(L, S.mixed(seed), _cfg(level, wbits, strategy))


@pytest.mark.parametrize("level", (1, 6, 9))
def test_sync_does_not_restart(level):
    """Check D's non-vacuity half on the reference: after sync the second copy
    of a segment refers to the first."""
    L = S.oracle_backend()
    S.check_sync_does_not_restart(L, S.full_restart(level), _cfg(level, 15, 0))


def test_flush_framing_of_the_reference():
    """What check C compares with: sync, full and trees end in 00 00 FF FF
    with nothing pending (trees falls into `flush != Flush::block`,
    deflate_stream.ipp:467-470), block and partial do not."""
    L = S.oracle_backend()
    for flush in ("partial", "sync", "full", "trees", "block"):
        steps = S.run(L, [("write", S.segment("json", 700), flush)])
        marker = S.framing(steps)[0][2]
        assert marker == (flush in ("sync", "full", "trees")), flush
        if marker:
            assert steps[0].pend == (0, 0)


@pytest.mark.parametrize("wbits", (9, 10, 15))
@pytest.mark.parametrize("level", (1, 6, 9))
def test_history_against_the_window(level, wbits):
    L = S.oracle_backend()
    for period in S.PERIODS:
        for n in (6000, 13000):
            script = S.history_window(period, n=n)
            steps = _abc(L, script, _cfg(level, wbits, 0, period))
            if wbits == 15 and period <= 2048:
                assert len(steps[1].out) < len(steps[0].out), (period, n, len(steps[0].out), len(steps[1].out))
                (status, back), fed = S.restart_after(steps, 0, wbits)
                assert status not in ("ok", "end_of_stream") or len(back) < len(fed), (period, n, status)


@pytest.mark.parametrize("k", (1, 2, 5, 7, 64))
def test_tight_output(k):
    L = S.oracle_backend()
    for level in (6, 0):
        for wbits in (9, 15):
            for n, script in enumerate(S.tight_scripts(level + wbits)):
                cfg = _cfg(level, wbits, 0, n)
                S.check_tight(S.run(L, script, room=("tight", k), **cfg), script, wbits, k)


@pytest.mark.parametrize("data", (S.HELLO, S.corpus56()), ids=("hello", "corpus56"))
def test_split_pattern(data):
    L = S.oracle_backend()
    for i in range(len(data) + 1):
        script = S.split_pattern(data, i)
        for j in (1, 2, 3, 5, 8, 13):
            steps = S.run(L, script, room=("split", j))
            S.check_decodable(steps, script, 15)
            assert [s.rc for s in steps] == [S.OK if i else S.NEED_BUFFERS, S.OK, S.END_OF_STREAM], (i, j)


@pytest.mark.parametrize("buffered", (False, True))
def test_params_mid_stream(buffered):
    L = S.oracle_backend()
    for seed in range(3):
        script = S.params_script(seed, buffered)
        steps = _abc(L, script, _cfg(6, 15, 0, seed))
        bad = [s.rc for st, s in zip(script, steps) if st[0] == "params" and not 0 <= st[1] <= 9]
        assert bad == [S.STREAM_ERROR] * 2
        cost = S.level0_cost(steps, script)
        assert cost and all(out >= n for out, n in cost), cost


@pytest.mark.parametrize("level", (6, 3))
def test_tune(level):
    L = S.oracle_backend()
    S.check_tune(L, lambda script, **cfg: S.run(L, script, **cfg), level=level)


@pytest.mark.parametrize("kind", sorted(S.PRIMES))
def test_prime(kind):
    L = S.oracle_backend()
    for between in (False, True):
        for level in (1, 6):
            _abc(L, S.prime_script(kind, level, between), _cfg(level, 15, 0))


def test_prime_only_pending():
    steps = S.run(S.oracle_backend(), S.prime_only())
    assert [s.pend for s in steps] == [(0, 5), (2, 2), (4, 2), (4, 2)]


def test_oracle_deflater_wrapper():
    """oracle.Deflater's params / tune / pending / prime / upper_bound reach
    bzo_deflate_*: the same numbers as through the backend library."""
    import ctypes
    from oracle import oracle as O
    z = O.Deflater(6, 15, 8, 0)
    got = []
    for bits, value in ((5, 0x15), (13, 0x1ABC), (16, 0xBEEF)):
        assert z.prime(bits, value) == 0
        got.append(z.pending())
    assert got == [(0, 5), (2, 2), (4, 2)]
    z.tune(*S.LEVEL_ROWS[1])
    data = S.segment("json", 3000)
    src = ctypes.create_string_buffer(data, len(data))
    room = O.upper_bound(len(data)) + 64
    out = ctypes.create_string_buffer(room)
    zs = O.ZParams(ctypes.addressof(src), len(data), 0, ctypes.addressof(out), room, 0, 2)
    assert z.write(zs, "none") == 0 and zs.avail_in == 0
    assert z.params(zs, 0, 0) == 0 and z.params(zs, 10, 0) == O.ERROR_CODES["stream_error"]
    assert z.write(zs, "finish") == O.ERROR_CODES["end_of_stream"]
    steps = S.run(S.oracle_backend(), [("prime", 5, 0x15), ("prime", 13, 0x1ABC), ("prime", 16, 0xBEEF),
                                       ("tune",) + S.LEVEL_ROWS[1], ("write", data, "none"), ("params", 0, 0),
                                       ("write", b"", "finish")], level=6, wbits=15, mem=8)
    assert out.raw[:zs.total_out] == S.output(steps)
    assert z.upper_bound(1000) == 1000 + (1000 >> 12) + (1000 >> 14) + (1000 >> 25) + 7   # deflate_stream.ipp:300-302
    assert O.Deflater(6, 10, 8, 0).upper_bound(1000) == 1000 + 125 + 16 + 5            # the conservative bound (:290-291)
