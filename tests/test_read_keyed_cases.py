"""The keyed receive path's test batches (tests/read_keyed_cases.py), checked
on the CPU: the builders give the lengths, alignments and counts that
tests/test_gpu_read_keyed.py relies on, and the compiled inflate_plan.h sends
each batch down the branch that test is about."""
import random

import pytest

from oracle import oracle as O
from tests import read_keyed_cases as K
from tests.test_inflate_plan import (AUTO, G_WAVE_ORDERED, lanes_plain, lanes_queue, lanes_wave_split, load_plan)

IN_CAP = K.in_cap()


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return load_plan(tmp_path_factory.mktemp("read_keyed_plan"))


@pytest.fixture(scope="module")
def grid():
    return K.edge_grid(IN_CAP)


def test_in_cap_is_whole_words():
    assert IN_CAP % 4 == 0 and IN_CAP >= 256


def test_stored_payload_has_the_exact_length_and_inflates():
    rng = random.Random(1)
    for n in list(range(6, 81)) + list(range(IN_CAP - 8, IN_CAP + 41)) + [2 * IN_CAP + 20, 4095, 4096, 4097]:
        p = K.stored_payload(n, rng)
        assert len(p) == n
        st, out = O.pmd_inflate(p, cap=n)
        assert st == 0
        # the stored bytes come back: total minus the headers and the closing byte
        blocks, pos = 0, 0
        while pos < n - 1:
            pos += 5 + int.from_bytes(p[pos + 1:pos + 3], "little")
            blocks += 1
        assert pos == n - 1 and len(out) == n - 1 - 5 * blocks


def test_truncated_is_a_prefix():
    p = O.pmd_deflate(K.synth_msg("json", 3000, 1), 6, 15, 4)
    for n in (0, 1, 7, len(p)):
        assert K.truncated(p, n) == p[:n]


def test_edge_grid_covers_every_alignment_and_length(grid):
    lengths = K.edge_lengths(IN_CAP)
    assert set(range(0, 81)) <= set(lengths)
    assert set(range(IN_CAP - 8, IN_CAP + 41)) <= set(lengths)
    assert set(range(2 * IN_CAP - 4, 2 * IN_CAP + 21)) <= set(lengths)
    have = {}
    for kind, p, a in zip(grid.info["kinds"], grid.payloads, grid.aligns):
        if kind[0] in ("stored", "truncated"):
            assert (kind[1], kind[2]) == (a, len(p))
            have.setdefault(kind[0], set()).add((a, len(p)))
    for a in range(16):
        for n in lengths:
            assert (a, n) in have["truncated"], (a, n)
            assert n < 6 or (a, n) in have["stored"], (a, n)
    assert grid.info["whole"] >= 200
    assert 4800 <= len(grid.payloads) <= 5400
    # the fixed keys and random ones, every 7th capacity one short, every 31st one byte
    assert set(K.FIXED_KEYS) <= set(grid.keys) and len(set(grid.keys)) > 100
    assert min(grid.caps) == 1


def test_edge_grid_one_byte_keys_meet_every_alignment(grid):
    seen = {(k, a) for k, a in zip(grid.keys, grid.aligns)}
    for k in K.FIXED_KEYS:
        for a in range(16):
            assert (k, a) in seen


def test_batch_oracle_equals_the_single_message_oracle(grid):
    st, ln, outs = K.expect(grid)
    for i in range(0, len(grid.payloads), 17):
        est, eout = O.pmd_inflate(grid.payloads[i], cap=grid.caps[i])
        assert (int(st[i]), int(ln[i]), outs[i]) == (est, len(eout), eout), i


@pytest.mark.parametrize("split", [4096, 1024])
def test_split_batch_counts(split):
    c = K.split_batch(2048, split, random.Random(31))
    lens = [len(p) for p in c.payloads]
    assert len(lens) == 2048
    for n in (split - 1, split, split + 1):
        assert n in lens
    assert sum(n > split for n in lens) >= 48
    assert sum(c.text) > 500 and len(set(c.keys)) > 2000
    st, _, _ = K.expect(c)
    assert (st == K.BAD_FRAME_PAYLOAD).sum() >= 20      # spoiled text


def test_queue_batch_counts():
    c = K.queue_batch(4096, 512, random.Random(41))
    lens = [len(p) for p in c.payloads]
    thr = max(4096, 200 * sum(lens) // (100 * 512))
    tk = (thr + 63) >> 6
    assert tk == c.info["thr_key"]
    long_ = [n for n in lens if (n >> 6) >= tk]
    mid = [n for n in lens if n >= 2048 and (n >> 6) < tk]
    assert len(long_) >= 16 and len(mid) >= 16
    assert len(lens) == 4096


def test_plans_of_the_gpu_tests(plan):
    wgs = 1024   # 4 workgroups on each of 256 compute units
    # in-process: 2048 keyed messages split at BPMD_INFLATE_SPLIT, 32768 on plain lanes
    assert plan(AUTO, 2048, key=True, wgs=wgs, split=4096) == lanes_wave_split(4096)
    assert plan(AUTO, 2048, key=True, wgs=wgs, split=1024) == lanes_wave_split(1024)
    assert plan(AUTO, 32768, key=True, wgs=wgs) == lanes_plain()
    # children: BPMD_QUEUE_WGS=8 BPMD_INFLATE_SPLIT=0, 4096 messages
    wave_ordered = lanes_queue(long=G_WAVE_ORDERED, args=(512, 4096, 200))
    assert plan(AUTO, 4096, key=True, wgs=8, split=0) == wave_ordered
    assert plan(AUTO, 4096, key=False, wgs=8, split=0, bp=False) == wave_ordered
    assert plan(AUTO, 4096, key=True, wgs=8, split=0, ordered=False) == lanes_queue(order=False)


def test_masking_is_an_involution_over_the_builders(grid):
    rng = random.Random(3)
    for i in range(0, len(grid.payloads), 13):
        p, k = grid.payloads[i], grid.keys[i]
        assert O.mask(O.mask(p, k), k) == p
        assert O.pmd_inflate(O.mask(O.mask(p, k), k), cap=grid.caps[i]) == O.pmd_inflate(p, cap=grid.caps[i])
    p = K.stored_payload(100, rng)
    assert O.mask(p, 0x000000FF)[:8] == bytes([p[0] ^ 0xFF, p[1], p[2], p[3], p[4] ^ 0xFF, p[5], p[6], p[7]])


def test_utf8_edge_cases_straddle_units_and_the_wave_step():
    cases = K.utf8_edge_cases()
    assert {a for a, _ in cases} == set(range(16))
    verdicts = {0: 0, 1: 0, 2: 0}
    for a, t in cases[::7]:
        verdicts[O.utf8_check(t)] += 1
    assert all(verdicts.values()), verdicts
    # a 4-byte code point over the 1 KiB step at every alignment, in all three forms
    for a in range(16):
        o = 1024 - a - 2
        lead = [t for b, t in cases if b == a and len(t) > o and t[o] == 0xF0]
        assert len(lead) >= 3, a
