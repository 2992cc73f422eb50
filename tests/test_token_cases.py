"""The token-level payloads of tests/token_cases.py, pinned on the CPU before
any GPU decodes them: every well-formed message must inflate to the builder's
own bytes in the oracle and in CPython's zlib (three independent decoders),
and the conditions the families are there for are asserted on the built
cases."""
import time
import zlib

import pytest

from oracle import oracle as O
from tests import token_cases as T

FAMS = sorted(T.FAMILIES)


def test_codes_of_the_long_renderer():
    assert T.kraft(T.LONG_LIT) == 1.0 and T.kraft(T.LONG_DIST) == 1.0
    assert all(T.LONG_LIT[s] == 15 for s in (281, 282, 283, 284))
    assert T.LONG_DIST[28] == T.LONG_DIST[29] == 15
    assert sorted(l for l in T.LONG_DIST if l) == list(range(1, 15)) + [15, 15]
    assert all(T.LEXT[s - 257] == 5 for s in (281, 282, 283, 284)) and T.DEXT[28] == T.DEXT[29] == 13
    # the one incomplete code the reference accepts: a single 1-bit symbol
    assert T.kraft(T.HOLE_DIST) == 0.5


def test_renderers_on_a_hand_checked_message():
    toks = [97, 98, (4, 2), T.CUT, 99, (3, 5)]
    want = b"ababab" + b"c" + b"aba"
    for mode in ("fixed", "dyn"):
        r = T.render(toks, mode)
        assert r.good and r.out == want, mode
        assert list(r.pos) == [0, 1, 2, 6, 6, 7, 10]
        assert O.pmd_inflate(r.payload) == (0, want)
    # fixed: 3 header bits, 8-bit literals, (4, 2) = 7 + 5 bits
    r = T.render(toks, "fixed")
    assert list(r.bit)[:4] == [3, 11, 19, 31]
    r = T.render([97] * 3 + [("m", 284, 31, 0, 0)], "long")
    assert r.out == b"a" * 261 and O.pmd_inflate(r.payload) == (0, r.out)


@pytest.mark.parametrize("fam", FAMS)
def test_well_formed_messages_in_three_decoders(fam):
    t0 = time.time()
    cases = T.family(fam)
    built = time.time() - t0
    good = 0
    for c in cases:
        st, out = O.pmd_inflate(c.payload, cap=len(c.out) + 300)
        if c.expect is None:   # a payload cut short: the oracle alone says what it is
            continue
        assert O.ERRORS[st] == c.expect, (c.describe(len(out)), O.ERRORS[st])
        assert out == c.out, c.describe(next((i for i, (a, b) in enumerate(zip(out, c.out)) if a != b),
                                             min(len(out), len(c.out))))
        if c.good:
            good += 1
            assert zlib.decompressobj(-15).decompress(c.payload + T.EB) == c.out, c.describe(0)
    assert good > 0 or fam == "H"
    assert built < 60, built
    # the block-parallel decoder takes payloads from 64 bytes up
    assert any(c.mode in ("dyn", "long", "hole") and len(c.payload) >= T.BP_FLOOR for c in cases), fam
    if fam != "H":   # the code of the dyn renderer is complete: it has no code word that stands for nothing
        assert any(c.mode == "dyn" and len(c.payload) >= T.BP_FLOOR for c in cases), fam
        assert {c.mode for c in cases} >= {"fixed", "dyn"}


def test_family_a_grid():
    cases = T.family("A")
    assert len(cases) == 2 * 576
    assert {c.key for c in cases} == {(d, lead) for d in T.A_DISTS for lead in range(6)}
    for c in cases[::37]:
        matches = [t for t in c.tokens if not isinstance(t, int)]
        assert [n for n, _ in matches] == T.A_LENS and {d for _, d in matches} == {c.key[0]}


def test_family_c_has_deep_chains():
    depths = [T.chain_depth([t for t in c.tokens[c.key[1]:]]) for c in T.family("C")]
    assert max(depths) >= 6 and sum(1 for d in depths if d >= 6) >= 100
    # the chains lie in one 64-byte chunk when nothing is put between their matches
    for c in T.family("C"):
        if c.key[2] == 0:
            assert len(c.out) - c.key[1] <= 64


def test_family_d_sources_end_at_the_destination():
    keys = {c.key for c in T.family("D")}
    for d in range(1, 41):
        want = {n for n in (d - 1, d, d + 1, 2 * d, 2 * d + 1) if 3 <= n <= 258} | ({258} if d >= 8 else set())
        assert {n for dd, n in keys if dd == d} == want, d
    for c in T.family("D"):
        d, n = c.key
        i = next(i for i, t in enumerate(c.tokens) if not isinstance(t, int))
        assert c.tokens[i] == (n, d) and c.pos[i] == d + 2   # its source ends n - d bytes past where it starts writing
        n2, d2 = c.tokens[i + 1]
        assert 1 <= d2 <= n and n2 >= 3   # the second match starts reading inside the first one's tail


def test_family_e_capacities():
    for c in T.family("E"):
        n = len(c.out)
        assert sorted(cap for cap, raw, _ in c.runs if not raw) == list(range(1, n + 3))
        assert sorted(cap for cap, raw, _ in c.runs if raw) == list(range(1, n + 3))
        for cap, raw, wbits in c.runs:
            st, out = O.pmd_inflate(c.payload, cap=cap, raw=raw, wbits=wbits)
            assert out == c.out[:cap]
            assert O.ERRORS[st] in ("ok", "need_buffers")
            if cap < n and not raw:
                assert O.ERRORS[st] == "need_buffers", (c.name, c.mode, cap)


def test_family_f_statuses():
    at = past = 0
    for c in T.family("F"):
        st, out = O.pmd_inflate(c.payload, cap=len(c.out) + 300)
        if c.key[-1] == "past":
            assert O.ERRORS[st] == "invalid_distance", c.name
            past += 1
        elif c.key[-1] == "at":
            assert O.ERRORS[st] == "ok" and out == c.out, c.name
            at += 1
        else:   # beyond 2^windowBits: a single call accepts any distance up to the bytes produced
            for cap, raw, wbits in c.runs:
                st, out = O.pmd_inflate(c.payload, cap=cap, raw=raw, wbits=wbits)
                assert O.ERRORS[st] == c.expect and out == c.out, (c.name, wbits)
    assert at >= 2 * 2 * 2 * (len(T.F_POS) - 1 + 5) and past >= 2 * 2 * 2 * (len(T.F_POS) + 5)


def _edge_token(c):
    return next(i for i, t in enumerate(c.tokens) if not isinstance(t, int)
                and (t[0] in ("L", "D", "X") or t[1] >= c.pos[i]))


@pytest.mark.parametrize("raw", [False, True])
def test_family_f_places_in_the_lane_decoders_iterations(raw):
    """From the built payloads (Case.lane_place models data_step's grouping):
    with literals after it, the token under test is the 1st, 2nd, 3rd and 4th
    symbol of an iteration that had the input for several symbols -- so
    `dist > pos + hist` is evaluated after the iteration's literals were
    added to pos, on the accepting and on the rejecting side, in both
    renderers; at the input's end it is the iteration's only symbol.  (An
    iteration is at most KLIT literals, or fewer and one main symbol: there
    is no 5th.)"""
    seen = {}
    for c in T.family("F"):
        if c.key[0] == "window":
            continue
        tail, side = c.key[-2], c.key[-1]
        i = _edge_token(c)
        roomy = max(cap for cap, r, _ in c.runs if r == raw)
        before, left = c.lane_place(roomy, raw)[i]
        if tail:
            assert left >= T.LANE_MULTI_BITS, (c.name, c.mode, left)
            if c.mode == "fixed":   # one block: r literals after a match, or i literals from the start
                assert before == (c.key[1] if c.key[0] == "match" else i) % T.KLIT, c.name
            seen.setdefault((c.mode, side, c.key[2]), set()).add(before)
        else:
            assert before == 0 or left >= T.LANE_MULTI_BITS, c.name
    assert len(seen) == 2 * 2 * 2
    for k, places in seen.items():
        assert places == set(range(T.KLIT)), (k, places)


def test_family_g_has_48_bit_tokens_at_every_bit_phase():
    phases = set()
    for c in T.family("G"):
        if c.mode != "long" or c.expect is None:
            continue
        group = [i for i, t in enumerate(c.tokens) if not isinstance(t, int) and t[0] == "m"]
        assert len(group) == 8
        for i in group:
            assert c.token_bits(i) == 48, (c.name, i, c.token_bits(i))
            phases.add(c.bit[i] % 8)
        assert c.pos[group[0]] > 32768   # every distance of 13 extra bits is within reach
        # the group ends within the last 48 bits + end of block of the payload
        assert 8 * len(c.payload) - c.bit[group[-1] + 1] <= 16
    assert phases == set(range(8))
    cuts = {c.key for c in T.family("G") if c.expect is None}
    assert len(cuts) == (8 + 2 * 2) * 12


def test_family_h_statuses():
    seen = set()
    for c in T.family("H"):
        st, _ = O.pmd_inflate(c.payload, cap=600)
        assert O.ERRORS[st] == c.expect, c.name
        seen.add((c.key[0], c.key[2]))
        # at the input's end: the bad symbol ends within its last 48 bits
        bad = next(i for i, t in enumerate(c.tokens) if not isinstance(t, int) and t[0] in ("L", "D", "X"))
        if c.key[3] == 0:
            assert 8 * len(c.payload) - c.bit[bad + 1] < 48, c.name
    assert len(seen) == 5 * 5
    # 24 literals before the input's end, every bad symbol is the 1st to 4th of a lane decoder iteration
    for raw in (False, True):
        places = {}
        for c in T.family("H"):
            if c.key[3]:
                before, left = c.lane_place(600, raw)[_edge_token(c)]
                assert left >= T.LANE_MULTI_BITS, c.name
                places.setdefault(c.key[0], set()).add(before)
        assert len(places) == 5 and all(v == set(range(T.KLIT)) for v in places.values()), places


def test_history_connections_in_the_oracle():
    conns = T.history_connections()
    assert len(conns) == 6 * 10 * 2
    ok = bad = 0
    for name, wbits, pls in conns:
        (s0, _), (s1, out) = O.pmd_inflate_stream(pls, cap=1024, wbits=wbits)
        assert s0 == 0, name
        ok += s1 == 0
        bad += O.ERRORS[s1] == "invalid_distance"
    assert ok == bad == 60
