"""The inputs of the long-message GPU tests of bpmd_receive_pieces_batch
(tests/receive_pieces_cases.py) run through the model alone
(tests/receive_pieces_model.py: the walk in Python, the oracle's inflate_stream
and utf8_checker), and the conditions on them that the GPU tests lean on: the
valid ones are valid and arrive whole, the invalid ones fail where they are
meant to, history is used where a case is there for the window, the sizes
pass the kernels' thresholds, and every split the UTF-8 cases are there for is
present and lies where its tag says."""
import collections
import itertools

import pytest

from oracle import oracle as O
from tests import receive_pieces_cases as C
from tests import receive_pieces_model as M

IST, FLUSH_AT, RING = 4096, 16384, 65536      # pmd_zstream.hip: input staging, flush threshold, history ring


def run_model(case):
    log = case.run(C.ModelRig(case.n, case.role, **case.rig))
    for c in range(case.n):
        assert C.events(log[c]) == case.want[c], (c, case.tags[c])
        bad = None if case.fail_piece is None else case.fail_piece[c]
        if bad is None:
            assert all(p.status == 0 for p in log[c]), (c, case.tags[c])
        else:
            assert [p.status for p in log[c]] == [0] * bad + [M.BAD_FRAME_PAYLOAD], (c, case.tags[c])
    return log


def alone(payload, n):
    return O.pmd_inflate(payload, cap=n + 64)


def check_history_used(case, first=1):
    """messages after the first do not inflate alone: their matches reach into
    the window.  Two kinds are exempt, because the window holds nothing for
    them.  random: the deflater stores its bytes, a stored block copies
    nothing, and every such message is shown to inflate alone.  binary
    (synth.c): each message is drawn on its own, 7/8 random bytes and 1/8
    copies of earlier spans of the same message, so an earlier message shares
    nothing with it but chance triples; shown by the history saving it under
    a tenth of a percent against the same message deflated alone."""
    for c in range(case.n):
        for k in range(first, len(case.msgs[c])):
            m, p = case.msgs[c][k], case.pays[c][k]
            if case.tags[c] == "random":
                assert (p[0] >> 1) & 3 == 0 and alone(p, len(m)) == (0, m), (c, k)
            elif case.tags[c] == "binary":
                assert len(p) > 0.999 * len(O.pmd_deflate(m, 6, case.rig["wbits"], 4)), (c, k)
            else:
                assert alone(p, len(m)) != (0, m), (c, k, case.tags[c])


def check_residues(case):
    for name in ("out_res", "wire_res", "msg_res"):
        assert set(case.rig[name]) == set(range(16)), name


def test_long_messages_in_read_buffer_pieces():
    case = C.long_messages()
    assert case.n == 70 and collections.Counter(case.tags) == {k: 14 for k in C.KINDS}
    assert all(len(m) == 16384 for ms in case.msgs for m in ms)
    assert case.rig["out_cap"] == 1540 and case.rig["msg_cap"] == 16384 and case.buf == case.step == 1536
    check_residues(case)
    log = run_model(case)
    check_history_used(case)
    for c in range(case.n):
        gathered = [p.out_len for p in log[c]]
        # pieces over 1 KiB (a second round of the copy), none over the buffer; zeros' whole payloads are a few bytes
        assert max(gathered) <= 1536 and (max(gathered) > 1024 or case.tags[c] == "zeros"), c
        assert sum(len(p.delivered) for p in log[c]) == 4 * 16384 > 32768           # through the window twice
        if case.tags[c] == "random":     # stored blocks: every message takes many pieces, a block spans them
            assert len(log[c]) >= 4 * (16384 // 1536) and all(len(p.delivered) <= 1536 for p in log[c])
    most = {k: max(len(p.delivered) for c in range(case.n) if case.tags[c] == k for p in log[c]) for k in C.KINDS}
    assert most["zeros"] == 16384 >= FLUSH_AT and most["json"] > IST, most


@pytest.mark.parametrize("wbits", [9, 10])
def test_small_window_wraps_many_times(wbits):
    case = C.small_window(wbits)
    assert case.n == 70 and case.rig["wbits"] == wbits and case.rig["out_cap"] == 104 and case.step == 100
    assert all(len(m) == 3000 for ms in case.msgs for m in ms)
    assert 4 * 3000 // (1 << wbits) >= 11
    check_residues(case)
    run_model(case)
    check_history_used(case)


def test_one_piece_over_staging_and_ring():
    case = C.over_staging_ring()
    for kind in ("random", "zeros"):
        cs = [c for c in range(case.n) if case.tags[c] == kind]
        assert {case.rig["out_res"][c] for c in cs} == {case.rig["msg_res"][c] for c in cs} == set(range(16)), kind
    log = run_model(case)
    for c in range(case.n):
        big, js, echo = log[c]
        assert [len(log[c]), big.ran, js.ran, echo.ran] == [3, True, True, True]
        assert len(big.delivered) == C.BIG[case.tags[c]] > RING > FLUSH_AT          # one call's output wraps the ring
        if case.tags[c] == "random":
            assert big.in_used > 65535 + IST and (case.pays[c][0][0] >> 1) & 3 == 0  # stored, staged many times over
        else:
            assert len(case.calls[0][c]) < 200
        assert len(js.delivered) == 2000 and len(case.msgs[c][2]) == 1600
        # the echo reaches the window's far end
        assert alone(case.pays[c][2], 1600) != (0, case.msgs[c][2])
        assert case.msgs[c][2][:1000] == (case.msgs[c][0] + case.msgs[c][1])[-32000:-31000]
    # why the echo is there: behind 70 000 random or zero bytes most json messages copy nothing from the window
    assert sum(alone(case.pays[c][1], 2000) == (0, case.msgs[c][1]) for c in range(case.n)) > case.n // 2


def _lies_across(text, s, r, k, seq):
    """seq lies in text k bytes before the boundary of round r, for a piece at residue s"""
    at = C.ROUND * r - s - k
    assert text[at:at + len(seq)] == seq
    assert (at + s + k) % C.ROUND == 0 and (at + s + k) // C.ROUND == r      # byte k is lane 0's first of round r
    assert k == 0 or (at + s) // C.ROUND == r - 1                           # the k bytes before it are lane 63's


@pytest.mark.parametrize("comp", [0, 1])
def test_utf8_over_scan_rounds(comp):
    case = C.utf8_rounds(comp)
    assert case.rig["out_res"] == case.rig["msg_res"] == [s for _, s in case.tags]
    assert case.rig["out_cap"] == C.TEXT_LEN + 4 and case.rig["msg_cap"] == C.TEXT_LEN
    log = run_model(case)
    splits = [(L, k) for L in (2, 3, 4) for k in range(L)]
    seen = collections.Counter()
    for c, ((tag, s), pieces) in enumerate(zip(case.tags, log)):
        name, L, k = tag[:3]
        # the text as the connection's pieces deliver it (an invalid one: as far as the failing piece)
        text = b"".join(p.delivered for p in pieces)
        if name == "valid":
            assert len(pieces) == 1 and len(text) == C.TEXT_LEN
            for r in tag[3]:
                _lies_across(text, s, r, k, C.CP[L])
                seen[("valid", s, L, k, r)] += 1
        elif name == "cut":
            r, j = tag[3:]
            _lies_across(text, s, r, k, C.CP[L])
            assert len(pieces) == 2 and len(pieces[0].delivered) == C.ROUND * r - s - k + j
            assert pieces[0].state[24] == j                       # the carry the first piece leaves
            assert len(pieces[2 - r].delivered) > C.ROUND           # r = 2: left by, r = 1: met by a piece over 1 KiB
            seen[("cut", s, L, k, r, j)] += 1
        else:
            r = tag[3]
            seq = {"cont_ascii": None, "cut_bad": None, "lone": b"\x80"}.get(name, C.BAD_SEQ.get(name))
            if seq is None:
                i = max(k, 1)
                seq = C.CP[L][:i] + b"x" + C.CP[L][i + 1:]
            want_pieces = 2 if name == "cut_bad" else 1
            assert len(pieces) == want_pieces and case.fail_piece[c] == want_pieces - 1
            assert len(text) == C.TEXT_LEN     # a failing piece's bytes are delivered all the same (d_msg_len)
            _lies_across(text, s, r, k, seq)
            if name == "cut_bad":
                assert pieces[0].state[24] == max(k, 1) and len(pieces[2 - r].delivered) > C.ROUND
            seen[(name, s, L, k, r)] += 1
    S, R = range(16), (1, 2)
    want = collections.Counter()
    want.update(("valid", s, L, k, r) for s, (L, k), r in itertools.product(S, splits, R))
    want.update(("cut", s, L, k, r, j) for s, (L, k), r in itertools.product(S, splits, R) for j in range(1, L))
    want.update((name, s, L, k, r) for name in ("cont_ascii", "cut_bad") for s, (L, k), r in itertools.product(S, splits, R))
    want.update(("lone", s, 1, k, r) for s, k, r in itertools.product(S, (0, 1), R))
    want.update((name, s, len(seq), k, r) for name, seq in C.BAD_SEQ.items()
                for s, r in itertools.product(S, R) for k in range(len(seq)))
    assert seen == want
    assert sum(1 for t in seen if t[0] == "valid") == 16 * 9 * 2 == 288
    assert sum(1 for t in seen if t[0] == "cut") == 16 * (2 * 1 + 3 * 2 + 4 * 3) * 2 == 640
    assert len(seen) == 288 + 640 + 2 * 288 + 16 * 2 * (2 + 3 + 3 + 4) and case.n == len(seen) - 144
