"""CPU: the host model of the GPU deflate algorithm (tests/model) produces
payloads that Beast's inflate (oracle restatement) decodes back to the
message, within the size tolerance the GPU tests apply.  This pins the
algorithm the kernel is compared against byte for byte."""
import numpy as np
import pytest

from beast_amd import synth
from oracle import oracle as O
from tests.model import model as M
from tests import takeover_cases as TC


def _run(kind, sizes, level=6, wbits=15, strategy=0, seed=1):
    lens = np.array(sizes, dtype=np.uint32)
    data, off, ln = synth.make_batch(kind, lens, seed=seed)
    pl = M.encode(data, off, ln, level=level, wbits=wbits, strategy=strategy)
    msgs = [bytes(data[int(off[i]):int(off[i]) + int(ln[i])]) for i in range(len(sizes))]
    for i, m in enumerate(msgs):
        st, out = O.pmd_inflate(pl[i], cap=max(len(m), 1), wbits=wbits)
        assert st == 0 and out == m, (kind, sizes[i], level, strategy, O.ERRORS[st])
        assert len(pl[i]) <= O.upper_bound(len(m))
    return msgs, pl


@pytest.mark.parametrize("level", range(10))
def test_model_roundtrip_levels(level):
    for kind in ("json", "corpus1", "random", "binary", "zeros"):
        _run(kind, [0, 1, 3, 100, 4096, 4097, 20000], level=level, seed=level)


@pytest.mark.parametrize("strategy", range(5))
def test_model_roundtrip_strategies(strategy):
    for kind in ("json", "binary", "zeros"):
        _run(kind, [0, 2, 300, 4096, 9000], strategy=strategy, seed=strategy)


@pytest.mark.parametrize("wbits", [8, 9, 12, 15])
def test_model_roundtrip_window_bits(wbits):
    _run("json", [5000, 30000], level=9, wbits=wbits)


def test_model_size_within_tolerance_of_beast():
    msgs, pl = _run("json", [4096] * 256, level=6, seed=0x5EED0003)
    ours = sum(len(p) for p in pl)
    beast = sum(len(O.pmd_deflate(m, 6, 15, 4)) for m in msgs)
    assert ours <= 1.10 * beast, ours / beast


def test_runwise_code_length_coding_equals_serial_state_machine():
    """The kernel codes code-length runs independently (lz::rle_run); it must
    reproduce the reference's scan_tree/send_tree state machine
    (deflate_stream.ipp:978-1110) symbol for symbol."""
    import ctypes
    import random
    L = M.lib()
    rng = random.Random(3)
    out1 = (ctypes.c_uint32 * 400)()
    out2 = (ctypes.c_uint32 * 400)()
    na, nb = ctypes.c_int(), ctypes.c_int()
    for trial in range(3000):
        n = rng.randrange(1, 320)
        mode = trial % 3
        if mode == 0:
            lens = [rng.choice([0, 0, 0, 5, 6, 7, 8]) for _ in range(n)]
        elif mode == 1:
            lens = []
            while len(lens) < n:
                lens += [rng.randrange(0, 16)] * rng.randrange(1, 160)
            lens = lens[:n]
        else:
            lens = [rng.randrange(0, 16) for _ in range(n)]
        buf = (ctypes.c_uint8 * n)(*lens)
        ok = L.dmodel_rle_check(buf, n, out1, out2, ctypes.byref(na), ctypes.byref(nb))
        assert ok == 1, (lens, na.value, nb.value)


def _slightly_compressible(n, seed, frac):
    # random bytes; a fraction of the 64-byte units copies 16-47 bytes from up
    # to 1.5 KiB back (inside a chunk's 2 KiB history), like C5's binary kind
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, n, dtype=np.uint8)
    for p in range(64, n, 64):
        if rng.random() < frac:
            span = int(rng.integers(16, 48))
            back = int(rng.integers(span, min(p, 1500) + 1))
            d[p:p + span] = d[p - back:p - back + span]
    return d


def test_minimum_gain_for_chunks_of_long_messages():
    """lz::chunk_stored (lz_core.h, BPMD_MIN_GAIN_SHIFT 4): a Huffman chunk of a
    multi-chunk message must save 1/16 of its bytes, else it is stored; a
    one-chunk message keeps Beast's rule (tr_flush_block,
    deflate_stream.ipp:1478: any saving keeps the Huffman block)."""
    data = _slightly_compressible(16384, 3, 1 / 16)
    (multi,) = M.encode(data, [0], [16384], level=1)
    st, out = O.pmd_inflate(multi, cap=16384)
    assert st == 0 and out == data.tobytes()
    assert len(multi) >= 16384   # every chunk saved < 256 bytes: all stored
    single = [M.encode(data[i * 4096:(i + 1) * 4096], [0], [4096], level=1)[0] for i in range(4)]
    assert sum(len(s) < 4096 for s in single) >= 2   # the same chunks alone: Huffman blocks
    # chunks that save more than 1/16 keep their Huffman blocks
    data = _slightly_compressible(16384, 3, 1 / 4)
    (multi,) = M.encode(data, [0], [16384], level=1)
    st, out = O.pmd_inflate(multi, cap=16384)
    assert st == 0 and out == data.tobytes()
    assert len(multi) < 16384 * 15 // 16 + 64


# ---------------------------------------------------------------------------
# History before a message (context takeover): model.encode(..., hist=...)

def test_model_without_history_is_unchanged():
    """Giving encode() a history argument changed nothing for plain batches:
    the payloads of this file's round-trip inputs hash to the digest taken
    from the model before the argument was added."""
    import hashlib
    h = hashlib.sha256()

    def run(kind, sizes, level=6, wbits=15, strategy=0, seed=1):
        data, off, ln = synth.make_batch(kind, np.array(sizes, dtype=np.uint32), seed=seed)
        for p in M.encode(data, off, ln, level=level, wbits=wbits, strategy=strategy):
            h.update(len(p).to_bytes(4, "little"))
            h.update(p)
    for level in range(10):
        for kind in ("json", "corpus1", "random", "binary", "zeros"):
            run(kind, [0, 1, 3, 100, 4096, 4097, 20000], level=level, seed=level)
    for strategy in range(5):
        for kind in ("json", "binary", "zeros"):
            run(kind, [0, 2, 300, 4096, 9000], strategy=strategy, seed=strategy)
    for wbits in (8, 9, 12, 15):
        run("json", [5000, 30000], level=9, wbits=wbits)
    assert h.hexdigest() == "ce795c5fb28634111fefa4f8293e2f5df5423471d730487767eccb602b2c3d60"


def _stream_payloads(msgs, level, wbits, **kw):
    plain, cuts = TC.stream_cuts(msgs)
    return M.encode_stream(plain, cuts, level, wbits, hist_cap=kw.pop("hist_cap", TC.DEFLATE_HIST), **kw)


@pytest.mark.parametrize("level,wbits", [(0, 15), (1, 15), (6, 15), (9, 15), (6, 9), (9, 9), (6, 10), (9, 10)])
def test_model_takeover_streams_inflate(level, wbits):
    """Every connection's model payloads, through one inflater that keeps its
    window at the deflater's windowBits, give back the messages."""
    _, msgs = TC.deflate_set(wbits, n_conn=48)
    assert any(len(m) == 0 for ms in msgs for m in ms) and any(len(m) > 8192 for ms in msgs for m in ms)
    for c, ms in enumerate(msgs):
        got = O.pmd_inflate_stream(_stream_payloads(ms, level, wbits), cap=TC.MAX_MSG, wbits=wbits)
        assert [g[0] for g in got] == [0] * len(ms), (c, [O.ERRORS[g[0]] for g in got])
        assert [g[1] for g in got] == ms, c


def test_model_history_is_clamped_to_the_chunk_history():
    """min(hist_len, chunk_hist(level)): more history than the level's window
    gives the bytes of exactly that much; an empty message is the one-byte
    tail whatever lies before it."""
    text = TC.json_message(12000, 5)
    for level, H in ((6, 2048), (9, 4096)):
        assert M.lib().dmodel_chunk_hist(level) == H
        data = np.frombuffer(text, dtype=np.uint8)
        (a,) = M.encode(data, [6000], [5000], level=level, hist=[6000])
        (b,) = M.encode(data, [6000], [5000], level=level, hist=[H])
        (c,) = M.encode(data, [6000], [5000], level=level, hist=[H // 2])
        (d,) = M.encode(data[6000 - H:], [H], [5000], level=level, hist=[H])
        assert a == b == d
        assert c != b   # (the clamp is not a no-op: half the history changes the bytes)
        assert M.encode(data, [6000], [0], level=level, hist=[4096]) == [b"\x00"]


# the single-chunk and multi-chunk chain limits (lz::gpu_chain): equal at the
# levels whose table value is within both caps
def _chain_caps(level):
    table = {1: 4, 6: 128, 9: 4096}[level]   # deflate_stream.ipp get_config: max_chain
    return min(table, 4), min(table, 32)


@pytest.mark.parametrize("level,wbits", TC.DEFLATE_CASES)
def test_takeover_inputs_tell_wrong_models_apart(level, wbits):
    """The message sets of test_takeover_deflate_equals_model
    (tests/test_gpu_takeover.py) discriminate: a model with the history forced
    to 0 (A), with the single-chunk chain cap (B), or with segment floor 16
    for a first chunk with history (C) differs from the right one on some
    message of each set -- so the GPU's byte comparison would notice a kernel
    with that mistake.  Level 0 stores every byte and has nothing to get
    wrong here; B cannot differ where both caps exceed the level's chain
    limit (level 1: 4)."""
    _, msgs = TC.deflate_set(wbits)
    sets = [ms for ms in msgs if ms]
    cap = TC.json_message(8000, 3)
    sets.append([cap[:3000], cap[3000:]])   # test_takeover_deflate_capacity_sweep's message and history
    right = [_stream_payloads(ms, level, wbits) for ms in sets]
    wrong_a = [_stream_payloads(ms, level, wbits, hist_cap=0) for ms in sets]
    wrong_c = [_stream_payloads(ms, level, wbits, min_seg_hist=16) for ms in sets]
    if level == 0:
        assert wrong_a == right and wrong_c == right
        return
    assert wrong_a != right and wrong_c != right
    single, multi = _chain_caps(level)
    wrong_b = [_stream_payloads(ms, level, wbits, chain_cap=single) for ms in sets]
    assert (wrong_b != right) == (single != multi)
    # the capacity sweep's own message tells A and B apart (C cannot show on
    # it: a first chunk of 2048 bytes or more has segments of 32 or more)
    assert wrong_a[-1] != right[-1] and (wrong_b[-1] != right[-1]) == (single != multi)


def test_model_takeover_size_within_tolerance_of_beast():
    """256 connections x 8 JSON messages of 1 KiB at level 6: the takeover
    model's bytes against Beast's deflater kept across the messages."""
    ours = beast = 0
    for c in range(256):
        ms = [TC.json_message(1024, 0x5EED0000 + c * 8 + r) for r in range(8)]
        ours += sum(len(p) for p in _stream_payloads(ms, 6, 15))
        beast += sum(len(p) for p in O.pmd_deflate_stream(ms, 6, 15, 4))
    print("takeover model / Beast: %.4f" % (ours / beast))
    assert ours <= 1.10 * beast, ours / beast
