"""Shared inputs of the context-takeover tests (tests/test_model.py on the
CPU, tests/test_gpu_takeover.py on the GPU): the same message sets feed the
host model's discrimination check and the kernel's byte comparison, so what
the former proves holds for the latter."""
import random
import zlib

import numpy as np

from beast_amd import synth

# both sides of one chunk (4096) and of half a chunk, tiny, empty, multi-chunk
LENS = (0, 1, 3, 300, 2047, 2048, 2049, 4095, 4096, 4097, 6000, 9000)
DEFLATE_CASES = [(0, 15), (1, 15), (6, 15), (9, 15), (6, 10), (9, 9)]
# periods on both sides of max_dist = 2^wbits - 262 for windowBits 9 (250) and
# 10 (762) and of the 2048- and 4096-byte chunk histories
PERIODS = (100, 250, 251, 300, 700, 762, 763, 2047, 2048, 2049, 4096, 5000)
DEFLATE_HIST = 4096      # pmd.TakeoverDeflater.HIST
MAX_MSG = 9000
# drawn more often, so that a connection's 2 * 4096 + 9000 bytes fill up and slide
LONG = (6000, 9000, 9000, 9000)


def round_conns(rng, n_conn, rounds, idle=3):
    """Per round, a random permutation of a random subset of the connections:
    at least one in `idle` sits the round out, so connections get out of step."""
    active = n_conn - (n_conn + idle - 1) // idle
    return [rng.sample(range(n_conn), rng.randrange(active - active // 8, active + 1)) for _ in range(rounds)]


def schedule(rng, counts):
    """Rounds of such subsets until connection c has had counts[c] turns."""
    left, out = list(counts), []
    while any(left):
        live = [c for c in range(len(left)) if left[c]]
        cr = rng.sample(live, max(1, len(live) * 2 // 3))
        for c in cr:
            left[c] -= 1
        out.append(cr)
    return out


def connection_messages(c, lens, wbits, seed=0):
    """Connection c's messages of the given lengths: JSON or corpus1 at
    windowBits 15, consecutive pieces of a periodic text below that."""
    if wbits == 15:
        kind = ("json", "corpus1")[c % 2]
        return [bytes(synth.make_batch(kind, [n], seed=seed + c * 131 + k)[0][:n]) for k, n in enumerate(lens)]
    from tests.deflate_scripts import periodic
    text = periodic(PERIODS[c % len(PERIODS)], sum(lens), seed=c % 5)
    cuts = np.concatenate([[0], np.cumsum(lens)]).tolist()
    return [text[a:b] for a, b in zip(cuts, cuts[1:])]


def deflate_set(wbits, n_conn=96, rounds=6, seed=77):
    """(conns, msgs): conns[r] the connections of round r in submission order,
    msgs[c] connection c's messages in the order it sends them (one per round
    it takes part in).  The schedule does not depend on the level."""
    rng = random.Random(seed)
    conns = round_conns(rng, n_conn, rounds)
    count = [sum(c in cr for cr in conns) for c in range(n_conn)]
    lens = [[rng.choice(LENS + LONG) for _ in range(count[c])] for c in range(n_conn)]
    return conns, [connection_messages(c, lens[c], wbits, seed) for c in range(n_conn)]


def stream_cuts(msgs):
    """(plaintext, cuts) of one connection: message k is plain[cuts[k]:cuts[k+1]]."""
    cuts = [0]
    for m in msgs:
        cuts.append(cuts[-1] + len(m))
    return b"".join(msgs), cuts


def slides(lens, slot, keep):
    """How often a connection's buffer slides (pmd.TakeoverDeflater.deflate's
    rule: before a message that does not fit after the earlier plaintext)."""
    pos = n = 0
    for ln in lens:
        if pos + ln > slot:
            pos = min(pos, keep)
            n += 1
        pos += ln
    return n


def takeover_slot(keep, max_msg):
    return (2 * keep + max_msg + 15) // 16 * 16


def json_message(n, seed):
    return bytes(synth.make_batch("json", [n], seed=seed)[0][:n])


def random_message(n, seed):
    return bytes(synth.make_batch("random", [n], seed=seed)[0][:n])


# ---------------------------------------------------------------- inflate side

STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)


def zlib_stream(msgs, level, wbits, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    """permessage-deflate payloads of one connection from CPython's zlib: one
    raw deflate stream, Z_SYNC_FLUSH per message, 00 00 FF FF stripped."""
    z = zlib.compressobj(level, zlib.DEFLATED, -wbits, mem_level, strategy)
    out = []
    for m in msgs:
        p = z.compress(m) + z.flush(zlib.Z_SYNC_FLUSH)
        assert p.endswith(b"\x00\x00\xff\xff")
        out.append(p[:-4])
    return out


FOREIGN_SIZES = (0, 1, 2, 5, 9, 300, 4096, 9000, 40000, 65536)


def foreign_set(n_conn=60, rounds=8, seed=9):
    """[(wbits, msgs, payloads)] per connection: CPython zlib streams with
    random windowBits 9..15, level, memLevel and strategy."""
    rng = random.Random(seed)
    out = []
    for c in range(n_conn):
        wbits, level, mem = rng.randrange(9, 16), rng.randrange(0, 10), rng.randrange(1, 10)
        strategy = STRATEGIES[c % 5]
        kind = ("json", "corpus1", "binary")[c % 3]
        sizes = [rng.choice(FOREIGN_SIZES) for _ in range(rounds)]
        msgs = [bytes(synth.make_batch(kind, [n], seed=seed + c * 31 + r)[0][:n]) for r, n in enumerate(sizes)]
        out.append((wbits, msgs, zlib_stream(msgs, level, wbits, mem, strategy)))
    return out


def tiny_history_set(pieces=16):
    """[(msgs, payloads)]: texts of period 1..9 cut into pieces of 3, 4, 5 and
    7 bytes (CPython level 9): from the second piece on, matches reach a few
    bytes back into a history shorter than the expander's 8-byte look-back."""
    out = []
    for period in range(1, 10):
        unit = bytes((37 * period + 11 * i) % 251 for i in range(period))
        for piece in (3, 4, 5, 7):
            text = (unit * (pieces * piece // period + 1))[:pieces * piece]
            msgs = [text[i * piece:(i + 1) * piece] for i in range(pieces)]
            out.append((msgs, zlib_stream(msgs, 9, 15)))
    return out
