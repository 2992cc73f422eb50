"""Batches for the keyed receive path (bpmd_read_batch with masking keys) and
the one runner every test of it goes through.

The builders need neither torch nor HIP: a case is the unmasked payloads, the
keys, text flags, capacities and start alignments, and its expectation is the
oracle's inflate (and UTF-8 verdict) of the unmasked payloads.  run() masks
them (O.mask), lays them out, calls bpmd_read_batch once over prefilled
buffers and returns every difference from that expectation.

    python -m tests.read_keyed_cases keyed|unkeyed

builds queue_batch(4096, 512), runs it once and prints one JSON line; the
knobs that the library reads once per process (BPMD_QUEUE_WGS,
BPMD_INFLATE_BP, BPMD_INFLATE_ORDER) come from the environment of this fresh
process (tests/test_gpu_read_keyed.py::test_queue_plans_in_child).
"""
from __future__ import annotations

import ctypes
import json
import os
import random
import re
import sys
import time
from dataclasses import dataclass, field, replace

import numpy as np

from beast_amd import synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_FRAME_PAYLOAD = 256     # beast_amd.pmd.BAD_FRAME_PAYLOAD (importing pmd imports torch)
SENTINEL = 0x5A5A5A5A       # status / out_len before the call
GUARD = 0xA5                # every byte of the input and output buffers outside a message or slot
FIXED_KEYS = (0, 0xFFFFFFFF, 0x000000FF, 0x0000FF00, 0x00FF0000, 0xFF000000)


def in_cap() -> int:
    """The wave kernel's input window of this build (BPMD_IN_CAP)."""
    m = re.search(r"-DBPMD_IN_CAP=(\d+)", open(os.path.join(ROOT, "beast_amd", "build.py")).read())
    if not m:
        src = open(os.path.join(ROOT, "beast_amd", "csrc", "pmd_inflate.hip")).read()
        m = re.search(r"#define BPMD_IN_CAP (\d+)", src)
    v = int(m.group(1))
    assert v % 4 == 0, v
    return v


@dataclass
class Case:
    payloads: list                 # unmasked permessage-deflate payloads
    caps: list                     # output capacity per message
    keys: list | None = None       # masking key per message
    text: list | None = None       # text flag per message
    aligns: list | None = None     # payload start address mod 16 (None: ragged)
    out_aligns: list | None = None  # output slot address mod 16 (None: ragged)
    raw: bool = False
    info: dict = field(default_factory=dict)


def synth_msg(kind: str, n: int, seed: int) -> bytes:
    d, _, _ = synth.make_batch(kind, [n], seed=seed)
    return bytes(d[:n])


# ------------------------------------------------------------ exact lengths

def stored_payload(n: int, rng) -> bytes:
    """A payload of exactly n compressed bytes: stored blocks of random bytes
    and the header byte of the empty stored block whose 00 00 FF FF is stripped."""
    assert n >= 6
    out, left = b"", n - 1
    while left:
        d = left - 5
        if d > 3000:
            d = rng.randrange(1000, 3001)
            if left - 5 - d < 5:
                d = left - 5
        out += b"\x00" + d.to_bytes(2, "little") + (d ^ 0xFFFF).to_bytes(2, "little") + rng.randbytes(d)
        left -= 5 + d
    out += b"\x00"
    assert len(out) == n
    return out


def truncated(p: bytes, n: int) -> bytes:
    assert n <= len(p)
    return p[:n]


def edge_lengths(cap_in: int) -> list:
    return sorted(set(range(0, 81)) | set(range(cap_in - 8, cap_in + 41)) |
                  set(range(2 * cap_in - 4, 2 * cap_in + 21)))


# ------------------------------------------------------------------ oracle

def oracle_inflate(payloads, caps, raw=False, threads=16):
    """(status, out_len, outputs) of the oracle's inflate of each payload."""
    lens = np.array([len(p) for p in payloads], dtype=np.uint32)
    off = synth.offsets(lens)
    data = np.frombuffer(b"".join(payloads) + b"\0", dtype=np.uint8)
    out, out_off, out_len, status = O.inflate_batch(data, off, lens, np.asarray(caps, dtype=np.uint32), raw=raw,
                                                    threads=threads)
    outs = [out[int(o):int(o) + int(n)].tobytes() for o, n in zip(out_off, out_len)]
    return status, out_len, outs


def oracle_deflate(msgs, level, threads=16):
    lens = np.array([len(m) for m in msgs], dtype=np.uint32)
    off = synth.offsets(lens)
    data = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8)
    out, out_off, out_len, status = O.deflate_batch(data, off, lens, level=level, wbits=15, mem_level=4,
                                                    threads=threads)
    assert not status.any()
    return [out[int(o):int(o) + int(n)].tobytes() for o, n in zip(out_off, out_len)]


def _caps(payloads, bounds, raw, cut=True):
    """The message length (what the oracle produces given room), minus 1 for
    every 7th message, 1 for every 31st."""
    _, full, _ = oracle_inflate(payloads, [max(b, 1) for b in bounds], raw=raw)
    caps = []
    for i, n in enumerate(full):
        c = int(n)
        if cut and i % 7 == 3:
            c -= 1
        if cut and i % 31 == 5:
            c = 1
        caps.append(max(c, 1))
    return caps


def expect(case: Case):
    """Status, length and bytes per message: the oracle on the unmasked payload,
    then the UTF-8 verdict of text messages that inflated with status 0."""
    st, ln, outs = oracle_inflate(case.payloads, case.caps, raw=case.raw)
    st = st.astype(np.int64)
    if case.text is not None:
        for i, t in enumerate(case.text):
            if t and st[i] == 0 and O.utf8_check(outs[i]) != 0:
                st[i] = BAD_FRAME_PAYLOAD
    return st, ln.astype(np.int64), outs


def _cycle_keys(n, rng):
    """0, all ones, the four one-byte keys and three random keys, in turn: a
    one-byte key shows a wrong rotation in a single byte position."""
    return [FIXED_KEYS[i % 9] if i % 9 < 6 else rng.getrandbits(32) for i in range(n)]


# --------------------------------------------------------------- edge grid

def edge_grid(cap_in: int, raw: bool = False, seed: int = 21) -> Case:
    rng = random.Random(seed)
    lengths = edge_lengths(cap_in)
    js = synth_msg("json", 48000, 5)
    dyn = O.pmd_deflate(js, 6, 15, 4)
    assert len(dyn) > lengths[-1], (len(dyn), lengths[-1])
    payloads, bounds, aligns, kinds = [], [], [], []
    for a in range(16):
        for n in lengths:
            if n >= 6:
                payloads.append(stored_payload(n, rng))
                bounds.append(n)
                aligns.append(a)
                kinds.append(("stored", a, n))
            payloads.append(truncated(dyn, n))
            bounds.append(len(js))
            aligns.append(a)
            kinds.append(("truncated", a, n))
    sizes = [0, 1, 3, 15, 64, 255, 1000, 2559, 4096, 5003, 9000, 20000, 40000]
    k = 0
    for kind in ("json", "binary", "zeros", "random"):
        for level, strategy in ((1, 0), (6, 0), (9, 0), (6, 4)):
            for n in sizes:
                m = synth_msg(kind, n, 100 + k)
                payloads.append(O.pmd_deflate(m, level, 15, 4, strategy))
                bounds.append(n)
                aligns.append(k % 16)
                kinds.append((kind, level, strategy, n))
                k += 1
    caps = _caps(payloads, bounds, raw)
    return Case(payloads, caps, keys=_cycle_keys(len(payloads), rng), aligns=aligns, raw=raw,
                info={"kinds": kinds, "whole": k})


# ------------------------------------------------------- lane / wave split

def _flip_second_half(p: bytes, rng) -> bytes:
    q = bytearray(p)
    q[rng.randrange(len(q) // 2, len(q))] ^= 1 << rng.randrange(8)
    return bytes(q)


def _spoil_utf8(m: bytes, rng) -> bytes:
    b = bytearray(m)
    b[rng.randrange(len(b))] = rng.choice([0x80, 0xC0, 0xED, 0xFF])
    return bytes(b)


def _mixed_batch(n_msgs, exact, n_long_min, long_min_len, rng, seed):
    """Short JSON messages, the stored payloads of the lengths `exact`, and long
    binary and JSON payloads (9000 to 70000 bytes, L1 and L6) until n_long_min
    of them have more than long_min_len compressed bytes; eight long and eight
    short payloads with one bit flipped in their second half; a text flag per
    message, a tenth of the text messages spoiled before deflate."""
    msgs, text, level = [], [], []
    n_short = n_msgs - len(exact)
    longs, over, tries = [], 0, 0
    while over < n_long_min:
        assert tries < 2 * n_long_min + 32, (over, tries)
        kind = ("binary", "json")[tries % 2]
        n = rng.randrange(9000, 70001) if kind == "binary" else rng.randrange(40000, 70001)
        lv = (1, 6)[(tries // 2) % 2]
        m = synth_msg(kind, n, seed + tries)
        t = int(kind == "json" and tries % 4 == 1)
        if t and tries % 12 == 1:
            m = _spoil_utf8(m, rng)
        p = O.pmd_deflate(m, lv, 15, 4)
        over += len(p) > long_min_len
        longs.append((p, len(m), t))
        tries += 1
    n_short -= len(longs)
    lens = [rng.randrange(40, 401) for _ in range(n_short)]
    d, off, _ = synth.make_batch("json", lens, seed=seed)
    for i, n in enumerate(lens):
        m = bytes(d[int(off[i]):int(off[i]) + n])
        t = int(rng.random() < 0.6)
        if t and rng.random() < 0.1:
            m = _spoil_utf8(m, rng)
        msgs.append(m)
        text.append(t)
    short = []
    for lv in (1, 6):
        idx = [i for i in range(n_short) if (i % 2 == 0) == (lv == 1)]
        for i, p in zip(idx, oracle_deflate([msgs[i] for i in idx], lv)):
            short.append((i, p))
    short = [p for _, p in sorted(short)]
    items = [(p, len(m), t) for p, m, t in zip(short, msgs, text)]
    for i in rng.sample(range(len(items)), 8):
        items[i] = (_flip_second_half(items[i][0], rng),) + items[i][1:]
    for i in rng.sample(range(len(longs)), 8):
        longs[i] = (_flip_second_half(longs[i][0], rng),) + longs[i][1:]
    items += longs
    items += [(stored_payload(n, rng), n, 0) for n in exact]
    rng.shuffle(items)
    assert len(items) == n_msgs
    payloads = [p for p, _, _ in items]
    caps = _caps(payloads, [b for _, b, _ in items], False, cut=False)
    return Case(payloads, caps, keys=[rng.getrandbits(32) for _ in items], text=[t for _, _, t in items])


def split_batch(n_msgs: int, split: int, rng) -> Case:
    c = _mixed_batch(n_msgs, [split - 1, split, split + 1], 48, split, rng, seed=1000 + split)
    lens = [len(p) for p in c.payloads]
    c.info = {"over": sum(n > split for n in lens), "lens": lens}
    assert c.info["over"] >= 48 and all(lens.count(n) >= 1 for n in (split - 1, split, split + 1))
    return c


def long_threshold(lens, lanes: int) -> int:
    """long_count_kernel for LONG_WAVE_ORDERED(lanes, 4096, 200), in 64-byte keys."""
    thr = max(4096, 200 * sum(lens) // (100 * lanes))
    return (thr + 63) >> 6


def queue_batch(n_msgs: int, lanes: int, rng) -> Case:
    """As split_batch, for the work-queue plan: at least 16 payloads are long
    under long_count_kernel's threshold, and at least 16 of 2048 compressed
    bytes or more are not (stored payloads under the 4096-byte floor)."""
    mid = [rng.randrange(2048, 4000) for _ in range(24)]
    c = _mixed_batch(n_msgs, mid, 32, 12000, rng, seed=2000 + lanes)
    lens = [len(p) for p in c.payloads]
    tk = long_threshold(lens, lanes)
    is_long = [(n >> 6) >= tk for n in lens]
    c.info = {"thr_key": tk, "total": sum(lens), "n_long": sum(is_long),
              "n_mid": sum(n >= 2048 and not g for n, g in zip(lens, is_long))}
    assert c.info["n_long"] >= 16 and c.info["n_mid"] >= 16, c.info
    return c


def lanes_batch(n_msgs: int, rng) -> Case:
    """A batch for the plain lane plan (32 Ki messages or more): 20 to 200 byte
    JSON and 32 long payloads (65536-byte binary at L1 and L6, 30000-byte
    JSON), four of the long ones with a flipped bit."""
    lens = [rng.randrange(20, 201) for _ in range(n_msgs - 32)]
    d, off, _ = synth.make_batch("json", lens, seed=77)
    msgs = [bytes(d[int(off[i]):int(off[i]) + n]) for i, n in enumerate(lens)]
    text = [int(rng.random() < 0.5) for _ in msgs]
    for i in range(0, len(msgs), 19):
        if text[i]:
            msgs[i] = _spoil_utf8(msgs[i], rng)
    items = list(zip(oracle_deflate(msgs, 6), lens, text))
    for j in range(32):
        kind, n, lv = (("binary", 65536, 1), ("binary", 65536, 6), ("json", 30000, 6), ("json", 30000, 1))[j % 4]
        p = O.pmd_deflate(synth_msg(kind, n, 500 + j), lv, 15, 4)
        if j % 8 == 5:
            p = _flip_second_half(p, rng)
        items.append((p, n, int(kind == "json")))
    rng.shuffle(items)
    payloads = [p for p, _, _ in items]
    caps = _caps(payloads, [b for _, b, _ in items], False, cut=False)
    return Case(payloads, caps, keys=[rng.getrandbits(32) for _ in items], text=[t for _, _, t in items])


# -------------------------------------------------------------- UTF-8 edges

_CP = {2: "é".encode(), 3: "語".encode(), 4: "\U0001f600".encode()}


def utf8_edge_cases(n: int = 1100):
    """(alignment, bytes) texts for utf8_kernel's 16-byte units and its 1 KiB
    wave step: ASCII with one code point of 2, 3 or 4 bytes that straddles an
    edge E (a multiple of 16 from the aligned base below the message; 1024 is
    the step at which lane 63 re-reads its look-ahead), and at E = 16, 1024
    and the last edge also one that ends or starts exactly there.  Each
    intact, cut inside the code point (at the edge when it straddles it) and
    with the continuation byte at the edge replaced by 'A'."""
    out = []
    for a in range(16):
        edges = list(range(16, a + n - 4, 16))
        for w in (2, 3, 4):
            for E in edges:
                touch = E in (16, 1024, edges[-1])
                for s in range(E - w if touch else E - w + 1, (E if touch else E - 1) + 1):
                    o = s - a
                    if o < 0:
                        continue
                    t = bytearray(b"a" * n)
                    t[o:o + w] = _CP[w]
                    j = max(1, min(w - 1, E - s))
                    bad = bytearray(t)
                    bad[o + j] = 0x41
                    out += [(a, bytes(t)), (a, bytes(t[:o + j])), (a, bytes(bad))]
    return out


# ------------------------------------------------------------------ layout

def layout(msgs, aligns, rng, fill=GUARD):
    """Messages at the given start alignments (mod 16; None: wherever the
    guard leaves them) with 0 to 19 guard bytes and the alignment gap between."""
    offs, pos = [], 0
    for i, m in enumerate(msgs):
        pos += rng.randrange(0, 20)
        if aligns is not None:
            pos += (aligns[i] - pos) % 16
        offs.append(pos)
        pos += len(m)
    buf = bytearray([fill]) * (pos + 64)
    for o, m in zip(offs, msgs):
        buf[o:o + len(m)] = m
    return bytes(buf), offs


# ------------------------------------------------------------------ runner

@dataclass
class Run:
    rc: int
    status: np.ndarray
    out_len: np.ndarray
    outs: list
    bad: list     # every difference from the expectation, as short strings


def run(case: Case, want=None, seed: int = 1) -> Run:
    """One bpmd_read_batch call over prefilled buffers: status and out_len hold
    SENTINEL, the output GUARD, slots 0 to 19 guard bytes apart.  Checks that
    no sentinel is left, nothing outside a slot or in the input changed, and
    status, length and bytes equal `want` (default expect(case))."""
    import torch
    from beast_amd import pmd
    L = pmd.lib()
    rng = random.Random(seed)
    n = len(case.payloads)
    want = want if want is not None else expect(case)
    wire = case.payloads if case.keys is None else [O.mask(p, k) for p, k in zip(case.payloads, case.keys)]
    buf, offs = layout(wire, case.aligns, rng)
    # slots of `cap` bytes; the decoders may use a whole slot, never a byte outside
    slots = [bytes(c) for c in case.caps]
    obuf, out_off = layout(slots, case.out_aligns, rng)
    inside = np.frombuffer(obuf, dtype=np.uint8) == 0

    def dev(a, dt):
        return torch.from_numpy(np.asarray(a, dtype=dt)).cuda()

    data = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    off, ln, cap = dev(offs, np.int64), dev([len(p) for p in wire], np.int32), dev(case.caps, np.int32)
    ooff = dev(out_off, np.int64)
    key = None if case.keys is None else dev(np.array(case.keys, dtype=np.uint32).view(np.int32), np.int32)
    text = None if case.text is None else dev(case.text, np.uint8)
    out = torch.full((len(obuf),), GUARD, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    out_len = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    cfg = pmd._Cfg(0, 15, 8, 0, pmd.F_RAW if case.raw else 0)
    p = pmd._ptr
    rc = L.bpmd_read_batch(ctypes.byref(cfg), p(data), p(off), p(ln), pmd._optr(key), pmd._optr(text), n, p(out),
                           p(ooff), p(cap), p(out_len), p(status), pmd._stream_handle(None))
    torch.cuda.synchronize()
    st, ol, o = status.cpu().numpy().astype(np.int64), out_len.cpu().numpy().astype(np.int64), out.cpu().numpy()
    bad = []
    if rc != 0:
        bad.append(f"bpmd_read_batch returned {rc}")
    if data.cpu().numpy().tobytes() != buf:
        bad.append("input buffer changed")
    for i in np.nonzero((st == SENTINEL) | (ol == SENTINEL))[0][:8]:
        bad.append(f"message {i}: no decoder wrote status / out_len")
    stray = np.nonzero(~inside & (o != GUARD))[0]
    if len(stray):
        bad.append(f"{len(stray)} bytes outside every slot changed, first at {int(stray[0])}")
    wst, wln, wouts = want
    outs = []
    for i in range(n):
        k = int(ol[i]) if 0 <= ol[i] <= case.caps[i] else 0
        outs.append(o[out_off[i]:out_off[i] + k].tobytes())
        if st[i] != wst[i] or ol[i] != wln[i] or outs[i] != wouts[i]:
            if len(bad) < 24:
                d = next((j for j, (x, y) in enumerate(zip(outs[i], wouts[i])) if x != y), None)
                bad.append(f"message {i} (in_len {len(wire[i])}, in_off%16 {offs[i] % 16}, cap {case.caps[i]}, "
                           f"key {case.keys[i] if case.keys else None}): status {st[i]} want {wst[i]}, "
                           f"out_len {ol[i]} want {wln[i]}, first byte differing {d}")
    return Run(rc, st, ol, outs, bad)


def unkeyed(case: Case) -> Case:
    return replace(case, keys=None)


def main(argv) -> int:
    which = argv[1] if len(argv) > 1 else ""
    if which not in ("keyed", "unkeyed"):
        print("usage: python -m tests.read_keyed_cases keyed|unkeyed", file=sys.stderr)
        return 2
    t0 = time.time()
    case = queue_batch(4096, 512, random.Random(41))
    if which == "unkeyed":
        case = unkeyed(case)
    t1 = time.time()
    r = run(case)
    print(json.dumps({"case": which, "n": len(case.payloads), "n_long": case.info["n_long"],
                      "n_mid": case.info["n_mid"], "nonzero_status": int((r.status != 0).sum()),
                      "mismatches": len(r.bad), "first_mismatch": r.bad[0] if r.bad else None,
                      "build_s": round(t1 - t0, 2), "run_s": round(time.time() - t1, 2)}))
    return 1 if r.bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
