"""Shared inputs of the long-message tests of bpmd_receive_pieces_batch
(tests/test_receive_pieces_cases.py on the CPU, tests/test_gpu_receive_pieces.py
on the GPU): the same wires feed the model's own checks of the inputs and the
kernels' comparison with the model, so what the former proves about a case
holds for the latter.  HIP-free.

  long_messages      70 kept-context connections, four 16 KiB messages each,
                     the wire handed over through a 1 536-byte read buffer
  small_window       the same at window bits 9 or 10 with 3 000-byte messages
                     in 100-byte pieces: the window wraps about twenty times
  over_staging_ring  one piece larger than the inflater's 4 KiB input staging
                     and than its 64 KiB output ring, then matches into the
                     window such a call leaves
  utf8_rounds        code points, valid and not, across the 1 024-byte rounds
                     of the finish kernel's UTF-8 scan at every start residue

drive and play run a case on anything with Rig's interface (n, call(wires,
msg_cap)): the GPU test's Rig, or ModelRig here, which is the model alone.  A
case is built once per run and never changed by what runs it."""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass, field

from beast_amd import synth
from oracle import oracle as O
from tests import frame_parse_model as FM
from tests import receive_pieces_model as M

SERVER, CLIENT = FM.SERVER, FM.CLIENT
EV = {FM.EV_PING: "ping", FM.EV_PONG: "pong", FM.EV_CLOSE: "close"}
KINDS = ("json", "binary", "random", "corpus1", "zeros")
READ_BUFFER = 1536      # Beast's default read buffer (stream_impl.hpp: tcp_frame_size)
ROUND = 1024            # utf8_scan and piece_copy_xor: 64 lanes x 16 bytes per round


def message(kind, n, seed):
    return bytes(synth.make_batch(kind, [n], seed=seed)[0][:n])


def drive(rig, wires, steps, msg_cap=None, buf=None):
    """Connection i gets steps[i] more bytes of wires[i] per call until it has
    taken them all or failed; with buf, never more than buf bytes in one call
    (a read buffer of that size).  Returns per connection its pieces."""
    n = rig.n
    steps = [steps] * n if isinstance(steps, int) else steps
    fed, used, done, log = [0] * n, [0] * n, [False] * n, [[] for _ in range(n)]
    while not all(done):
        chunk = []
        for i in range(n):
            if not done[i]:
                fed[i] = min(len(wires[i]), fed[i] + steps[i])
                if buf:
                    fed[i] = min(fed[i], used[i] + buf)
            chunk.append(b"" if done[i] else wires[i][used[i]:fed[i]])
        for i, p in enumerate(rig.call(chunk, msg_cap)):
            if done[i]:
                continue
            used[i] += p.stop.consumed
            log[i].append(p)
            stuck = fed[i] == len(wires[i]) and p.stop.consumed == 0 and p.stop.event == FM.EV_NEED_MORE
            done[i] = bool(p.status) or used[i] == len(wires[i]) or stuck
    return log


def play(rig, calls, msg_caps=None):
    """calls[t][i] is what connection i is handed in call t, whole (every call
    must take all it is given); a connection that failed gets nothing more.
    Returns per connection its pieces, idle calls left out."""
    log, dead = [[] for _ in range(rig.n)], [False] * rig.n
    for t, row in enumerate(calls):
        ps = rig.call(row, None if msg_caps is None else msg_caps[t])
        for i, p in enumerate(ps):
            if dead[i] or not row[i]:
                continue
            assert p.status or p.stop.consumed == len(row[i]), (t, i)
            log[i].append(p)
            dead[i] = bool(p.status)
    return log


def events(pieces):
    """what a connection's pieces amount to: [("message", op, compressed, bytes) | ("ping", payload) | ("error", status)]"""
    out, cur = [], b""
    for p in pieces:
        cur += p.delivered
        if p.status:
            out.append(("error", p.status))
            break
        if p.stop.event == FM.EV_MESSAGE:
            out.append(("message", p.stop.op, p.stop.compressed, cur))
            cur = b""
        elif p.stop.event != FM.EV_NEED_MORE:
            out.append((EV[p.stop.event], p.stop.ctl))
    return out


class ModelRig:
    """Rig's interface on the model alone: what the GPU test compares the kernels with"""

    def __init__(self, n, role, wbits=15, out_cap=64, msg_cap=4096, **_layout):
        lst = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n  # noqa: E731
        self.n, self.out_cap, self.msg_cap = n, lst(out_cap), lst(msg_cap)
        self.conns = [M.Conn(role, wbits) for _ in range(n)]
        self.dead = [False] * n

    def call(self, wires, msg_cap=None):
        n = self.n
        msg_cap = self.msg_cap if msg_cap is None else ([msg_cap] * n if isinstance(msg_cap, int) else list(msg_cap))
        assert all(a <= b for a, b in zip(msg_cap, self.msg_cap))
        ps = [None if self.dead[i] else self.conns[i].call(bytes(wires[i]), self.out_cap[i], msg_cap[i]) for i in range(n)]
        for i, p in enumerate(ps):
            if p is not None and p.status:
                self.dead[i] = True
        return ps


@dataclass
class Case:
    """n connections: the Rig they need, the wire they get and what it must amount to"""
    n: int
    role: int
    rig: dict                                    # Rig's keyword arguments
    want: list                                   # per connection, events() of its pieces
    wires: list = None                           # drive: per connection its whole wire, ...
    step: int = 0                                # ... handed over `step` bytes a call through a buffer of `buf`
    buf: int = None
    calls: list = None                           # play: per call, per connection
    msg_caps: list = None                        # play: d_msg_cap per call
    msgs: list = field(default_factory=list)     # per connection its messages
    pays: list = field(default_factory=list)     # per connection their payloads, one deflate history
    tags: list = field(default_factory=list)     # per connection, what the case is there for
    fail_piece: list = None                      # per connection: the piece that must fail, None = none

    def run(self, rig):
        if self.calls is not None:
            return play(rig, self.calls, self.msg_caps)
        return drive(rig, self.wires, self.step, buf=self.buf)


def _residues(n):
    """out, wire and message slots: each covers every residue mod 16, in different orders"""
    return dict(out_res=[c % 16 for c in range(n)], wire_res=[(c // 16 + 3 * c) % 16 for c in range(n)],
                msg_res=[(5 * c + 3) % 16 for c in range(n)])


def _kept_context(n, size, wbits, step, kind_of, seed):
    rng = random.Random(seed)
    msgs, pays, wires, want, tags = [], [], [], [], []
    for c in range(n):
        kind = kind_of(c)
        ms = [message(kind, size, seed * 1000 + 17 * c + k) for k in range(4)]
        ps = O.pmd_deflate_stream(ms, 6, wbits, 4)
        ops = [1 + (k & 1) if kind == "json" else 2 for k in range(4)]
        wires.append(b"".join(FM.frame(p, op, True, 4, rng.getrandbits(32)) for p, op in zip(ps, ops)))
        want.append([("message", op, 1, m) for m, op in zip(ms, ops)])
        msgs.append(ms), pays.append(ps), tags.append(kind)
    rig = dict(wbits=wbits, out_cap=step + 4, msg_cap=size, **_residues(n))
    return Case(n, SERVER, rig, want, wires=wires, step=step, buf=step, msgs=msgs, pays=pays, tags=tags)


@functools.lru_cache(maxsize=None)
def long_messages(n=70):
    """connection c: four 16 384-byte messages of kind KINDS[c % 5], one deflate
    history, one masked frame each (json alternating text and binary), through
    a 1 536-byte read buffer into out slots of 1 540 bytes: every connection
    inflates 64 KiB through a 32 KiB window, random's stored blocks span pieces"""
    return _kept_context(n, 16384, 15, READ_BUFFER, lambda c: KINDS[c % 5], 41)


@functools.lru_cache(maxsize=None)
def small_window(wbits, n=70):
    """four 3 000-byte json messages per connection at window bits 9 or 10 in
    100-byte pieces: 12 000 bytes through a window of 512 or 1 024"""
    return _kept_context(n, 3000, wbits, 100, lambda c: "json", 43 + wbits)


BIG = {"random": 70000, "zeros": 100000}


@functools.lru_cache(maxsize=None)
def over_staging_ring(n=32):
    """connection c sends, each as one masked frame taken in one call: a
    70 000-byte random message (c even: stored blocks, 70 KB of input staged
    from a misaligned slot, output that wraps the 64 KiB ring) or a 100 000-byte
    zeros message (c odd: under 200 wire bytes give more than FLUSH_AT and more
    than the ring); a 2 000-byte json message; and an echo of 1 600 bytes of the
    connection's text from 32 000 and from 1 900 bytes back -- a 2 000-byte json
    message behind 70 000 random or zero bytes finds next to nothing to copy in
    the window, the echo's matches do reach the window the long call wrote
    back, almost to its far edge.  Both kinds sit at every residue of the out slot and
    the message slot; d_msg_cap is each message's length."""
    rng = random.Random(47)
    msgs, pays, want, tags, frames = [], [], [], [], []
    for c in range(n):
        kind = ("random", "zeros")[c & 1]
        big, js = message(kind, BIG[kind], 4700 + c), message("json", 2000, 4800 + c)
        text = big + js
        ms = [big, js, text[-32000:-31000] + text[-1900:-1300]]
        ps = O.pmd_deflate_stream(ms, 6, 15, 4)
        ops = [2, 1, 2]
        frames.append([FM.frame(p, op, True, 4, rng.getrandbits(32)) for p, op in zip(ps, ops)])
        want.append([("message", op, 1, m) for m, op in zip(ms, ops)])
        msgs.append(ms), pays.append(ps), tags.append(kind)
    wire_max = max(len(f) for fs in frames for f in fs)
    rig = dict(wbits=15, out_cap=wire_max + 4, msg_cap=[BIG[t] for t in tags], out_res=[(c >> 1) % 16 for c in range(n)],
               wire_res=[(c // 16 + 3 * c) % 16 for c in range(n)], msg_res=[(5 * (c >> 1) + 3) % 16 for c in range(n)])
    calls = [[frames[c][t] for c in range(n)] for t in range(3)]
    msg_caps = [[len(msgs[c][t]) for c in range(n)] for t in range(3)]
    return Case(n, SERVER, rig, want, calls=calls, msg_caps=msg_caps, msgs=msgs, pays=pays, tags=tags)


# ---------------------------------------------------------------- UTF-8 across the scan's rounds

TEXT_LEN = 2600
FILL = b"pack my box with five dozen liquor jugs; "
CP = {2: "é".encode(), 3: "€".encode(), 4: "\U0001f600".encode()}
# the invalid sequences (utf8_checker.ipp's valid()): overlong, surrogate, above U+10FFFF
BAD_SEQ = {"overlong": b"\xe0\x80\x80", "surrogate": b"\xed\xa0\x80", "over_10ffff": b"\xf4\x90\x80\x80"}


def boundary(s, r):
    """the piece offset where lane 0 of round r takes over from lane 63 of round
    r - 1, for a piece that starts at residue s mod 16"""
    return ROUND * r - s


def utf8_text(s, put):
    """TEXT_LEN bytes of ASCII filler with put = [(r, k, bytes)]: the bytes lie
    k bytes before boundary(s, r)"""
    t = bytearray((FILL * (TEXT_LEN // len(FILL) + 1))[:TEXT_LEN])
    for r, k, b in put:
        at = boundary(s, r) - k
        t[at:at + len(b)] = b
    return bytes(t)


def _deliver(text, cut, comp, key):
    """(first call, second call) that deliver text in one piece (cut None) or as text[:cut] and text[cut:]"""
    rsv = 4 if comp else 0
    if cut is None:
        return FM.frame(O.pmd_deflate(text) if comp else text, 1, True, rsv, key()), b""
    if comp:
        a, b = M.deflate_chunks([text[:cut], text[cut:]])
        b = b[:-4]
    else:
        a, b = text[:cut], text[cut:]
    return FM.frame(a, 1, False, rsv, key()), FM.frame(b, 0, True, 0, key())


@functools.lru_cache(maxsize=None)
def utf8_rounds(comp):
    """One text message per connection, plain (comp 0: the piece lies in the
    out slot) or compressed (comp 1: in the message slot), the slot at residue s:

      valid    (s, L, k): a code point of L bytes k bytes before each of the
               two boundaries -- every split of every length between lane 63
               of one round and lane 0 of the next -- in one piece of 2 600
      cut      (s, L, k, r, j): the same text in two pieces cut j bytes into
               the code point at boundary r: a piece over 1 KiB leaves a carry
               (r = 2) or meets one (r = 1)
      cont_ascii, lone, overlong, surrogate, over_10ffff  (s, ..., k, r): the
               text made invalid k bytes before boundary r; in one piece
      cut_bad  (s, L, k, r): the continuation byte behind the cut replaced by
               ASCII: the first piece is fine, the second fails on its carry"""
    rng = random.Random(53 + comp)
    key = lambda: rng.getrandbits(32)  # noqa: E731
    rows, tags, want, fail = [], [], [], []

    def add(tag, s, text, cut, fail_piece):
        rows.append(_deliver(text, cut, comp, key))
        tags.append((tag, s))
        want.append([("error", M.BAD_FRAME_PAYLOAD)] if fail_piece is not None else [("message", 1, comp, text)])
        fail.append(fail_piece)

    other = lambda r: (3 - r, 1, CP[3])  # noqa: E731  (a valid split code point at the other boundary)
    for s in range(16):
        for L in (2, 3, 4):
            for k in range(L):
                text = utf8_text(s, [(1, k, CP[L]), (2, k, CP[L])])
                add(("valid", L, k, (1, 2)), s, text, None, None)
                for r in (1, 2):
                    for j in range(1, L):
                        add(("cut", L, k, r, j), s, text, boundary(s, r) - k + j, None)
                    i = max(k, 1)            # the first continuation byte behind the boundary (k = 0: the first)
                    bad = CP[L][:i] + b"x" + CP[L][i + 1:]
                    add(("cont_ascii", L, k, r), s, utf8_text(s, [other(r), (r, k, bad)]), None, 0)
                    add(("cut_bad", L, k, r), s, utf8_text(s, [other(r), (r, k, bad)]), boundary(s, r) - k + i, 1)
        for r in (1, 2):
            for k in (0, 1):
                add(("lone", 1, k, r), s, utf8_text(s, [other(r), (r, k, b"\x80")]), None, 0)
            for name, seq in BAD_SEQ.items():
                for k in range(len(seq)):
                    add((name, len(seq), k, r), s, utf8_text(s, [other(r), (r, k, seq)]), None, 0)
    n = len(rows)
    res = [t[1] for t in tags]
    rig = dict(wbits=15, out_cap=TEXT_LEN + 4, msg_cap=TEXT_LEN, out_res=res, msg_res=res,
               wire_res=[(3 * i + i // 16) % 16 for i in range(n)])
    calls = [[row[t] for row in rows] for t in range(2)]
    return Case(n, SERVER, rig, want, calls=calls, tags=tags, fail_piece=fail)
