"""Permessage-deflate payloads written token by token, for the step of the
inflate kernels that turns decoded symbols into bytes (tests/test_token_cases.py
pins them on the CPU, tests/test_gpu_inflate_tokens.py decodes them on the GPU).

A message is a list of tokens:

    b                          a literal byte
    (len, dist)                a match
    ("m", lsym, lx, dsym, dx)  a match by its symbols and extra bits
    CUT                        end the block here and start another
    ("L", sym)                 a lone literal/length symbol (286, 287)
    ("D", len, dsym)           a length, then a distance symbol (30, 31)
    ("X", len, bits, n)        a length, then n raw bits where a distance code goes

render() writes it in one of three ways and returns the payload (ended as a
sync flush does, less its 00 00 ff ff) with the bytes it should inflate to,
from a byte-at-a-time copy of its own:

    fixed   one fixed-Huffman block (cuts are ignored)
    dyn     dynamic blocks over a code that holds every symbol (complete(286)
            and complete(30)), cut every K tokens: the block-parallel decoder
            starts segments inside the message and matches reach back over them
    long    one dynamic block whose literal/length and distance codes both
            reach 15 bits: length symbols 281-284 (5 extra bits) and distance
            symbols 28 and 29 (13 extra bits) carry 15-bit codes, so a match
            is 15 + 5 + 15 + 13 = 48 bits, the most a token can take
    hole    the long literal/length code with a distance code of one 1-bit
            symbol: the one incomplete code the reference accepts, whose other
            code word no symbol owns

The families (A-H) are chosen from the constants of the kernels; DESIGN.md
lists which edge each one is for."""
import random
from array import array

from tests.test_gpu_lane3_headers import (CL_LENS, CL_ORDER, DBASE, DEXT, FIXED_DIST, FIXED_LIT, LBASE, LEXT, Bits,
                                          canon_codes, complete, lens_of, rle_ops)

CUT = "cut"
K_DEFAULT = 24
EB = b"\x00\x00\xff\xff"

# the kernels' constants the values below are chosen from
KLIT = 4          # pmd_inflate_lane3.hip: literals taken ahead of a token
RING = 4096       # pmd_inflate.hip: LDS history ring
R_MAX = 3840      # pmd_inflate.hip: output bytes per round
BP_FLOOR = 64     # pmd_inflate_bp.hip: shortest payload decoded block-parallel
LANE_MULTI_BITS = 48 + 15 * (KLIT - 1)   # pmd_inflate_lane3.hip: input left for an iteration of several symbols

LONG_LIT = lens_of(286, {97: 1, 98: 2, 285: 3, 256: 4, **{99 + i: 5 + i for i in range(9)},
                         281: 15, 282: 15, 283: 15, 284: 15})
LONG_DIST = lens_of(30, {**{i: i + 1 for i in range(14)}, 28: 15, 29: 15})
LONG_LETTERS = list(range(98, 108))
HOLE_DIST = [1]


def _rev(c, l):
    return int(format(c, "0%db" % l)[::-1], 2) if l else 0


class WordBits(Bits):
    """Bits that moves eight bytes at a time to its buffer: the same bits in
    the same order, for payloads of tens of thousands of tokens."""

    def put(self, v, k):   # k <= 16
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        if self.n >= 64:
            self.buf += (self.acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            self.acc >>= 64
            self.n -= 64

    def align(self):
        self.put(0, -self.n % 8)
        self.buf += self.acc.to_bytes(self.n // 8, "little")
        self.acc = self.n = 0


class Code:
    """A Huffman code as (bit-reversed code, length) per symbol."""

    def __init__(self, lens):
        self.lens = list(lens)
        self.rev = [_rev(c, l) for c, l in zip(canon_codes(self.lens), self.lens)]

    def put(self, w, s):
        assert s < len(self.lens) and self.lens[s], ("symbol has no code", s)
        w.put(self.rev[s], self.lens[s])


def kraft(lens):
    return sum(2.0 ** -l for l in lens if l)


assert kraft(LONG_LIT) == 1.0 and kraft(LONG_DIST) == 1.0 and max(LONG_LIT) == max(LONG_DIST) == 15
_CODES = {
    "fixed": (Code(FIXED_LIT), Code(FIXED_DIST + [5, 5])),   # distance symbols 30 and 31 have code words too
    "dyn": (Code(complete(286)), Code(complete(30))),
    "long": (Code(LONG_LIT), Code(LONG_DIST)),
    "hole": (Code(LONG_LIT), Code(HOLE_DIST)),
}
_HDR_LENS = {"dyn": (complete(286), complete(30)), "long": (LONG_LIT, LONG_DIST), "hole": (LONG_LIT, HOLE_DIST)}
_CL = Code(CL_LENS)

_LSYM = [None] * 259
for _l in range(3, 258):
    _i = max(i for i in range(28) if LBASE[i] <= _l)
    _LSYM[_l] = (257 + _i, _l - LBASE[_i])
_LSYM[258] = (285, 0)


def dist_sym(d):
    i = max(i for i in range(30) if DBASE[i] <= d)
    return i, d - DBASE[i]


def _header(w, mode):
    if mode == "fixed":
        w.put(1 << 1, 3)
        return
    lit, dist = _HDR_LENS[mode]
    w.put(2 << 1, 3)
    w.put(len(lit) - 257, 5)
    w.put(len(dist) - 1, 5)
    w.put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(CL_LENS[s], 3)
    for s, x in rle_ops(lit + dist):
        _CL.put(w, s)
        if s >= 16:
            w.put(x, {16: 2, 17: 3, 18: 7}[s])


class Rendered:
    """payload; out: the bytes up to the first token that cannot be decoded
    (all of them when good); bit[i] / pos[i]: where token i starts in the
    payload (bits) and in the output, with one more entry for the end;
    starts: the tokens that are the first of a block."""
    __slots__ = ("payload", "out", "good", "bit", "pos", "starts")


def render(tokens, mode="fixed", K=K_DEFAULT):
    w, out, good = WordBits(), bytearray(), True
    lc, dc = _CODES[mode]
    bit, pos, starts = array("I"), array("I"), set()
    _header(w, mode)
    in_block = 0

    def cut():
        lc.put(w, 256)
        _header(w, mode)

    for t in tokens:
        if t is CUT:
            bit.append(w.nbits())
            pos.append(len(out))
            if mode != "fixed" and in_block:
                cut()
                in_block = 0
            continue
        if mode == "dyn" and in_block == K:
            cut()
            in_block = 0
        if in_block == 0:
            starts.add(len(bit))
        in_block += 1
        bit.append(w.nbits())
        pos.append(len(out))
        if isinstance(t, int):
            lc.put(w, t)
            if good:
                out.append(t)
            continue
        if t[0] == "L":
            lc.put(w, t[1])
            good = False
            continue
        if t[0] == "m":
            _, ls, lx, ds, dx = t
        elif t[0] in ("D", "X"):
            ls, lx = _LSYM[t[1]]
        else:
            (ls, lx), (ds, dx) = _LSYM[t[0]], dist_sym(t[1])
        lc.put(w, ls)
        w.put(lx, LEXT[ls - 257])
        if t[0] == "D":
            dc.put(w, t[2])
            good = False
            continue
        if t[0] == "X":
            w.put(t[2], t[3])
            good = False
            continue
        dc.put(w, ds)
        w.put(dx, DEXT[ds])
        n, d = LBASE[ls - 257] + lx, DBASE[ds] + dx
        if d > len(out):
            good = False
        if good:
            for _ in range(n):
                out.append(out[-d])
    bit.append(w.nbits())
    pos.append(len(out))
    lc.put(w, 256)
    w.put(0, 3)
    w.align()
    r = Rendered()
    r.payload, r.out, r.good, r.bit, r.pos, r.starts = bytes(w.buf), bytes(out), good, bit, pos, starts
    return r


class Case:
    """One message in one renderer.  runs: the (cap, raw, window_bits) it is
    decoded at in a batch.  expect: the status the oracle must give at a roomy
    capacity, or None where only the oracle says (cut payloads).  key: what
    the family varies, for the tests that take a part of a family."""

    def __init__(self, family, name, tokens, mode, runs=None, expect="ok", key=(), K=K_DEFAULT, cut=None):
        r = render(tokens, mode, K)
        self.family, self.name, self.tokens, self.mode, self.key = family, name, tokens, mode, key
        self.payload = r.payload if cut is None else r.payload[:cut]
        self.whole = r.payload
        self.out, self.good, self.bit, self.pos, self.starts = r.out, r.good, r.bit, r.pos, r.starts
        self.expect = expect if cut is None else None
        assert r.good == (expect == "ok"), (family, name, mode)
        self.runs = runs or [(max(1, len(r.out)) + (0 if r.good else 300), False, 15)]

    def token_at(self, byte):
        """Index of the token that writes output byte `byte`."""
        lo, hi = 0, len(self.pos) - 1
        while lo < hi:   # the last token starting at or before it
            mid = (lo + hi + 1) // 2
            if self.pos[mid] <= byte:
                lo = mid
            else:
                hi = mid - 1
        return lo

    def describe(self, byte):
        """family, token index, token and output position for a failure at `byte`."""
        i = min(self.token_at(byte), len(self.tokens) - 1) if self.tokens else 0
        t = self.tokens[i] if self.tokens else None
        return "family %s %s [%s] token %d %r written at output %d, payload bit %d" % (
            self.family, self.name, self.mode, i, t, self.pos[i] if self.tokens else 0, self.bit[i] if self.tokens else 0)

    def token_bits(self, i):
        return self.bit[i + 1] - self.bit[i]

    def lane_place(self, cap, raw):
        """Where the lane decoder's iterations put every token of the whole
        payload (pmd_inflate_lane3.hip data_step): {token: (symbols taken
        before it in its iteration, input bits left at the iteration's start)}.
        An iteration takes up to KLIT leading literals and then, if there were
        fewer than KLIT, one main symbol -- so a token is the 1st to KLIT-th
        symbol of its iteration, never a later one -- but only while
        48 + 15 * (KLIT - 1) bits of input are left (pmd framing counts its 32
        tail bits) and KLIT bytes of output; otherwise it takes one symbol.
        An iteration does not go on into the next block."""
        total = 8 * len(self.whole) + (0 if raw else 32)
        toks, place, i = self.tokens, {}, 0
        assert CUT not in toks
        while i < len(toks):
            left = total - self.bit[i]
            k = 0
            if left >= LANE_MULTI_BITS and self.pos[i] + KLIT <= cap:
                while k < KLIT and i + k < len(toks) and isinstance(toks[i + k], int) and not (k and i + k in self.starts):
                    place[i + k] = (k, left)
                    k += 1
                if k < KLIT and i + k < len(toks) and not (k and i + k in self.starts):
                    place[i + k] = (k, left)   # the main symbol; otherwise it is the end of the block
                    k += 1
            else:
                place[i] = (0, left)
                k = 1
            i += max(k, 1)
        return place


def _lits(rng, n):
    return [rng.randrange(256) for _ in range(n)]


# ---------------------------------------------------------------- family A
A_DISTS = (list(range(1, 73)) + [127, 128, 129] + list(range(255, 260)) + [511, 512, 513]
           + [3839, 3840, 3841, 4095, 4096, 4097, 8191, 8192, 8193] + [16384, 24577, 32767, 32768])
A_LENS = [3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 258]
A_LEADS = range(6)


def family_a(modes=("fixed", "dyn")):
    """distance x length x lead-in: one distance and one lead-in per message,
    every length in it, after dist .. dist + 2 random literals."""
    cases = []
    for d in A_DISTS:
        for lead in A_LEADS:
            rng = random.Random(1000 * d + lead)
            toks = _lits(rng, d + rng.randrange(3))
            for n in A_LENS:
                toks += _lits(rng, lead)
                toks.append((n, d))
            for mode in modes:
                cases.append(Case("A", "dist %d lead %d" % (d, lead), toks, mode, key=(d, lead)))
    return cases


# ---------------------------------------------------------------- family B
def family_b():
    """4300 random literals, then (70, d) for every d of a range around the
    wave kernel's 4 KiB ring and around its round limit: length 70 moves the
    64-byte chunk phase by 6 per token."""
    cases = []
    for name, ds in (("ring", range(RING - 136, RING + 135)), ("round", range(R_MAX - 64, R_MAX + 65))):
        rng = random.Random(len(ds))
        toks = _lits(rng, 4300) + [(70, d) for d in ds]
        for mode in ("fixed", "dyn"):
            cases.append(Case("B", name, toks, mode, key=(name,)))
    return cases


# ---------------------------------------------------------------- family C
def chain_depth(tokens):
    """The longest chain of matches each of which reads bytes that the one
    before it wrote (a match reading its own bytes does not count twice)."""
    owner, depth, best = [], [], 0   # owner[byte] = token index; depth[token]
    for i, t in enumerate(tokens):
        if isinstance(t, int):
            owner.append(i)
            depth.append(0)
            continue
        n, d = t
        at = len(owner)
        srcs = {owner[p] for p in range(at - d, min(at, at - d + n))}
        depth.append(1 + max(depth[s] for s in srcs))
        owner += [i] * n
        best = max(best, depth[-1])
    return best


def _chain(rng, total=64):
    """One literal, then matches that fill `total` bytes, each one reading
    from inside the match before it."""
    toks, at, last = [rng.randrange(256)], 1, 1
    while at < total:
        n = min(total - at, rng.choice([3, 3, 4, 5, 8, 16, 31]))
        if n < 3:
            toks += [rng.randrange(256)] * n
            at += n
            continue
        d = rng.randrange(1, min(last, 63) + 1)
        toks.append((n, d))
        at, last = at + n, n
    return toks


def family_c():
    """64 bytes built from one literal by matches whose sources are earlier
    matches of the same 64-byte chunk, at chunk offsets 0, 1, 31, 32, 63; the
    same with every match preceded by 1-4 literals."""
    base = [[97, (3, 1), (4, 2), (8, 4), (16, 8), (32, 16)], [97, (3, 1), (4, 2), (8, 4), (16, 8), (31, 16), 98]]
    rng = random.Random(0xC)
    while len(base) < 14:
        c = _chain(rng)
        if chain_depth(c) >= 6:
            base.append(c)
    # distances up to 63: a short pattern copied from ever farther back in the chunk
    base.append([97, 98, 99, (3, 3), (4, 5), (5, 9), (6, 14), (7, 20), (8, 27), (9, 35), (10, 44), (9, 54)])
    base.append([97, (3, 1), (5, 4), (7, 9), (9, 16), (11, 25), (13, 36), (15, 49)])
    cases = []
    for ci, chain in enumerate(base):
        for off in (0, 1, 31, 32, 63):
            for nl in range(5):
                rng = random.Random(100 * ci + 10 * off + nl)
                toks = _lits(rng, off)
                for t in chain:
                    if not isinstance(t, int):
                        toks += _lits(rng, nl)
                    toks.append(t)
                for mode in ("fixed", "dyn"):
                    cases.append(Case("C", "chain %d offset %d literals %d" % (ci, off, nl), toks, mode,
                                      key=(ci, off, nl)))
    return cases


# ---------------------------------------------------------------- family D
def family_d():
    """A match whose source ends at, just before and just after the byte its
    destination begins at, followed directly by a match that reads the tail
    of the first."""
    cases = []
    for d in range(1, 41):
        lens = {d - 1, d, d + 1, 2 * d, 2 * d + 1} | ({258} if d >= 8 else set())
        for n in sorted(x for x in lens if 3 <= x <= 258):
            rng = random.Random(1000 * d + n)
            d2 = min(n, 7 + d % 11)
            toks = _lits(rng, d + 2) + [(n, d), (n, d2)] + _lits(rng, 3)
            for mode in ("fixed", "dyn"):
                cases.append(Case("D", "dist %d len %d then dist %d" % (d, n, d2), toks, mode, key=(d, n)))
    return cases


# ---------------------------------------------------------------- family E
def family_e():
    """Two messages decoded once per capacity from 1 to two past their length,
    in both framings."""
    cases = []
    for name, tail in (("tail 4", 4), ("tail 12", 12)):
        rng = random.Random(tail)
        toks = _lits(rng, 20) + [(100, 3)] + _lits(rng, 5) + [(258, 17)] + _lits(rng, 6) + [(9, 1)] + _lits(rng, tail)
        n = 20 + 100 + 5 + 258 + 6 + 9 + tail
        for mode in ("fixed", "dyn"):
            runs = [(cap, raw, 15) for raw in (False, True) for cap in range(1, n + 3)]
            c = Case("E", name, toks, mode, runs=runs, key=(tail,))
            assert len(c.out) == n
            cases.append(c)
    return cases


# ---------------------------------------------------------------- family F
F_POS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 300]
F_TAIL = 16   # literals after the token: 128 bits or more, so the token's iteration takes several symbols


def family_f():
    """A distance equal to the bytes produced (accepted) and one more
    (invalid_distance), at a roomy capacity and at capacities equal to the
    position and one and two above it, where the reference's order between
    "full" and "too far" decides; distances beyond 2^windowBits.  Every
    message comes with the token at the input's end, where the lane decoder
    takes one symbol per iteration, and with F_TAIL literals after it, where
    the token is the 1st to 4th symbol of an iteration that took the
    literals before it first (Case.lane_place)."""
    cases = []

    def pair(name, pre, n, mode, runs_of, key):
        pos = sum(1 if isinstance(t, int) else t[0] for t in pre)
        for tail in (0, F_TAIL):
            after = _lits(random.Random(pos + n), tail)
            tn = "%s, %d literals after," % (name, tail)
            if pos:
                cases.append(Case("F", "%s dist = pos = %d len %d" % (tn, pos, n), pre + [(n, pos)] + after, mode,
                                  runs=runs_of(pos, n + tail), key=key + (tail, "at")))
            cases.append(Case("F", "%s dist = pos + 1 = %d len %d" % (tn, pos + 1, n), pre + [(n, pos + 1)] + after,
                              mode, runs=runs_of(pos, n + tail), expect="invalid_distance",
                              key=key + (tail, "past")))

    def edge_runs(pos, n):
        return [(cap, raw, 15) for raw in (False, True) for cap in (pos + n + 5, pos, pos + 1, pos + 2) if cap >= 1]

    for mode in ("fixed", "dyn"):
        for n in (3, 258):
            # pos literals: with input left, the token is symbol 1 + pos % KLIT of its iteration
            for pos in F_POS:
                pair("literals", _lits(random.Random(pos), pos), n, mode, edge_runs, ("lit", pos, n))
            # a match, then r literals: symbol 1 + r % KLIT of an iteration after the match's
            for r in range(KLIT + 1):
                rng = random.Random(50 + r)
                pair("after a match, %d literals," % r, _lits(rng, 8) + [(3, 1)] + _lits(rng, r), n, mode, edge_runs,
                     ("match", r, n))
        # beyond the window: a single call accepts every distance up to the bytes produced
        rng = random.Random(700)
        pre = _lits(rng, 700)
        for d in (500, 512, 513, 600, 700, 701):
            cases.append(Case("F", "window: 700 literals, (258, %d)" % d, pre + [(258, d)], mode,
                              runs=[(1000, False, 9), (1000, False, 15)],
                              expect="ok" if d <= 700 else "invalid_distance", key=("window", d)))
    rng = random.Random(40000)
    pre = _lits(rng, 40000)
    for mode in ("fixed", "dyn"):
        for d in (32767, 32768):
            cases.append(Case("F", "window: 40000 literals, (258, %d)" % d, pre + [(258, d)], mode,
                              runs=[(40258, False, 9)], key=("window", d)))
    return cases


# ---------------------------------------------------------------- family G
G_GROUP = [(281, 0, 28, 0), (284, 31, 29, 8191), (282, 31, 28, 8191), (283, 0, 29, 0),
           (284, 0, 28, 8191), (281, 31, 29, 0), (283, 31, 29, 8191), (282, 0, 28, 0)]
G_CUTS = range(1, 13)


def family_g():
    """Tokens of 48 bits (15-bit length code, 5 extra bits, 15-bit distance
    code, 13 extra bits, all ones and all zeros) at every bit phase, at the
    end of the input; the payloads cut at each of their last 12 bytes."""
    cases = []
    rng = random.Random(0x6)
    prefix, last = [], 0
    for _ in range(128):   # 128 x 259 bytes: past 32768, in runs of letters that no period repeats
        last = rng.choice([c for c in LONG_LETTERS if c != last])
        prefix += [last, (258, 1)]
    for phase in range(8):
        toks = prefix + [97] * phase + [("m",) + g for g in G_GROUP]
        whole = Case("G", "48-bit tokens after %d one-bit literals" % phase, toks, "long", key=("long", phase))
        cases.append(whole)
        for k in G_CUTS:
            cases.append(Case("G", "48-bit tokens after %d one-bit literals, less %d bytes" % (phase, k), toks, "long",
                              key=("long", phase, k), cut=len(whole.payload) - k,
                              runs=[(len(whole.out) + 300, False, 15), (len(whole.out) + 300, True, 15)]))
    rng = random.Random(0x66)
    for name, toks in (("16 literals at the end", _lits(rng, 40) + [(30, 7)] + _lits(rng, 16)),
                       ("(258, 32768) at the end", _lits(rng, 32768) + [(258, 32768)])):
        for mode in ("fixed", "dyn"):
            whole = Case("G", name, toks, mode, key=(mode, name))
            cases.append(whole)
            for k in G_CUTS:
                cases.append(Case("G", "%s, less %d bytes" % (name, k), toks, mode, key=(mode, name, k),
                                  cut=len(whole.payload) - k,
                                  runs=[(len(whole.out) + 300, False, 15), (len(whole.out) + 300, True, 15)]))
    return cases


# ---------------------------------------------------------------- family H
def family_h():
    """Symbols that are coded but stand for nothing, after 0 to 4 literals (24
    literals before the input's end they are the 1st to 4th symbol of a lane
    decoder iteration, Case.lane_place; at the input's end the 1st).  The fixed
    code has four of them; a dynamic block can have one only in a distance
    code of a single 1-bit symbol (every other incomplete code is refused at
    the header), so the dyn renderer, whose codes are complete, has none."""
    cases = []
    bads = [("fixed", "length symbol 286", ("L", 286), "invalid_literal_length"),
            ("fixed", "length symbol 287", ("L", 287), "invalid_literal_length"),
            ("fixed", "distance symbol 30", ("D", 9, 30), "invalid_distance_code"),
            ("fixed", "distance symbol 31", ("D", 258, 31), "invalid_distance_code"),
            ("hole", "unowned distance code word", ("X", 258, 1, 1), "invalid_distance_code")]
    for mode, what, bad, expect in bads:
        letters = LONG_LETTERS if mode == "hole" else list(range(256))
        for lead in (False, True):
            for r in range(KLIT + 1):
                for tail in (0, 24):
                    rng = random.Random(10 * r + tail)
                    pick = lambda n: [rng.choice(letters) for _ in range(n)]   # noqa: E731
                    toks = (pick(6) + [(258, 1) if mode == "hole" else (4, 2)] if lead else []) + pick(r) + [bad] + pick(tail)
                    cases.append(Case("H", "%s after %s%d literals, %d after" % (what, "a match and " if lead else "", r, tail),
                                      toks, mode, expect=expect, key=(what, lead, r, tail),
                                      runs=[(600, False, 15), (600, True, 15)]))
    return cases


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f,
            "G": family_g, "H": family_h}
_BUILT = {}


def family(letter):
    """The cases of one family, built once."""
    if letter not in _BUILT:
        _BUILT[letter] = FAMILIES[letter]()
    return _BUILT[letter]


# ------------------------------------------------------------------ history
def history_connections():
    """(name, window_bits, [first payload, second payload]) of connections
    whose second message reaches into the first: k literals, then a match of
    distance k + h (the whole history) and, in a sibling, of k + h + 1."""
    conns = []

    def add(wbits, h, reach):
        first = render(_lits(random.Random(h), h)).payload
        for k in range(10):
            for extra in (0, 1):
                toks = _lits(random.Random(100 * h + k), k) + [(5, k + reach + extra)]
                conns.append(("h %d k %d dist %d" % (h, k, k + reach + extra), wbits,
                              [first, render(toks).payload]))

    for h in (1, 7, 8, 9, 600):
        add(15, h, h)
    add(9, 600, 512)
    return conns
