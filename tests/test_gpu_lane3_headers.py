"""Dynamic block headers of the lane inflate kernel (pmd_inflate_lane3.hip),
built bit by bit: the list of coded runs that the code-length pass leaves for
symbol placement (hdr_list.h), its fit rule at the boundary, the walk over
every symbol that headers which do not fit fall back to, and the reference's
header errors -- each beside other kinds of header in the same 64-lane wave.
Status, length and bytes of every message are compared with the oracle's
inflate, in the lane mode and in the block-parallel mode."""
import random

import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

CAP = 2048
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# a complete code-length code over all 19 symbols: 13 of 4 bits, 6 of 5 bits
CL_LENS = [4] * 13 + [5] * 6
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def canon_codes(lens):
    """RFC 1951 3.2.2 code values (garbage, but defined, for a bad length set)."""
    mx = max(lens) if lens else 0
    cnt = [0] * (mx + 2)
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * (mx + 2), 0
    for b in range(1, mx + 1):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        out.append(nxt[l] if l else 0)
        nxt[l] += 1 if l else 0
    return out


class Bits:
    def __init__(self):
        self.acc, self.n, self.buf = 0, 0, bytearray()

    def put(self, v, k):   # k bits of v, least significant first
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.buf.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, l):   # a Huffman code: most significant bit first
        self.put(int(format(c, "0%db" % l)[::-1], 2) if l else 0, l)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def nbits(self):
        return 8 * len(self.buf) + self.n


def rle_ops(seq):
    """Greedy code-length symbols for `seq`: 16 repeats a non-zero length 3-6
    times, 17 / 18 write 3-10 / 11-138 zeros.  Returns (symbol, extra) pairs."""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 3:
                k = min(run, 138)
                ops.append((18, k - 11) if k >= 11 else (17, k - 3))
                run -= k
            ops += [(0, 0)] * run
        else:
            ops.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                ops.append((16, k - 3))
                run -= k
            ops += [(v, 0)] * run
        i = j
    return ops


def plain_ops(seq):
    """Every non-zero length as itself (one list entry per coded symbol);
    zeros run-length coded."""
    ops, i = [], 0
    while i < len(seq):
        if seq[i]:
            ops.append((seq[i], 0))
            i += 1
        else:
            j = i
            while j < len(seq) and seq[j] == 0:
                j += 1
            ops += rle_ops([0] * (j - i))
            i = j
    return ops


def op_spans(ops):
    """(symbol, first, rep, length value) of every op, as the decoder sees it."""
    have, prev, out = 0, 0, []
    for s, x in ops:
        if s < 16:
            val, rep = s, 1
        elif s == 16:
            val, rep = prev, 3 + x
        else:
            val, rep = 0, (3 if s == 17 else 11) + x
        out.append((s, have, rep, val))
        have += rep
        prev = val
    return out


def fit_sum(ops, nlen):
    """2 entries + coded literal/length symbols (hdr_list.h list_fits)."""
    sp = op_spans(ops)
    entries = sum(1 for _, _, _, v in sp if v)
    coded = sum(max(0, min(a + r, nlen) - a) for _, a, r, v in sp if v and a < nlen)
    return 2 * entries + coded


class Msg:
    """One permessage-deflate payload and the bytes it should inflate to."""

    def __init__(self, rng):
        self.w, self.out, self.rng = Bits(), bytearray(), rng

    def tokens(self, lit, dist, nbytes):
        w, rng, out = self.w, self.rng, self.out
        lc, dc = canon_codes(lit), canon_codes(dist)
        lits = [s for s in range(min(256, len(lit))) if lit[s]]
        lsyms = [s for s in range(257, min(286, len(lit))) if lit[s]]
        dsyms = [s for s in range(min(30, len(dist))) if dist[s]]
        end = len(out) + nbytes
        while len(out) < end:
            ds = [s for s in dsyms if DBASE[s] <= len(out)]
            if lsyms and ds and (not lits or rng.random() < 0.3):
                ls, d = rng.choice(lsyms), rng.choice(ds)
                lx = rng.randrange(1 << LEXT[ls - 257])
                dx = rng.randrange(min(1 << DEXT[d], len(out) - DBASE[d] + 1))
                w.code(lc[ls], lit[ls])
                w.put(lx, LEXT[ls - 257])
                w.code(dc[d], dist[d])
                w.put(dx, DEXT[d])
                for _ in range(LBASE[ls - 257] + lx):
                    out.append(out[-(DBASE[d] + dx)])
            elif lits:
                s = rng.choice(lits)
                w.code(lc[s], lit[s])
                out.append(s)
            else:
                break
        w.code(lc[256], lit[256])

    def dynamic(self, lit, dist, ops=None, nbytes=200, hlit=None, hdist=None, cl_lens=None, data=True, final=0):
        """lit / dist: code lengths of the nlen literal/length and ndist
        distance symbols; ops: the code-length symbols that spell them."""
        w = self.w
        cl = cl_lens or CL_LENS
        ops = rle_ops(lit + dist) if ops is None else ops
        w.put(final | 2 << 1, 3)
        w.put(len(lit) - 257 if hlit is None else hlit, 5)
        w.put(len(dist) - 1 if hdist is None else hdist, 5)
        w.put(19 - 4, 4)
        for s in CL_ORDER:
            w.put(cl[s], 3)
        cc = canon_codes(cl)
        for s, x in ops:
            w.code(cc[s], cl[s])
            if s >= 16:
                w.put(x, {16: 2, 17: 3, 18: 7}[s])
        if data:
            self.tokens(lit, dist, nbytes)
        return self

    def fixed(self, nbytes):
        self.w.put(1 << 1, 3)
        self.tokens(FIXED_LIT, FIXED_DIST, nbytes)
        return self

    def stored(self, nbytes):
        w = self.w
        w.put(0, 3)
        w.align()
        w.put(nbytes, 16)
        w.put(nbytes ^ 0xffff, 16)
        for _ in range(nbytes):
            b = self.rng.randrange(256)
            w.put(b, 8)
            self.out.append(b)
        return self

    def payload(self):
        """Ends the message as a sync flush does, less its 00 00 ff ff."""
        self.w.put(0, 3)
        self.w.align()
        return bytes(self.w.buf)


def lens_of(n, coded):
    a = [0] * n
    for s, l in coded.items():
        a[s] = l
    return a


def complete(n):
    """n lengths of a complete code (n >= 2)."""
    k = n.bit_length() - 1
    return [k] * (2 ** (k + 1) - n) + [k + 1] * (2 * (n - 2 ** k))


TINY_LIT = lens_of(258, {97: 2, 98: 2, 256: 2, 257: 2})
TINY_DIST = [1]


def tiny(rng, nbytes=None):
    return Msg(rng).dynamic(TINY_LIT, TINY_DIST, nbytes=nbytes or rng.randrange(40, 500))


def boundary_lit(c):
    """c coded literal/length symbols: literals from 32 up, 256 and 257."""
    syms = list(range(32, 32 + c - 2)) + [256, 257]
    return lens_of(258, dict(zip(syms, complete(c))))


LONG_SYMS = [256, 101, 32, 258, 116, 97, 111, 105, 110, 115, 114, 104, 108, 100, 99, 117]


def longest(rng, lmax, dmax, nbytes):
    """Literal/length lengths 1 .. lmax, lmax and distance lengths 1 .. dmax, dmax."""
    ll, dl = list(range(1, lmax + 1)) + [lmax], list(range(1, dmax + 1)) + [dmax]
    return Msg(rng).dynamic(lens_of(259, dict(zip(LONG_SYMS, ll))), dl, nbytes=nbytes)


def uniform_batch(lmax, dmax, n=128):
    """A batch in which every code's longest length is the same: whole waves
    on one side of a code-length threshold of the decoder's search."""
    rng = random.Random(100 * lmax + dmax)
    cases = []
    for _ in range(n):
        m = longest(rng, lmax, dmax, rng.randrange(40, 400))
        cases.append(("long%d_%d" % (lmax, dmax), m.payload(), bytes(m.out)))
    return cases


def build_cases():
    """(name, payload, expected bytes or None for a bad header) of every message."""
    rng = random.Random(0x1157)
    cases = []

    def good(name, m):
        cases.append((name, m.payload(), bytes(m.out)))

    def bad(name, p):
        cases.append((name, p, None))

    # 1. tiny codes (they also sit between all the others)
    for i in range(24):
        good("tiny", tiny(rng))
    # 2. every symbol coded: the list cannot fit
    full_lit, full_dist = [8] * 226 + [9] * 60, [4] * 2 + [5] * 28
    for i in range(6):
        ops = plain_ops(full_lit + full_dist) if i % 2 else None
        assert fit_sum(ops or rle_ops(full_lit + full_dist), 286) > 288
        good("full", Msg(rng).dynamic(full_lit, full_dist, ops=ops, nbytes=rng.randrange(100, 400)))
    # 3. the fit boundary: 2 entries + coded literal/length symbols = 287, 288, 289
    for want, c, d in ((287, 95, [1]), (288, 94, [1, 2, 2]), (289, 95, [1, 1])):
        lit = boundary_lit(c)
        ops = plain_ops(lit + d)
        assert fit_sum(ops, len(lit)) == want
        for i in range(5):
            good("fit%d" % want, Msg(rng).dynamic(lit, d, ops=ops, nbytes=rng.randrange(100, 600)))
    # the same sums reached with repeats: 30 runs of 4 equal lengths (one
    # literal length and a 16 x 3 each) are 60 entries over 120 symbols
    lit = lens_of(258, {s: 7 for s in range(16, 136)} | {s: 6 for s in range(140, 142)} | {256: 6, 257: 6})
    base = rle_ops(lit[:16]) + [op for _ in range(30) for op in ((7, 0), (16, 0))] + rle_ops(lit[136:140]) \
        + plain_ops(lit[140:])
    for extra in ([1], [1, 1], [1, 2, 2]):   # 2 * (64 + len(extra)) + 124 + ... = 254 .. 258: all fit
        good("fitrep", Msg(rng).dynamic(lit, extra, ops=base + plain_ops(extra), nbytes=300))
    # 4. code lengths 1 .. 15
    l15 = list(range(1, 16)) + [15]
    lit = lens_of(259, dict(zip(LONG_SYMS, l15)))
    dist = l15[:]
    for i in range(6):
        good("len15", Msg(rng).dynamic(lit, dist, ops=plain_ops(lit + dist) if i % 2 else None,
                                       nbytes=rng.randrange(100, 800)))
    # 5. repeats: non-zero lengths 3 and 6 times, one across nlen; zero runs across nlen
    lit = lens_of(260, {s: 4 for s in range(48, 52)} | {s: 4 for s in range(65, 72)} | {256: 4, 258: 3, 259: 3})
    dist = [3] * 8   # 3 3 | 3 x 8: a literal 3 at 258, then 16 x 6 over [259, 265) and 16 x 3
    ops = rle_ops(lit + dist)
    sp = op_spans(ops)
    assert any(s == 16 and r == 3 for s, _, r, _ in sp) and any(s == 16 and r == 6 for s, _, r, _ in sp)
    assert any(s == 16 and a < 260 < a + r for s, a, r, _ in sp)
    for i in range(6):
        good("rep16", Msg(rng).dynamic(lit, dist, ops=ops, nbytes=rng.randrange(100, 800)))
    for nl, dist, zsym in ((260, [0, 0, 0, 1], 17), (270, [0, 0, 0, 0, 1], 18), (270, [0] * 12 + [1, 1], 18)):
        lit = lens_of(nl, {97: 2, 98: 2, 256: 2, 257: 2})   # zeros from 258 into the distances
        ops = rle_ops(lit + dist)
        assert any(s == zsym and a < nl < a + r for s, a, r, _ in op_spans(ops))
        for i in range(3):
            good("zerorun", Msg(rng).dynamic(lit, dist, ops=ops, nbytes=rng.randrange(100, 500)))
    # 6. the longest literal/length and distance code exactly 10 and 11 bits,
    # here among other headers; uniform_batch() has them alone in their waves
    for lmax, dmax in ((10, 10), (11, 10), (10, 11), (11, 11)):
        for i in range(3):
            good("long%d_%d" % (lmax, dmax), longest(rng, lmax, dmax, rng.randrange(100, 600)))
    # 7. dynamic, fixed, stored and a second dynamic block: the lengths differ,
    # so lanes reach their second header while others are in data
    for i in range(24):
        m = tiny(rng, rng.randrange(20, 300)) if i % 3 else Msg(rng).dynamic(full_lit, full_dist, nbytes=rng.randrange(20, 200))
        m.fixed(rng.randrange(1, 120)).stored(rng.randrange(0, 60))
        if i % 2:
            m.dynamic(boundary_lit(95), [1, 1] if i % 4 == 1 else [1], nbytes=rng.randrange(20, 200))
        else:
            m.dynamic(TINY_LIT, TINY_DIST, nbytes=rng.randrange(20, 300))
        good("blocks", m)

    # 8. bad headers
    def hdr(lit, dist, **kw):
        m = Msg(rng).dynamic(lit, dist, data=False, **kw)
        for _ in range(12):
            m.w.put(rng.randrange(256), 8)
        return m.payload()

    for rep in range(2):
        bad("over_lit", hdr(lens_of(258, {97: 1, 98: 1, 256: 1}), [1]))
        bad("incomplete_lit", hdr(lens_of(258, {97: 2, 98: 2, 256: 2}), [1]))
        bad("over_dist", hdr(TINY_LIT, [1, 1, 1]))
        bad("incomplete_dist", hdr(TINY_LIT, [2, 2]))
        bad("over_cl", hdr(TINY_LIT, TINY_DIST, cl_lens=[4] * 14 + [5] * 5))
        bad("incomplete_cl", hdr(TINY_LIT, TINY_DIST, cl_lens=[4] * 12 + [5] * 7))
        bad("no_eob", hdr(lens_of(258, {97: 2, 98: 2, 99: 2, 257: 2}), [1]))
        bad("rep_no_prev", hdr(TINY_LIT, TINY_DIST, ops=[(16, 1)] + rle_ops((TINY_LIT + TINY_DIST)[4:])))
        ops = rle_ops(TINY_LIT + TINY_DIST)
        bad("rep_past_end", hdr(TINY_LIT, TINY_DIST, ops=ops[:-1] + [(16, 0)]))
        bad("zeros_past_end", hdr(TINY_LIT, TINY_DIST, ops=ops[:-1] + [(18, 20)]))
        for hl in (30, 31):
            bad("nlen%d" % (257 + hl), hdr(TINY_LIT, TINY_DIST, hlit=hl))
        for hd in (30, 31):
            bad("ndist%d" % (1 + hd), hdr(TINY_LIT, TINY_DIST, hdist=hd))
    # a header cut short in every field (block type, counts, code-length code
    # lengths, code lengths, data), byte by byte
    for lit, dist in ((TINY_LIT, TINY_DIST), (boundary_lit(95), [1])):
        m = Msg(rng).dynamic(lit, dist, ops=plain_ops(lit + dist), nbytes=6)
        whole = m.payload()
        for k in range(0, len(whole), 1 if len(whole) < 40 else 4):
            bad("cut", whole[:k])
    return cases


@pytest.fixture(scope="module")
def batches():
    """The messages in a fixed shuffled order, in batches of at most 256 (full,
    mixed 64-lane waves), with the oracle's status and bytes for each."""
    cases = build_cases()
    rng = random.Random(2)
    while len(cases) < 256:
        m = tiny(rng)
        cases.append(("tiny", m.payload(), bytes(m.out)))
    assert len(cases) == 256
    rng.shuffle(cases)
    cases += uniform_batch(10, 10) + uniform_batch(11, 11) + uniform_batch(10, 11) + uniform_batch(11, 10)
    expect = []
    for name, p, want in cases:
        assert len(p) <= 1024, name
        est, eout = O.pmd_inflate(p, cap=CAP)
        if want is not None:   # the writer wrote what it meant to
            assert est == 0 and eout == want, (name, O.ERRORS[est])
        else:
            assert name == "cut" or est != 0, name
        expect.append((est, eout))
    names = {n for n, _, _ in cases}
    assert {"tiny", "full", "fit287", "fit288", "fit289", "len15", "rep16", "zerorun", "blocks", "no_eob"} <= names
    cuts = (0, 256, 384, 512, 768)   # the mixed batch, 10 / 10, 11 / 11, and both mixed halves together
    return [(cases[a:b], expect[a:b]) for a, b in zip(cuts, cuts[1:])]


@pytest.mark.parametrize("mode", ["lane", "bp"])
def test_built_headers_match_the_oracle(batches, mode):
    import torch
    from beast_amd import pmd

    L = pmd.lib()
    assert L.bpmd_set_inflate_kernel({"lane": 1, "bp": 3}[mode]) == 0
    try:
        for cases, expect in batches:
            assert 128 <= len(cases) <= 256
            res = pmd.inflate_batch(pmd.Batch.from_host([p for _, p, _ in cases]), CAP)
            torch.cuda.synchronize()
            st, outs = res.status.cpu().tolist(), res.out.to_host()
            for i, (name, p, _) in enumerate(cases):
                est, eout = expect[i]
                assert st[i] == est, (mode, i, name, O.ERRORS[st[i]], O.ERRORS[est])
                assert outs[i] == eout, (mode, i, name, len(outs[i]), len(eout))
    finally:
        L.bpmd_set_inflate_kernel(0)
