"""GPU: bpmd_read_batch with masking keys in every decoder plan, against the
oracle on the unmasked payloads -- exact status, length and bytes, input
unchanged, nothing written outside a slot, no message left unclaimed
(tests/read_keyed_cases.py run()).

The key is applied inside the decoders' input loads, in four places with
their own edge handling: the lane kernel's 16-byte blocks
(pmd_inflate_lane3.hip begin / open_view, lane_io.h finish_in / finish_block),
the wave kernel's window (pmd_inflate.hip load_window: aligned fast path,
in_word, in_byte, refilled every BPMD_IN_CAP bytes), the wave kernel behind a
lane / wave split (inflate_keyed_split, grid-strided or from a work queue)
and over the long prefix of the order (inflate_wave_ordered).  Before each
call the compiled inflate_plan.h is asked which of them the batch takes, so
a later change of thresholds fails here instead of leaving a branch unrun.
"""
import json
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import oracle as O
from tests import read_keyed_cases as K
from tests.test_inflate_plan import (AUTO, G_WAVE_ORDERED, lanes_plain, lanes_queue, lanes_wave_split, load_plan)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_CAP = K.in_cap()


def _pmd():
    import torch  # noqa: F401
    from beast_amd import pmd
    return pmd


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return load_plan(tmp_path_factory.mktemp("read_keyed_plan"))


@pytest.fixture(scope="module")
def wgs():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(params=["lane", "wave", "auto"])
def inflate_kernel(request):
    pmd = _pmd()
    assert pmd.lib().bpmd_set_inflate_kernel({"lane": 1, "wave": 2, "auto": 0}[request.param]) == 0
    yield request.param
    pmd.lib().bpmd_set_inflate_kernel(0)


_GRID = {}


def _edge_grid(raw):
    if raw not in _GRID:
        c = K.edge_grid(IN_CAP, raw=raw)
        _GRID[raw] = (c, K.expect(c))
    return _GRID[raw]


@pytest.mark.parametrize("raw", [False, True])
def test_edge_grid(inflate_kernel, raw):
    """Every payload start alignment 0..15 times every compressed length in
    0..80, IN_CAP - 8 .. IN_CAP + 40 and 2 IN_CAP - 4 .. 2 IN_CAP + 20, as
    stored blocks and as a cut dynamic block, and about 200 whole payloads;
    keys 0, all ones, one byte each and random; capacities exact, one short
    and 1.  raw: no 00 00 FF FF tail is spliced behind the unmasked bytes."""
    case, want = _edge_grid(raw)
    r = K.run(case, want)
    assert not r.bad, r.bad[:8]


_SPLIT = {}


def _split_batch(split):
    if split not in _SPLIT:
        c = K.split_batch(2048, split, random.Random(31))
        _SPLIT[split] = (c, K.expect(c))
    return _SPLIT[split]


@pytest.mark.parametrize("how", ["grid", "queue"])
@pytest.mark.parametrize("split", [4096, 1024])
def test_split_plan(plan, wgs, monkeypatch, split, how):
    """2048 keyed messages in automatic mode: payloads up to the split on
    lanes, the rest one wave each (inflate_keyed_split with min_in), the
    waves grid-strided or, with a grid of 64, from their work queue.  Stored
    payloads of split - 1, split and split + 1 bytes sit on both sides."""
    pmd = _pmd()
    monkeypatch.setenv("BPMD_INFLATE_SPLIT", str(split))
    assert plan(AUTO, 2048, key=True, wgs=wgs, split=split) == lanes_wave_split(split)
    case, want = _split_batch(split)
    assert pmd.lib().bpmd_set_inflate_kernel(0) == 0
    try:
        if how == "queue":
            pmd.lib().bpmd_diag_set_grid(64)
        r = K.run(case, want)
    finally:
        pmd.lib().bpmd_diag_set_grid(0)
    assert not r.bad, r.bad[:8]


def test_plain_lanes_32k(plan, wgs, monkeypatch):
    """From 32 Ki messages the lanes take every payload, the 64 KiB ones too."""
    pmd = _pmd()
    monkeypatch.delenv("BPMD_INFLATE_SPLIT", raising=False)
    assert plan(AUTO, 32768, key=True, wgs=wgs) == lanes_plain()
    case = K.lanes_batch(32768, random.Random(51))
    assert pmd.lib().bpmd_set_inflate_kernel(0) == 0
    r = K.run(case)
    assert not r.bad, r.bad[:8]


def test_unkeyed_equals_keyed_with_zero_key(plan, wgs, monkeypatch):
    """No key: payloads over the split decode block-parallel.  Keys all zero:
    the same bytes through lanes and waves.  Both equal the oracle, hence
    each other."""
    pmd = _pmd()
    monkeypatch.delenv("BPMD_INFLATE_SPLIT", raising=False)
    assert plan(AUTO, 2048, key=True, wgs=wgs) == lanes_wave_split(4096)
    assert plan(AUTO, 2048, key=False, wgs=wgs) != lanes_wave_split(4096)
    case, want = _split_batch(4096)
    assert pmd.lib().bpmd_set_inflate_kernel(0) == 0
    a = K.run(K.unkeyed(case), want)
    b = K.run(K.replace(case, keys=[0] * len(case.payloads)), want)
    assert not a.bad, a.bad[:8]
    assert not b.bad, b.bad[:8]
    assert (a.status == b.status).all() and (a.out_len == b.out_len).all() and a.outs == b.outs


# One child on the MI355X: 2.2 to 2.6 s wall (6.53 and 7.71 s for the three in
# two runs of the suite, of which 1.6-1.8 s each from building the batch to the
# checked result; the rest is the interpreter, torch and the library load).
# Five times that on a shared machine with a cold library load, and never less
# than 60 s.
CHILD_SECONDS_MEASURED = 2.6
CHILD_TIMEOUT = max(60.0, 5 * CHILD_SECONDS_MEASURED)

QUEUE_ENV = {"BPMD_QUEUE_WGS": "8", "BPMD_INFLATE_SPLIT": "0"}


def test_queue_plans_in_child(plan):
    """The knobs read once per process, each in a fresh child
    (python -m tests.read_keyed_cases): 4096 messages over 8 workgroups of
    lanes run from the work queue, (1) keyed, the long prefix of the order on
    waves (inflate_wave_ordered with a key, the lanes skip it), (2) the same
    plan without a key (BPMD_INFLATE_BP=0), (3) keyed with BPMD_INFLATE_ORDER=0,
    the queue in batch order and nothing split off."""
    wave_ordered = lanes_queue(long=G_WAVE_ORDERED, args=(512, 4096, 200))
    children = [
        ("keyed", {}, dict(key=True), wave_ordered),
        ("unkeyed", {"BPMD_INFLATE_BP": "0"}, dict(key=False, bp=False), wave_ordered),
        ("keyed", {"BPMD_INFLATE_ORDER": "0"}, dict(key=True, ordered=False), lanes_queue(order=False)),
    ]
    for which, extra, knobs, want in children:
        assert plan(AUTO, 4096, wgs=8, split=0, **knobs) == want
    for which, extra, knobs, want in children:
        env = {k: v for k, v in os.environ.items()
               if not k.startswith(("BPMD_INFLATE", "BPMD_QUEUE_WGS", "BPMD_LONG_SHARE_PCT"))}
        env.update(QUEUE_ENV)
        env.update(extra)
        t0 = time.monotonic()
        r = subprocess.run([sys.executable, "-m", "tests.read_keyed_cases", which], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        wall = time.monotonic() - t0
        # a child that faulted, was killed or could not start ends the test: no further child
        assert r.returncode in (0, 1), (which, extra, r.returncode, r.stderr[-2000:])
        lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        print(f"child {which} {extra}: {wall:.2f} s wall", lines[0])
        assert r.returncode == 0 and lines[0]["mismatches"] == 0, (which, extra, lines[0])
        assert lines[0]["n"] == 4096 and lines[0]["n_long"] >= 16 and lines[0]["n_mid"] >= 16


# ------------------------------------------------- UTF-8 at unit / step edges

@pytest.fixture(scope="module")
def utf8_edges():
    cases = K.utf8_edge_cases()
    return cases, np.array([O.utf8_check(t) for _, t in cases])


def test_utf8_verdicts_at_unit_and_step_edges(utf8_edges):
    """utf8_kernel: one code point of 2, 3 or 4 bytes across every 16-byte unit
    edge and the 1 KiB wave step, at every alignment; intact, cut and broken."""
    import torch
    pmd = _pmd()
    cases, want = utf8_edges
    buf, offs = K.layout([t for _, t in cases], [a for a, _ in cases], random.Random(2))
    b = pmd.Batch(torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda(),
                  torch.tensor(offs, dtype=torch.int64).cuda(),
                  torch.tensor([len(t) for _, t in cases], dtype=torch.int32).cuda())
    got = pmd.utf8_check_batch(b).cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(cases[i][0], len(cases[i][1]), int(got[i]), int(want[i])) for i in bad[:8]]
    assert set(want.tolist()) == {0, 1, 2}


def test_utf8_edges_as_text_of_a_keyed_read(utf8_edges):
    """The same texts deflated, masked and read as text messages, each output
    slot at the text's alignment: BAD_FRAME_PAYLOAD exactly where the oracle's
    checker does not accept the inflated bytes."""
    pmd = _pmd()
    cases, verdict = utf8_edges
    rng = random.Random(3)
    texts = [t for _, t in cases]
    case = K.Case(K.oracle_deflate(texts, 1), [len(t) for t in texts], keys=[rng.getrandbits(32) for _ in texts],
                  text=[1] * len(texts), out_aligns=[a for a, _ in cases])
    want = K.expect(case)
    assert ((want[0] == K.BAD_FRAME_PAYLOAD) == (verdict != 0)).all()
    assert pmd.lib().bpmd_set_inflate_kernel(0) == 0
    r = K.run(case, want)
    assert not r.bad, r.bad[:8]
