#!/usr/bin/env python3
"""Benchmark: device-resident permessage-deflate throughput on MI355X.

Headline workload (BASELINE.json configs[1], "C2"): 64 Ki independent 4 KiB
JSON-like WebSocket payloads per GPU, compressed with compLevel=6,
memLevel=4, windowBits=15 and Beast's pmd framing (impl_base.hpp:85-154),
resident in HBM.  One step = one batched inflate launch over the whole
batch; `value` is that inflate rate.

A plain run (`--gpus N --steps K --warmup W`) does only that: it builds the
C2 inputs, warms up, times the K steps, writes the last step's outputs when
`--dump-outputs DIR` is given, and prints the result line (the contract's
keys, the config, and the roofline from the timed steps' own HIP events).
Everything below runs only with `--full`.

`--dump-outputs DIR` writes what the last timed step returned, as .npy files:
`status` and `out_len` (float32, one entry per message), `out_msg_sum`
(float64, the byte sum of every inflated message), and `out_sample` (float32,
the bytes of a fixed seeded sample of messages, whose indices are in
`out_sample_index`).  The inputs are seeded, so two builds given the same
arguments can be compared output for output.

With `--full` the line also reports the parity check of the C2 output
against the plaintext and, under key "deflate", configs[2] ("C3"): the
round trip of 64 Ki x 4 KiB JSON (seed 0x5EED0003) through the GPU deflater
and back through the GPU inflater -- deflate GiB/s, round-trip GiB/s,
compressed size vs Beast's deflate at the same level.  Key "mixed":
configs[3] ("C4", 1 Mi Zipf 256 B-64 KiB JSON messages at L6/mem4) and
configs[4] ("C5", 16 Ki x 64 KiB binary at L1 and L6): the WHOLE config's
batch is sharded over the ranks in byte-balanced contiguous ranges
(beast_amd/shard.py; strong scaling: at N=1 one GPU runs all of it), GPU
deflate and GPU inflate rates with a byte-exact round-trip check (--no-mixed
skips them).  Key "cpu_baseline": the same C2 payloads (and the C3 messages
for deflate) on the host cores, at 1 thread and at the cores this process
may use, by the C restatement of Beast's zlib ("port") and by the
reference's own zlib 1.3.1 compiled from its sources (oracle/_ref, when
present).

Launch:  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
N > 1 runs under torch.distributed.run (started here as a child process when
no launcher set WORLD_SIZE; under one, WORLD_SIZE must equal N): every rank works on its own 64 Ki
messages (independent streams under no_context_takeover), so there is no
collective on the data path; scaling is weak.  Timing is barrier +
synchronize on both sides, max over ranks.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from beast_amd import pmd, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md)
N_MSGS = 1 << 16
MSG_BYTES = 4096
SEED_C2 = 0x5EED0002
SEED_C3 = 0x5EED0003
SEED_C4 = 0x5EED0004
SEED_C5 = 0x5EED0005


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def pmd_compress_host(data, off, lens, level=6, wbits=15, mem=4):
    """Inputs for the inflate benchmark, produced the way a Beast peer's
    deflater produces them (Flush::none, Flush::block, Flush::sync, strip
    00 00 FF FF).  The system zlib is byte-identical to Beast at these
    settings (tests/test_oracle.py::test_python_zlib_agrees_at_pmd_defaults)."""
    out = []
    mv = memoryview(data)
    for i in range(len(lens)):
        o, n = int(off[i]), int(lens[i])
        c = zlib.compressobj(level, zlib.DEFLATED, -wbits, mem)
        p = c.compress(mv[o:o + n]) + c.flush(zlib.Z_BLOCK) + c.flush(zlib.Z_SYNC_FLUSH)
        out.append(p[:-4])
    return out


def beast_payloads(raw, off, lens, level, mem=4, wbits=15, threads=None):
    """pmd_compress_host over a whole batch on the host's cores: CPython's
    zlib (byte-identical to Beast's deflate_stream at these settings,
    tests/test_oracle.py) releases the GIL while it compresses, so a thread
    pool scales.  These are the payloads a Beast peer sends: blocks every
    lit_bufsize - 1 symbols (deflate_stream.ipp:1406), stored / fixed /
    dynamic as tr_flush_block picks, no sync markers inside a message."""
    from concurrent.futures import ThreadPoolExecutor
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    threads = threads or max(1, min(16, cores))
    mv = memoryview(raw)
    n = len(lens)
    step = max(1, min(4096, n // (4 * threads) or 1))

    def chunk(a):
        out = []
        for i in range(a, min(n, a + step)):
            o, k = int(off[i]), int(lens[i])
            c = zlib.compressobj(level, zlib.DEFLATED, -wbits, mem)
            out.append((c.compress(mv[o:o + k]) + c.flush(zlib.Z_BLOCK) + c.flush(zlib.Z_SYNC_FLUSH))[:-4])
        return out

    with ThreadPoolExecutor(threads) as ex:
        return [p for part in ex.map(chunk, range(0, n, step)) for p in part], threads


def pack(payloads, align=16):
    lens = np.fromiter((len(p) for p in payloads), dtype=np.int64, count=len(payloads))
    slot = (lens + align - 1) // align * align
    off = np.zeros(len(payloads), dtype=np.int64)
    off[1:] = np.cumsum(slot[:-1])
    buf = np.zeros(int(slot.sum()) + 64, dtype=np.uint8)
    for i, p in enumerate(payloads):
        buf[off[i]:off[i] + lens[i]] = np.frombuffer(p, dtype=np.uint8)
    return buf, off, lens.astype(np.int32)


def _median3(fn):
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return sorted(times)[1]


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


CPU_REPS = 5   # median of 5 timed runs per measurement


def _cpu_threads():
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    # T = 32: the per-GPU share of an 8-GPU node's 256 hardware threads,
    # capped at the cores this process may use
    return cores, max(1, min(cores, 32))


def cpu_measure(impl, inflate, data, off, lens, caps, raw_bytes, threads, target_s=0.5, level=6, reps=CPU_REPS):
    """One host-core measurement (oracle.time_batch: outputs preallocated, the
    threads take contiguous message ranges): a probe of 64 messages on one
    thread sizes a sample of ~target_s of work per thread; GiB/s of
    uncompressed bytes, median of `reps` runs.  None when `impl` is absent."""
    from oracle import oracle as O
    n = len(lens)
    probe = min(n, 64)
    pr = O.time_batch(impl, inflate, data, off[:probe], lens[:probe], caps[:probe], threads=1, reps=1, level=level)
    if pr is None:
        return None
    per_msg = max(pr[0] / probe, 1e-9)
    k = int(min(n, max(probe, target_s / per_msg * threads)))
    t, olen = O.time_batch(impl, inflate, data, off[:k], lens[:k], caps[:k], threads=threads, reps=reps, level=level)
    gib = float(np.asarray(raw_bytes[:k], dtype=np.int64).sum()) / (1 << 30)
    return {"value": round(gib / t, 4), "msgs": k, "seconds": round(t, 4), "out_len": olen}


def cpu_baselines(comp_buf, comp_off, comp_len, raw_lens, raw3, off3, len3):
    """Host-core baselines on bounded samples of the C2 payloads (inflate)
    and C3 messages (deflate, L6/mem4/w15 + pmd framing).  Codecs: the
    reference's own zlib 1.3.1 ("reference", compiled from
    test/extern/zlib-1.3.1 by oracle/Makefile) -- Beast's zlib equals it at
    levels 1-9, as the reference's own bench asserts
    (test/bench/zlib/deflate_stream.cpp:147,168), and it is the faster of the
    two, so it is the headline; the C restatement of Beast's zlib ("port",
    oracle/) beside it; the image's system zlib ("system") as an extra
    column.  1 thread and T = 32 threads; median of 5 per measurement."""
    from oracle import oracle as O
    cores, T = _cpu_threads()
    out = {"cpu_model": _cpu_model(), "nproc": os.cpu_count(), "cores_available": cores, "threads": T}
    n = len(comp_len)
    ub = np.full(n, pmd.upper_bound(MSG_BYTES) + 16, dtype=np.uint32)
    raw_c2 = np.full(n, MSG_BYTES, dtype=np.int64)
    for name, inflate in (("inflate", True), ("deflate", False)):
        args = (comp_buf, comp_off, comp_len, raw_lens) if inflate else (raw3, off3, len3, ub)
        r = {}
        for impl, ths in (("reference", (1, T)), ("port", (1, T)), ("system", (T,))):
            row = {}
            for th in ths:
                m = cpu_measure(impl, inflate, *args, raw_c2, th)
                if m is None:
                    break
                row[f"{th}_threads"] = m["value"]
                row[f"sample_{th}"] = f"{m['msgs']} msgs"
                if inflate:   # the sample decodes exactly (every message is 4096 bytes)
                    row["exact"] = bool(row.get("exact", True) and (m["out_len"] == MSG_BYTES).all())
                if not inflate and impl == "port" and th == T:
                    r["_beast_len"] = m["out_len"]   # the port = Beast's deflate: sizes for size_vs_beast
            if row:
                r[impl] = row
        if "system" in r:
            r["system"]["version"] = O.zsys().zref_version().decode()
        if "port" in r and "reference" in r:
            # per-byte time of the port relative to zlib 1.3.1, one core and T threads
            r["t_port_over_t_zlib_1thread"] = round(r["reference"]["1_threads"] / r["port"]["1_threads"], 3)
            r[f"t_port_over_t_zlib_{T}threads"] = round(r["reference"][f"{T}_threads"] / r["port"][f"{T}_threads"], 3)
        out[name] = r
    return out


def _newest(pattern):
    import glob
    import re
    files = glob.glob(os.path.join(ROOT, "profiles", pattern))
    # newest tag: round number, then the letter suffix (r02 < r02b < r02c);
    # file times are no guide in a fresh checkout
    def key(f):
        t = re.match(r"r(\d+)([a-z]*)_", os.path.basename(f))
        return (int(t.group(1)), t.group(2)) if t else (-1, "")
    return max(files, key=key) if files else None


def pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` on the C2 workload, from the newest
    rocprofv3 PMC summary of the C2-only bench (profiles/rNN_c2_pmc.csv,
    scripts/profile.sh) and the FETCH_SIZE calibration of the same run
    (profiles/rNN_fetch_calib.csv: bytes per counted byte for the lane
    kernel's per-lane 16-B reads, measured on a known 2 GiB read).  Counters
    are in KiB.  Returns (bytes, details) or (None, None)."""
    import csv
    f = _newest("r*_c2_pmc.csv")
    if not f:
        return None, None
    fetch, write = [], []
    with open(f) as fh:
        for r in csv.DictReader(fh):
            if r["kernel"].split("::")[-1].split("<")[0] != kernel:
                continue
            try:
                (fetch if r["counter"] == "FETCH_SIZE" else write).append(float(r["value_kB"]) * 1024)
            except (TypeError, ValueError):
                continue
    if not fetch or not write:
        return None, None
    factor, calib = 1.0, None
    c = _newest("r*_fetch_calib.csv")
    if c:
        with open(c) as fh:
            for r in csv.DictReader(fh):
                if r["pattern"] == "lane_slots":
                    factor, calib = float(r["bytes_per_counted_byte"]), os.path.relpath(c, ROOT)
    fb, wb = float(np.median(fetch)), float(np.median(write))
    return int(fb * factor + wb), {"source": os.path.relpath(f, ROOT), "fetch_bytes_raw": int(fb),
                                   "write_bytes": int(wb), "fetch_factor": factor, "fetch_calibration": calib}


# the kernel one step of each profiled op launches once (its launch count is
# the number of steps in the PMC pass)
LEG_ANCHOR = {("c3", "deflate"): "deflate_kernel", ("c4_l6", "deflate"): "stitch_kernel",
              ("c4_l6", "inflate"): "inflate_lane3_kernel", ("c5_l1", "deflate"): "stitch_kernel",
              ("c5_l1", "inflate"): "inflate_lane3_seg_kernel", ("c5_l6", "deflate"): "stitch_kernel",
              ("c5_l6", "inflate"): "inflate_lane3_seg_kernel"}


def pmc_traffic_leg(leg, op):
    """HBM bytes per step of one op of a bench leg, from the newest PMC
    summary of scripts/leg_profile.py (profiles/rNN_<leg>_<op>_pmc.csv: every
    non-torch kernel of that op, FETCH_SIZE and WRITE_SIZE in separate passes)
    with the FETCH_SIZE calibration factor.  Returns (bytes, details) or None."""
    import csv
    f = _newest(f"r*_{leg}_{op}_pmc.csv")
    if not f:
        return None
    fetch = write = 0.0
    anchors = 0
    with open(f) as fh:
        for r in csv.DictReader(fh):
            k = r["kernel"].split("::")[-1].split("<")[0]
            if op == "inflate" and "dfl::" in r["kernel"]:
                continue   # the one setup deflate of scripts/leg_profile.py
            try:
                v = float(r["value_kB"]) * 1024
            except (TypeError, ValueError):
                continue   # a malformed row (never a reason to lose the bench line)
            if r["counter"] == "FETCH_SIZE":
                fetch += v
                anchors += k == LEG_ANCHOR[(leg, op)]
            else:
                write += v
    if not anchors:
        return None
    factor = 1.0
    c = _newest("r*_fetch_calib.csv")
    if c:
        with open(c) as fh:
            for r in csv.DictReader(fh):
                if r["pattern"] == "coalesced_16B":
                    factor = float(r["bytes_per_counted_byte"])
    per = (fetch * factor + write) / anchors
    return int(per), {"source": os.path.relpath(f, ROOT), "steps": anchors,
                      "fetch_bytes_raw_per_step": int(fetch / anchors), "write_bytes_per_step": int(write / anchors),
                      "fetch_factor": factor}


class Timer:
    """K timed steps bracketed by barrier + synchronize; per-step HIP events
    on the launch stream for the kernel-side average."""

    def __init__(self, dist):
        self.dist = dist

    def run(self, step, steps, warmup):
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        if self.dist:
            self.dist.barrier()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        t0 = time.perf_counter()
        for i in range(steps):
            ev[i][0].record()
            step()
            ev[i][1].record()
        torch.cuda.synchronize()
        if self.dist:
            self.dist.barrier()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        # per-step HIP event times on the launch stream, median over the
        # timed steps (the warmup's cold launch is not among them)
        kern_ms = float(np.median([a.elapsed_time(b) for a, b in ev]))
        if self.dist:
            t = torch.tensor([wall, kern_ms], dtype=torch.float64, device="cuda")
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            wall, kern_ms = float(t[0]), float(t[1])
        return wall / steps, kern_ms


C4_MSGS = 1 << 20     # configs[3]: 1 Mi Zipf messages (the whole batch, sharded over the ranks)
C5_MSGS = 16384       # configs[4]: 16 Ki x 64 KiB


def shard_config(lens_all, rank, world):
    """This rank's contiguous, byte-balanced message range of a whole config
    batch and every rank's byte count: (start, end, bytes)."""
    from beast_amd import shard
    ranges = shard.byte_balanced_ranges(lens_all, world)
    s0, e0 = ranges[rank]
    return s0, e0, [int(np.asarray(lens_all[a:b], dtype=np.int64).sum()) for a, b in ranges]


def roofline(alg_bytes, kern_ms, kernels, traffic=None):
    """`roofline` object: algorithmic bytes of one launch (or one step of
    several launches) over its HIP-event time on the launch stream."""
    a = alg_bytes / (kern_ms * 1e-3) / 1e9
    return {"bound": "hbm", "achieved": round(a, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(a / HBM_PEAK_GBS, 5), "traffic": traffic[0] if traffic else None,
            "traffic_source": traffic[1] if traffic else None, "kernel": kernels,
            "kernel_ms": round(kern_ms, 4), "alg_bytes_per_launch": int(alg_bytes)}


DEFLATE_STEP_KERNELS = "deflate_kernel + count_chunks + scan + fill_items + deflate_chunks + stitch"
INFLATE_STEP_KERNELS = {
    "c4_l6": "order_keys + radix sort + inflate_lane3_kernel (work queue; at N >= 2 the long payloads "
             "block-parallel on a side stream: bp_scan + inflate_lane3_seg_kernel + bp_resolve)",
    "c5_l1": "order_keys + radix sort + bp_stats + bp_scan + bp_slots + inflate_lane3_seg_kernel + bp_resolve "
             "(block-parallel)",
    "c5_l6": "order_keys + radix sort + bp_stats + bp_scan + bp_slots + inflate_lane3_seg_kernel + bp_resolve "
             "(block-parallel)"}


def mixed_legs(args, rank, world, timer, dev):
    """configs[3] (C4: Zipf 256 B-64 KiB JSON, L6/mem4) and configs[4] (C5: 64 KiB
    low-compressibility binary, L1 and L6).  Each config is ONE global batch,
    split over the ranks into byte-balanced contiguous message ranges
    (shard.byte_balanced_ranges); each rank synthesizes only
    its own range (seeded by global message index), deflates it on its GPU,
    inflates the payloads back and checks them byte for byte on the device.
    No payload crosses ranks.  Values are GiB/s of uncompressed bytes of the
    whole batch over the max-over-ranks time (strong scaling); each step's
    roofline is its algorithmic bytes over the step's HIP-event time (all of
    its kernels).  At N=1, "virtual_shards" runs every rank's share of an
    N = 2, 4, 8 split alone on this GPU and projects the N-GPU aggregate from
    the slowest share (each rank of a real node has a whole GPU too)."""
    steps = max(1, min(args.steps, 3))
    out = {"steps": steps, "unit": "GiB/s", "scaling": "strong"}
    c4_all = synth.zipf_sizes(args.c4_msgs, SEED_C4)
    c5_all = np.full(args.c5_msgs, 65536, dtype=np.uint32)
    legs = [("c4_l6", "json", c4_all, SEED_C4, 6), ("c5_l1", "binary", c5_all, SEED_C5, 1),
            ("c5_l6", "binary", c5_all, SEED_C5, 6)]
    if args.legs:
        legs = [l for l in legs if l[0] in args.legs.split(",")]
    batches = {}
    host = {}
    for name, kind, lens_all, seed, level in legs:
        s0, e0, per_rank = shard_config(lens_all, rank, world)
        lens = lens_all[s0:e0]
        key = (kind, seed)
        if key not in batches:
            raw, off, ln = synth.make_batch(kind, lens, seed=seed, first=s0)
            batches = {key: pmd.Batch(torch.from_numpy(raw).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
                                      torch.from_numpy(ln.astype(np.int32)).to(dev))}
            host = {key: (raw, off, ln)} if not args.no_beast_payloads else {}
            del raw
        src = batches[key]
        total = int(lens.astype(np.int64).sum())
        total_all = int(lens_all.astype(np.int64).sum())
        ub = lens.astype(np.int64) + (lens.astype(np.int64) + 7) // 8 + (lens.astype(np.int64) + 63) // 64 + 11
        cap = torch.from_numpy(ub.astype(np.int32)).to(dev)
        coff = pmd.slot_offsets(cap)
        cbuf = torch.empty(int(coff[-1].item()) + int(cap[-1].item()) + 64, dtype=torch.uint8, device=dev)

        def deflate_step(a=0, b=len(lens)):
            sub = src if (a, b) == (0, len(lens)) else pmd.Batch(src.data, src.off[a:b], src.len[a:b])
            return pmd.deflate_batch(sub, level=level, mem_level=4, out_cap=cap[a:b], out=cbuf, out_off=coff[a:b])

        d = deflate_step()
        torch.cuda.synchronize()
        comp = pmd.Batch(cbuf, coff, d.out.len.clone())
        rbuf = torch.empty_like(src.data)

        def inflate_step(a=0, b=len(lens)):
            sub = comp if (a, b) == (0, len(lens)) else pmd.Batch(cbuf, coff[a:b], comp.len[a:b])
            return pmd.inflate_batch(sub, src.len[a:b], out=rbuf, out_off=src.off[a:b])

        r = inflate_step()
        torch.cuda.synchronize()
        ok = (int((d.status != 0).sum()) == 0 and int((r.status != 0).sum()) == 0
              and torch.equal(r.out.len, src.len) and torch.equal(rbuf[:total], src.data[:total]))
        if not ok:
            log(f"[rank {rank}] {name} ROUND-TRIP FAILURE")
        d_step, d_kern = timer.run(deflate_step, steps, 1)
        i_step, i_kern = timer.run(inflate_step, steps, 1)
        comp_bytes = int(d.out.len.to(torch.int64).sum())
        alg = total + comp_bytes + 16 * len(lens)
        out[name] = {"msgs": len(lens_all), "bytes": total_all, "msgs_rank0": int(e0 - s0) if rank == 0 else None,
                     "bytes_per_rank": per_rank,
                     "imbalance_max_over_min": round(max(per_rank) / max(1, min(per_rank)), 4),
                     "deflate_value": round(total_all / (1 << 30) / d_step, 3),
                     "inflate_value": round(total_all / (1 << 30) / i_step, 3),
                     "deflate_roofline": roofline(alg, d_kern, DEFLATE_STEP_KERNELS, pmc_traffic_leg(name, "deflate")),
                     "inflate_roofline": roofline(alg, i_kern, INFLATE_STEP_KERNELS[name],
                                                  pmc_traffic_leg(name, "inflate")),
                     "ratio_rank_local": round(comp_bytes / max(1, total), 4), "roundtrip_ok": bool(ok)}
        # the same messages as a Beast peer deflates them (host zlib, this
        # leg's level, memLevel 4): the inflate rate on payloads without this
        # library's sync markers (VERDICT r4 "what's weak" 2)
        bstep = None
        if key in host:
            hraw, hoff, hln = host[key]
            t0 = time.perf_counter()
            bp_list, thr = beast_payloads(hraw, hoff, hln, level)
            t_comp = time.perf_counter() - t0
            bbuf, boff, blen = pack(bp_list)
            del bp_list
            bsrc = pmd.Batch(torch.from_numpy(bbuf).to(dev), torch.from_numpy(boff).to(dev),
                             torch.from_numpy(blen).to(dev))
            bcomp = int(blen.astype(np.int64).sum())
            if rank == 0 and world == 1 and not args.no_cpu_baseline:
                # the leg on the host cores (reference/test/bench/zlib/
                # inflate_stream.cpp:100-125 times Beast's and zlib's inflate
                # of the same payloads): zlib 1.3.1 (= Beast) at T threads,
                # inflate of the Beast payloads, deflate of the messages at the
                # leg's level; bounded samples, median of 5
                _, T = _cpu_threads()
                hcap = hln.astype(np.uint32)
                ci = cpu_measure("reference", True, bbuf, boff.astype(np.uint64), blen.astype(np.uint32), hcap, hln,
                                 T, level=level)
                dub = (hln.astype(np.int64) + (hln.astype(np.int64) + 7) // 8 + (hln.astype(np.int64) + 63) // 64
                       + 16).astype(np.uint32)
                cd = cpu_measure("reference", False, hraw, hoff.astype(np.uint64), hln.astype(np.uint32), dub, hln, T,
                                 level=level)
                if ci and cd:
                    out[name]["cpu_baseline"] = {
                        "kind": "reference", "codec": "zlib 1.3.1 (reference/test/extern, = Beast's zlib)",
                        "cores": T, "unit": "GiB/s", "inflate": ci["value"], "deflate": cd["value"],
                        "inflate_exact": bool((ci["out_len"] == hln[:ci["msgs"]]).all()),
                        "sample": f"inflate {ci['msgs']} / deflate {cd['msgs']} of the leg's messages "
                                  f"(Beast payloads for inflate), median of {CPU_REPS}"}
            del bbuf

            def beast_step(a=0, b=len(lens)):
                sub = bsrc if (a, b) == (0, len(lens)) else pmd.Batch(bsrc.data, bsrc.off[a:b], bsrc.len[a:b])
                return pmd.inflate_batch(sub, src.len[a:b], out=rbuf, out_off=src.off[a:b])

            rb = beast_step()
            torch.cuda.synchronize()
            okb = (int((rb.status != 0).sum()) == 0 and torch.equal(rb.out.len, src.len)
                   and torch.equal(rbuf[:total], src.data[:total]))
            if not okb:
                log(f"[rank {rank}] {name} BEAST-PAYLOAD INFLATE FAILURE")
            bstep, b_kern = timer.run(beast_step, steps, 1)
            out[name].update({
                "inflate_beast_value": round(total_all / (1 << 30) / bstep, 3),
                "inflate_beast_roofline": roofline(total + bcomp + 16 * len(lens), b_kern, INFLATE_STEP_KERNELS[name]),
                "inflate_beast_ok": bool(okb), "beast_ratio_rank_local": round(bcomp / max(1, total), 4),
                "beast_payloads": f"host zlib (= Beast deflate_stream) L{level}/mem4/w15 + pmd framing, "
                                  f"{thr} threads, {t_comp:.1f} s"})
        if world == 1 and not args.no_virtual_shards:
            from beast_amd import shard
            vs = {}
            for parts in (2, 4, 8):
                dt, it, bt = [], [], []
                for a, b in shard.byte_balanced_ranges(lens, parts):
                    dt.append(timer.run(lambda: deflate_step(a, b), steps, 1)[0])
                    it.append(timer.run(lambda: inflate_step(a, b), steps, 1)[0])
                    if bstep is not None:
                        bt.append(timer.run(lambda: beast_step(a, b), steps, 1)[0])
                vs[str(parts)] = {
                    "deflate_shard_ms": [round(t * 1e3, 3) for t in dt],
                    "inflate_shard_ms": [round(t * 1e3, 3) for t in it],
                    "deflate_projected_value": round(total / (1 << 30) / max(dt), 3),
                    "inflate_projected_value": round(total / (1 << 30) / max(it), 3),
                    "deflate_projected_speedup": round(d_step / max(dt), 3),
                    "inflate_projected_speedup": round(i_step / max(it), 3)}
                if bt:
                    vs[str(parts)].update({
                        "inflate_beast_shard_ms": [round(t * 1e3, 3) for t in bt],
                        "inflate_beast_projected_value": round(total / (1 << 30) / max(bt), 3),
                        "inflate_beast_projected_speedup": round(bstep / max(bt), 3)})
            out[name]["virtual_shards"] = vs
        if bstep is not None:
            del bsrc, rb
        del cbuf, rbuf, comp, d, r
    return out


LINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
             "vs_baseline", "dtype", "data", "config", "parity_ok")

DUMP_SAMPLE_MSGS = 2048      # --dump-outputs: messages whose bytes are written whole (32 MiB as float32)
DUMP_SAMPLE_SEED = 0x5EED00D0


def plain_line(result):
    """The stdout line of a plain run: the contract's keys, the config and the
    C2 roofline from the timed steps' own HIP events."""
    line = {k: result[k] for k in LINE_KEYS if k in result and k != "parity_ok"}   # no parity check ran
    line["roofline"] = result["roofline"]
    return line


def dump_outputs(dirname, res, out, n, rank, world):
    """--dump-outputs: what the last timed inflate step returned (`res`, whose
    bytes are in `out`, one MSG_BYTES slot per message), as DIR/<name>.npy in
    float32 / float64: status and length of every message, the byte sum of
    every message, and the bytes of a fixed seeded sample of messages."""
    os.makedirs(dirname, exist_ok=True)
    torch.cuda.synchronize()
    msgs = out[: n * MSG_BYTES].view(n, MSG_BYTES)
    sums = torch.cat([msgs[a:a + 4096].sum(dim=1, dtype=torch.int64) for a in range(0, n, 4096)])
    idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, size=min(n, DUMP_SAMPLE_MSGS), replace=False))
    sample = msgs[torch.from_numpy(idx).to(out.device)]
    arrays = {"status": res.status.cpu().numpy().astype(np.float32),
              "out_len": res.out.len.cpu().numpy().astype(np.float32),
              "out_msg_sum": sums.cpu().numpy().astype(np.float64),
              "out_sample_index": idx.astype(np.float64),
              "out_sample": sample.cpu().numpy().astype(np.float32)}
    suffix = f"_rank{rank}" if world > 1 else ""
    for name, a in arrays.items():
        np.save(os.path.join(dirname, f"{name}{suffix}.npy"), a)


def compact_line(full):
    """The bench's stdout line: the contract's keys, the C2 roofline and CPU
    baseline, and every north-star number (C3 deflate and size, C4 / C5
    deflate, inflate of this library's and of a Beast peer's payloads, the
    projected 2 / 4 / 8-way speed-ups, the legs' CPU columns, parity).  The
    whole record goes to gpurun_out/bench_detail.json."""
    line = {k: full[k] for k in LINE_KEYS if k in full}
    rf = dict(full["roofline"])
    src = rf.pop("traffic_source", None)
    rf["traffic_source"] = src.get("source") if isinstance(src, dict) else src
    line["roofline"] = rf
    cb = full.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind", "sample", "one_thread")}
        line["cpu_baseline"]["port_value"] = (cb.get("port") or {}).get("value")
        line["cpu_baseline"]["cpu_model"] = cb.get("cpu_model")
    ns = {"c2_inflate": full["value"]}
    ok = [bool(full.get("parity_ok"))]
    d = full.get("deflate")
    if d:
        ns["c3"] = {"deflate": d["deflate_value"], "roundtrip": d["roundtrip_value"],
                    "inflate_own": d["inflate_of_gpu_payloads_value"], "size_vs_beast": d.get("size_vs_beast"),
                    "deflate_frac": d["roofline"]["frac"],
                    "exact_deflate": (d.get("exact") or {}).get("deflate_value"),
                    "exact_same_size": (d.get("exact") or {}).get("same_size_as_beast"),
                    "cpu_deflate": (d.get("cpu_baseline") or {}).get("value")}
        ok.append(bool(d["roundtrip_ok"]))
    fr = full.get("frame")
    if fr:
        ns["n1"] = {"read": fr["read_value"], "utf8": fr["utf8_value"], "mask": fr["mask_value"],
                    "frame": fr["frame_value"]}
        ok += [bool(fr["read_ok"]), bool(fr["utf8_ok"]), bool(fr["frame_ok"])]
    for leg, m in (full.get("mixed") or {}).items():
        if not isinstance(m, dict) or "deflate_value" not in m:
            continue
        e = {"deflate": m["deflate_value"], "inflate": m["inflate_value"], "inflate_beast": m.get("inflate_beast_value"),
             "ratio": m["ratio_rank_local"], "beast_ratio": m.get("beast_ratio_rank_local"),
             "inflate_frac": m["inflate_roofline"]["frac"], "deflate_frac": m["deflate_roofline"]["frac"]}
        if m.get("beast_ratio_rank_local"):
            e["size_vs_beast"] = round(m["ratio_rank_local"] / m["beast_ratio_rank_local"], 4)
        vs = m.get("virtual_shards")
        if vs:
            # projected N-GPU speed-ups, N = 2, 4, 8: [deflate, inflate, inflate of Beast payloads]
            e["x_projected"] = {n: [v.get("deflate_projected_speedup"), v.get("inflate_projected_speedup"),
                                    v.get("inflate_beast_projected_speedup")] for n, v in vs.items()}
            e["shard8_ms_max"] = [max(vs["8"]["deflate_shard_ms"]), max(vs["8"]["inflate_shard_ms"]),
                                  max(vs["8"].get("inflate_beast_shard_ms") or [0])]
        if m.get("cpu_baseline"):
            e["cpu"] = {"inflate": m["cpu_baseline"]["inflate"], "deflate": m["cpu_baseline"]["deflate"],
                        "cores": m["cpu_baseline"]["cores"]}
        ns[leg] = e
        ok += [bool(m["roundtrip_ok"]), bool(m.get("inflate_beast_ok", True))]
    line["parity_ok"] = all(ok)
    line["north_star"] = ns
    line["detail"] = "gpurun_out/bench_detail.json"
    return line


def launch_cmd(argv, n, port, python=sys.executable, script=None):
    """The command that runs this bench as N ranks of one node (one process
    per GPU, the driver's own form): torch.distributed.run over 127.0.0.1,
    the same bench arguments (--gpus included, so every rank checks WORLD_SIZE
    against it)."""
    return [python, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
            "--master-addr=127.0.0.1", f"--master-port={port}", script or os.path.abspath(__file__), *argv]


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def maybe_launch(args, argv):
    """`--gpus N` without a launcher: start N ranks under torch.distributed.run
    as a CHILD process (nothing here has touched the GPU yet; no exec) and
    return its exit code.  Under a launcher, WORLD_SIZE must equal N.
    Returns None when this process is itself the (only or a) rank."""
    ws = os.environ.get("WORLD_SIZE")
    if ws is not None:
        if int(ws) != args.gpus:
            log(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={ws}")
            return 2
        return None
    if args.gpus <= 1:
        return None
    import subprocess
    return subprocess.run(launch_cmd(argv, args.gpus, _free_port())).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--msgs", type=int, default=N_MSGS)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (see the module docstring)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything besides the headline: the C2 parity check, the frame passes, C3, the "
                         "C4 / C5 legs, the CPU baselines and the PMC traffic lookup (the --no-* options trim it)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-exact", action="store_true", help="skip the exact-mode (BPMD_F_EXACT) deflate leg")
    ap.add_argument("--no-deflate", action="store_true")
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--no-mixed", action="store_true")
    ap.add_argument("--legs", default="", help="comma list of mixed legs to run (c4_l6,c5_l1,c5_l6); default all")
    ap.add_argument("--no-beast-payloads", action="store_true",
                    help="skip the mixed legs' inflate of Beast-produced (host zlib) payloads")
    ap.add_argument("--no-virtual-shards", action="store_true",
                    help="skip the N=1 per-shard timing that projects the 2/4/8-GPU aggregate")
    ap.add_argument("--c4-msgs", type=int, default=C4_MSGS, help="configs[3] batch (all ranks together)")
    ap.add_argument("--c5-msgs", type=int, default=C5_MSGS, help="configs[4] batch (all ranks together)")
    args = ap.parse_args()
    if not args.full:   # a plain run: the headline only
        args.no_cpu_baseline = args.no_deflate = args.no_frame = args.no_mixed = True
    rc = maybe_launch(args, sys.argv[1:])
    if rc is not None:
        sys.exit(rc)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    # BPMD_BENCH_BACKEND=gloo rehearses the multi-rank logic with several ranks
    # on one GPU (RCCL refuses two ranks on one device); the driver's runs use
    # nccl (= RCCL), one rank per GPU
    backend = os.environ.get("BPMD_BENCH_BACKEND", "nccl")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if backend != "nccl":
        local %= max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    timer = Timer(dist)
    dev = torch.device("cuda", local)
    n = args.msgs
    lens = np.full(n, MSG_BYTES, dtype=np.uint32)

    # ------------------------------------------------------------ C2 inflate
    t0 = time.perf_counter()
    raw, raw_off, raw_len = synth.make_batch("json", lens, seed=SEED_C2, first=rank * n)
    payloads = pmd_compress_host(raw, raw_off, raw_len)
    comp_buf, comp_off, comp_len = pack(payloads)
    log(f"[rank {rank}] C2 inputs ready in {time.perf_counter() - t0:.1f}s, ratio "
        f"{comp_len.sum() / raw_len.astype(np.int64).sum():.4f}")
    src = pmd.Batch(torch.from_numpy(comp_buf).to(dev), torch.from_numpy(comp_off).to(dev),
                    torch.from_numpy(comp_len).to(dev))
    cap = torch.full((n,), MSG_BYTES, dtype=torch.int32, device=dev)
    out_off = pmd.slot_offsets(cap)
    out = torch.empty(n * MSG_BYTES + 64, dtype=torch.uint8, device=dev)

    last = [None]   # what the newest step returned (--dump-outputs writes the last timed step's)

    def inflate_step():
        last[0] = pmd.inflate_batch(src, cap, out=out, out_off=out_off)
        return last[0]

    r = inflate_step()
    torch.cuda.synchronize()
    ok = None
    if args.full:
        ok = int((r.status != 0).sum()) == 0 and torch.equal(
            out[: n * MSG_BYTES].view(n, MSG_BYTES), torch.from_numpy(raw.reshape(n, MSG_BYTES)).to(dev))
        if not ok:
            log(f"[rank {rank}] C2 PARITY FAILURE")
    step_s, kern_ms = timer.run(inflate_step, args.steps, args.warmup)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last[0], out, n, rank, world)
    last[0] = None

    uncomp = n * MSG_BYTES
    comp = int(comp_len.astype(np.int64).sum())
    value = uncomp * world / (1 << 30) / step_s
    alg_bytes = comp + uncomp + 16 * n
    achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
    kname = "inflate_lane3_kernel" if n >= 2048 else "inflate_kernel"   # bpmd_set_inflate_kernel(0) policy
    traffic, traffic_src = pmc_traffic(kname) if args.full and n == N_MSGS else (None, None)
    # (traffic_src: the PMC file, its raw FETCH/WRITE bytes and the FETCH calibration used)
    result = {
        "metric": "GiB/s device-resident inflate+deflate over batched WS payloads, 1/2/4/8 GPU",
        "value": round(value, 3),
        "unit": "GiB/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(step_s * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic (seeded JSON-like text, compressed host-side with zlib L6/mem4/w15 + pmd framing)",
        "config": {"workload": "C2 inflate-only: 64Ki x 4KiB payloads/GPU, compLevel=6, memLevel=4, windowBits=15",
                   "msgs_per_gpu": n, "msg_bytes": MSG_BYTES, "compressed_bytes_per_gpu": comp,
                   "parallelism": f"dp{world} (independent message shards)"},
        "parity_ok": None if ok is None else bool(ok),
        "roofline": {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                     "traffic_source": traffic_src,
                     "kernel": kname, "kernel_ms": round(kern_ms, 4),
                     "alg_bytes_per_launch": alg_bytes},
    }

    # ---------------------------------- N1 frame passes on the same C2 batch
    if not args.no_frame:
        g = torch.Generator().manual_seed(0x5EED0011 + rank)
        keys = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, generator=g).to(dev)
        text = torch.ones(n, dtype=torch.uint8, device=dev)
        msrc = pmd.Batch(src.data.clone(), src.off, src.len)
        pmd.mask_batch(msrc, keys)   # the clients' masked frames

        def read_step():
            return pmd.read_batch(msrc, cap, key=keys, text=text, out=out, out_off=out_off)

        rr = read_step()
        torch.cuda.synchronize()
        ref_dev = torch.from_numpy(raw.reshape(n, MSG_BYTES)).to(dev)
        okr = int((rr.status != 0).sum()) == 0 and torch.equal(out[: n * MSG_BYTES].view(n, MSG_BYTES), ref_dev)
        r_step, _ = timer.run(read_step, args.steps, args.warmup)
        ob = pmd.Batch(out, out_off, rr.out.len)
        ures = torch.empty(n, dtype=torch.int32, device=dev)

        def utf8_step():
            return pmd.utf8_check_batch(ob, result=ures)

        u_step, u_kern = timer.run(utf8_step, args.steps, args.warmup)
        oku = int((ures != 0).sum()) == 0

        def mask_step():
            pmd.mask_batch(msrc, keys)

        m_step, m_kern = timer.run(mask_step, args.steps, args.warmup)
        # client send framing of the same payloads (bpmd_frame_batch): 4 KiB
        # frames, RSV1, a key per frame, masked on the way out
        fplan = pmd.frame_plan(src, 4096, masked=True)
        fkeys = torch.randint(-2**31, 2**31 - 1, (fplan["n_keys"],), dtype=torch.int32, generator=g).to(dev)
        fwire = torch.empty(fplan["total"] + 16, dtype=torch.uint8, device=dev)
        fop = torch.ones(n, dtype=torch.uint8, device=dev)

        def frame_step():
            return pmd.frame_batch(src, 4096, op=fop, compressed=True, keys=fkeys, plan=fplan, wire=fwire)

        f_step, f_kern = timer.run(frame_step, args.steps, args.warmup)
        fw = pmd.frame_batch(src, 4096, op=fop, compressed=True, keys=fkeys, plan=fplan, wire=fwire)
        torch.cuda.synchronize()
        i0 = n // 3   # spot check one message against the oracle-free header layout
        w0 = fw.message(i0)
        okf = (w0[0] & 0xC0) == 0xC0 and len(w0) == int(fplan["sizes"][i0])
        fbytes = comp + int(fplan["total"])
        result["frame"] = {
            "workload": "C2 payloads as masked client text frames: fused unmask+inflate+UTF-8 (bpmd_read_batch); "
                        "UTF-8 check of the 256 MiB inflated batch; in-place mask of the compressed batch; "
                        "client framing of the compressed batch (bpmd_frame_batch, 4 KiB frames, a key per frame)",
            "read_value": round(uncomp * world / (1 << 30) / r_step, 3), "read_ms_per_step": round(r_step * 1e3, 4),
            "read_ok": bool(okr),
            "utf8_value": round(uncomp * world / (1 << 30) / u_step, 3), "utf8_ok": bool(oku),
            "utf8_roofline": {"bound": "hbm", "achieved": round((uncomp + 16 * n) / (u_kern * 1e-3) / 1e9, 2),
                              "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": round((uncomp + 16 * n) / (u_kern * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                              "kernel": "utf8_kernel", "kernel_ms": round(u_kern, 4)},
            "mask_value": round(comp * world / (1 << 30) / m_step, 3),
            "mask_roofline": {"bound": "hbm", "achieved": round((2 * comp + 16 * n) / (m_kern * 1e-3) / 1e9, 2),
                              "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": round((2 * comp + 16 * n) / (m_kern * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                              "kernel": "mask_kernel", "kernel_ms": round(m_kern, 4)},
            "frame_value": round(comp * world / (1 << 30) / f_step, 3), "frame_ok": bool(okf),
            "frame_roofline": {"bound": "hbm", "achieved": round((fbytes + 32 * n) / (f_kern * 1e-3) / 1e9, 2),
                               "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": round((fbytes + 32 * n) / (f_kern * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                               "kernel": "frame_kernel", "kernel_ms": round(f_kern, 4)},
            "unit": "GiB/s (mask, frame: of compressed bytes)",
        }
        if not (okr and oku):
            log(f"[rank {rank}] FRAME PARITY FAILURE read={okr} utf8={oku}")
        del msrc, ob, rr, fw, fwire
    del src, out, r

    # ------------------------------------------------- C3 deflate round trip
    if not args.no_deflate:
        raw3, off3, len3 = synth.make_batch("json", lens, seed=SEED_C3, first=rank * n)
        src3 = pmd.Batch(torch.from_numpy(raw3).to(dev), torch.from_numpy(off3.astype(np.int64)).to(dev),
                         torch.from_numpy(len3.astype(np.int32)).to(dev))
        ub = pmd.upper_bound(MSG_BYTES)
        cap3 = torch.full((n,), ub, dtype=torch.int32, device=dev)
        off3o = pmd.slot_offsets(cap3)
        out3 = torch.empty(int(off3o[-1].item()) + ub + 64, dtype=torch.uint8, device=dev)

        def deflate_step():
            return pmd.deflate_batch(src3, level=6, mem_level=4, out_cap=cap3, out=out3, out_off=off3o)

        d = deflate_step()
        torch.cuda.synchronize()
        comp_b = pmd.Batch(out3, off3o, d.out.len.clone())
        cap_in = torch.full((n,), MSG_BYTES, dtype=torch.int32, device=dev)
        rt_off = pmd.slot_offsets(cap_in)
        rt_out = torch.empty(n * MSG_BYTES + 64, dtype=torch.uint8, device=dev)

        def reinflate_step():
            return pmd.inflate_batch(comp_b, cap_in, out=rt_out, out_off=rt_off)

        rr = reinflate_step()
        torch.cuda.synchronize()
        ok3 = (int((d.status != 0).sum()) == 0 and int((rr.status != 0).sum()) == 0
               and torch.equal(rt_out[: n * MSG_BYTES].view(n, MSG_BYTES), src3.data[: n * MSG_BYTES].view(n, MSG_BYTES)))
        if not ok3:
            log(f"[rank {rank}] C3 ROUND-TRIP FAILURE")
        gpu_len = d.out.len.cpu().numpy().astype(np.int64)
        d_step, d_kern = timer.run(deflate_step, args.steps, args.warmup)
        i_step, i_kern = timer.run(reinflate_step, args.steps, args.warmup)
        comp3 = int(gpu_len.sum())
        dval = uncomp * world / (1 << 30) / d_step
        dalg = uncomp + comp3 + 16 * n
        result["deflate"] = {
            "workload": "C3 round trip: 64Ki x 4KiB JSON/GPU (seed 0x5EED0003), GPU deflate L6 then GPU inflate",
            "deflate_value": round(dval, 3), "deflate_ms_per_step": round(d_step * 1e3, 4),
            "roundtrip_value": round(uncomp * world / (1 << 30) / (d_step + i_step), 3),
            "inflate_of_gpu_payloads_value": round(uncomp * world / (1 << 30) / i_step, 3),
            "unit": "GiB/s", "roundtrip_ok": bool(ok3),
            "ratio": round(comp3 / uncomp, 4),
            "roofline": roofline(dalg, d_kern, "deflate_kernel", pmc_traffic_leg("c3", "deflate")),
        }
        exact_len = None
        if not args.no_exact:
            # BPMD_F_EXACT: the reference's own parse, blocks and trees, bit for bit
            def exact_step():
                return pmd.deflate_batch(src3, level=6, mem_level=4, out_cap=cap3, out=out3, out_off=off3o, exact=True)

            ex = exact_step()
            torch.cuda.synchronize()
            exact_len = ex.out.len.cpu().numpy().astype(np.int64)
            e_ok = int((ex.status != 0).sum()) == 0
            e_step, _ = timer.run(exact_step, min(args.steps, 3), 1)
            result["deflate"]["exact"] = {
                "deflate_value": round(uncomp * world / (1 << 30) / e_step, 3),
                "ms_per_step": round(e_step * 1e3, 3), "ratio": round(int(exact_len.sum()) / uncomp, 4),
                "status_ok": bool(e_ok), "steps": min(args.steps, 3),
                "mode": "BPMD_F_EXACT (bit-identical to Beast's deflate_stream; tests/test_gpu_deflate_exact.py)"}
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            cpu = cpu_baselines(comp_buf, comp_off, comp_len, raw_len.astype(np.uint32), raw3, off3, len3)
            dcpu = cpu["deflate"]
            beast_len = dcpu.pop("_beast_len", None)
            if beast_len is not None:
                k = len(beast_len)
                result["deflate"]["size_vs_beast"] = round(float(gpu_len[:k].sum()) / float(beast_len.sum()), 4)
                if exact_len is not None:
                    result["deflate"]["exact"]["same_size_as_beast"] = f"{int((exact_len[:k] == beast_len).sum())}/{k}"
                result["deflate"]["size_sample"] = f"first {k} messages, Σ GPU bytes / Σ Beast bytes at L6/mem4"
            if "reference" in dcpu:
                T = cpu["threads"]
                result["deflate"]["cpu_baseline"] = {
                    "value": dcpu["reference"][f"{T}_threads"], "unit": "GiB/s", "cores": T, "kind": "reference",
                    "sample": f"C3 messages, {dcpu['reference'][f'sample_{T}']}, L6/mem4/w15 + pmd framing, "
                              f"zlib 1.3.1 (= Beast), median of {CPU_REPS}",
                    "one_thread": dcpu["reference"]["1_threads"], "port": dcpu.get("port"),
                    "system_zlib": dcpu.get("system")}
        del src3, out3, rt_out, d, rr

    # --------------------------------- C4 / C5 shapes (configs[3], configs[4])
    if not args.no_mixed:
        result["mixed"] = mixed_legs(args, rank, world, timer, dev)

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        if args.no_deflate:
            cpu = cpu_baselines(comp_buf, comp_off, comp_len, raw_len.astype(np.uint32), raw, raw_off, raw_len)
        icpu = cpu["inflate"]
        T = cpu["threads"]
        if "reference" in icpu:
            ref_, port_ = icpu["reference"], icpu.get("port") or {}
            result["cpu_baseline"] = {
                "value": ref_[f"{T}_threads"], "unit": "GiB/s", "cores": T, "kind": "reference",
                "sample": f"C2 payloads, {ref_[f'sample_{T}']} x {MSG_BYTES} B, zlib 1.3.1 of the reference "
                          f"(oracle/_ref; = Beast's zlib), {T} threads, median of {CPU_REPS}",
                "one_thread": ref_["1_threads"], "exact": ref_.get("exact"),
                "port": {"value": port_.get(f"{T}_threads"), "one_thread": port_.get("1_threads"),
                         "t_port_over_t_zlib_1thread": icpu.get("t_port_over_t_zlib_1thread"),
                         f"t_port_over_t_zlib_{T}threads": icpu.get(f"t_port_over_t_zlib_{T}threads")},
                "system_zlib": (icpu.get("system") or {}).get(f"{T}_threads"),
                "cpu_model": cpu["cpu_model"], "nproc": cpu["nproc"], "cores_available": cpu["cores_available"]}
    if rank == 0 and not args.full:
        print(json.dumps(plain_line(result)), flush=True)
    elif rank == 0:
        # the whole record to a side file; stdout gets one line under ~4 KB
        # with every north-star number (the driver keeps only a tail of it)
        try:
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            with open(os.path.join(ROOT, "gpurun_out", "bench_detail.json"), "w") as fh:
                json.dump(result, fh)
        except OSError:
            pass
        print(json.dumps(compact_line(result)), flush=True)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
