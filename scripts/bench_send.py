"""Time of the batch send side (bpmd_send_batch) on one GPU, client role, over
the shapes of scripts/bench_unframe.py:

    python scripts/bench_send.py --shape a    64 Ki JSON messages of 4 KiB (bench.py C2's messages),
                                              each compressed and sent as one masked frame
    python scripts/bench_send.py --shape b    16 Ki messages of 64 KiB random bytes in masked 4 KiB frames

Two comparisons per shape, each printed as one JSON line:

  whole     bpmd_send_batch against the path a caller had before it on the
            same inputs: pmd.deflate_batch + pmd.frame_plan + pmd.frame_batch.
            That path waits on the host (frame_plan reads the deflated lengths
            back), so it is timed with a host clock around a final
            synchronise; bpmd_send_batch with HIP events and, for the same
            footing, with the host clock too.
  framing   the size, scan and frame kernels (steps 3-5 of bpmd_send_batch)
            against bpmd_frame_batch with a precomputed plan over the
            identical deflated payloads, alternated in the same run.  The
            yardstick's own spread is max/min of its repeated medians.

Times are HIP events around `--inner` back-to-back calls after `--warmup`
untimed rounds; a figure is the median of `--repeats` rounds."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from beast_amd import pmd, synth  # noqa: E402


def timed(fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return float(np.median(ms))


def timed_host(fn, warmup, repeats):
    """wall time of one call followed by a synchronise"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def shape_a(n):
    lens = np.full(n, bench.MSG_BYTES, dtype=np.uint32)
    raw, off, ln = synth.make_batch("json", lens, seed=bench.SEED_C2)
    src = pmd.Batch.from_arrays(raw, off, ln)
    return src, 1 << 20, f"{n} JSON messages of {bench.MSG_BYTES} B, compressed, one masked frame each"


def shape_b(n, size=65536):
    g = torch.Generator(device="cuda").manual_seed(0xB)
    data = torch.randint(0, 256, (n * size + 16,), dtype=torch.uint8, device="cuda", generator=g)
    src = pmd.Batch(data, torch.arange(n, dtype=torch.int64, device="cuda") * size,
                    torch.full((n,), size, dtype=torch.int32, device="cuda"))
    return src, 4096, f"{n} messages of {size} random bytes, compressed, masked 4 KiB frames"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["a", "b"], required=True)
    ap.add_argument("--msgs", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=0)
    ap.add_argument("--blocks", type=int, default=3, help="repeated medians of the framing comparison")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    src, frame_max, what = shape_a(args.msgs or 65536) if args.shape == "a" else shape_b(args.msgs or 16384)
    inner = args.inner or (20 if args.shape == "a" else 2)
    n = src.n
    dev = src.data.device
    L, P, S = pmd._send_lib(), pmd._ptr, pmd._stream_handle(None)

    # ---- buffers of the new path, sized from the input lengths alone
    fb, wb = pmd.send_bounds(src.len, frame_max, True, True, True)
    key_bound = (torch.cumsum(fb, 0) - fb).to(torch.int32)
    g = torch.Generator(device="cuda").manual_seed(7)
    keys = torch.randint(-2**31, 2**31 - 1, (int(fb.sum().item()),), dtype=torch.int32, device=dev, generator=g)
    ln = src.len.to(torch.int64)
    zcap = (ln + (ln + 7) // 8 + (ln + 63) // 64 + 11).to(torch.int32)
    zoff = pmd.slot_offsets(zcap)
    z = torch.empty(int(zoff[-1].item() + zcap[-1].item()) + 16, dtype=torch.uint8, device=dev)
    zlen = torch.zeros(n, dtype=torch.int32, device=dev)
    wire_cap = int(wb.sum().item())
    wire = torch.zeros(wire_cap + 16, dtype=torch.uint8, device=dev)
    w_off = torch.zeros(n, dtype=torch.int64, device=dev)
    w_len = torch.zeros(n, dtype=torch.int32, device=dev)
    comp = torch.zeros(n, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    cfg = pmd._Cfg(6, 15, 4, 0, 0)

    def send_c(kb=key_bound):
        assert L.bpmd_send_batch(ctypes.byref(cfg), P(src.data), P(src.off), P(src.len), n, pmd.ROLE_CLIENT, 1, 0, 1,
                                 frame_max, None, None, P(z), P(zoff), P(zcap), P(zlen), P(keys), P(kb), P(wire),
                                 wire_cap, P(w_off), P(w_len), P(comp), P(status), P(total), S) == 0

    # ---- the path before bpmd_send_batch
    zres = pmd.deflate_batch(src, out_cap=zcap, out=z.clone(), out_off=zoff)
    torch.cuda.synchronize()

    def parent():
        d = pmd.deflate_batch(src, out_cap=zcap, out=zres.out.data, out_off=zoff)
        plan = pmd.frame_plan(d.out, frame_max, masked=True)
        return pmd.frame_batch(d.out, frame_max, op=2, compressed=True, keys=keys, plan=plan), plan

    ref, plan = parent()
    torch.cuda.synchronize()
    # with the plan's exact key bases both paths write the same bytes
    kb = plan["key_base"]
    send_c(kb)
    torch.cuda.synchronize()
    tot = int(total.item())
    ok = bool(tot == plan["total"] and torch.equal(w_off, plan["woff"]) and torch.equal(w_len, plan["sizes"])
              and torch.equal(wire[:tot], ref.data[:tot]) and not status.any() and bool(comp.all())
              and torch.equal(zlen, zres.out.len))
    payload = int(src.len.to(torch.int64).sum().item())
    base = {"shape": args.shape, "what": what, "ok": ok, "messages": n, "frames": int(plan["n_keys"]),
            "input_bytes": payload, "deflated_bytes": int(zlen.to(torch.int64).sum().item()), "wire_bytes": tot,
            "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}

    t_send_ev = timed(send_c, args.warmup, args.repeats, inner)
    t_send_host = timed_host(send_c, args.warmup, args.repeats)
    t_parent_host = timed_host(parent, args.warmup, args.repeats)
    print(json.dumps({**base, "compare": "whole", "inner": inner, "send_batch_ms_events": t_send_ev,
                      "send_batch_ms_host": t_send_host, "deflate_plan_frame_ms_host": t_parent_host,
                      "parent_over_send_host": round(t_parent_host / t_send_host, 3)}), flush=True)

    # ---- the framing part alone over the identical deflated payloads
    zb = zres.out
    fa = (P(zb.data), P(zb.off), P(zb.len), None, None, P(keys), P(kb), frame_max, n, P(ref.data), P(plan["woff"]), S)
    ones = torch.ones(n, dtype=torch.uint8, device=dev)
    sa = (P(src.data), P(src.off), P(src.len), n, pmd.ROLE_CLIENT, 1, 1, frame_max, None, P(zb.data), P(zb.off),
          P(zb.len), P(keys), P(kb), P(wire), wire_cap, P(w_off), P(w_len), P(ones), P(status), P(total), S)

    def frame_c():
        assert L.bpmd_frame_batch(*fa) == 0

    def frames_c():
        assert L.bpmd_internal_send_frames(*sa) == 0

    status.zero_()
    meds = {"frame_batch": [], "send_frames": []}
    for _ in range(args.blocks):
        meds["frame_batch"].append(timed(frame_c, args.warmup, args.repeats, inner))
        meds["send_frames"].append(timed(frames_c, args.warmup, args.repeats, inner))
    torch.cuda.synchronize()
    ok2 = bool(torch.equal(wire[:tot], ref.data[:tot]) and not status.any())
    mid = {k: float(np.median(v)) for k, v in meds.items()}
    print(json.dumps({**base, "ok": ok and ok2, "compare": "framing", "inner": inner, "medians_ms": meds,
                      "yardstick_spread": round(max(meds["frame_batch"]) / min(meds["frame_batch"]), 4),
                      "send_frames_over_frame_batch": round(mid["send_frames"] / mid["frame_batch"], 4),
                      "frame_batch_GiBps": round(tot / (mid["frame_batch"] * 1e-3) / 2**30, 2),
                      "send_frames_GiBps": round(tot / (mid["send_frames"] * 1e-3) / 2**30, 2)}), flush=True)
    sys.exit(0 if ok and ok2 else 1)


if __name__ == "__main__":
    main()
