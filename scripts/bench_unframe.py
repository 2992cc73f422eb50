"""Rate of the receive side's frame pass (bpmd_unframe_batch) beside the mask
pass (bpmd_mask_batch) over the same payload bytes, on one GPU.  The mask pass
reads and writes each payload byte once, as the frame pass does apart from the
headers, so it is the yardstick.

    python scripts/bench_unframe.py --shape a    64 Ki messages of the headline workload's compressed
                                                  payloads (bench.py C2), one masked frame each
    python scripts/bench_unframe.py --shape b    16 Ki payloads of 64 KiB in masked 4 KiB frames

Times are HIP events around `--inner` back-to-back calls, after `--warmup`
untimed rounds; the figure is the median of `--repeats` rounds.  Prints one
JSON line per shape.  Rates are payload bytes per second (GiB/s)."""
import argparse
import json
import os
import sys

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
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def shape_a(n):
    lens = np.full(n, bench.MSG_BYTES, dtype=np.uint32)
    raw, off, ln = synth.make_batch("json", lens, seed=bench.SEED_C2)
    payloads, _ = bench.beast_payloads(raw, off, ln, 6)
    buf, poff, plen = bench.pack(payloads)
    src = pmd.Batch(torch.from_numpy(buf).cuda(), torch.from_numpy(poff).cuda(), torch.from_numpy(plen).cuda())
    return src, 1 << 20, f"{n} compressed payloads of 4 KiB JSON messages, one masked frame each"


def shape_b(n, size=65536):
    g = torch.Generator(device="cuda").manual_seed(0xB)
    data = torch.randint(0, 256, (n * size + 16,), dtype=torch.uint8, device="cuda", generator=g)
    src = pmd.Batch(data, torch.arange(n, dtype=torch.int64, device="cuda") * size,
                    torch.full((n,), size, dtype=torch.int32, device="cuda"))
    return src, 4096, f"{n} payloads of {size} B in masked 4 KiB frames"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["a", "b"], required=True)
    ap.add_argument("--msgs", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    src, frame_max, what = shape_a(args.msgs or 65536) if args.shape == "a" else shape_b(args.msgs or 16384)
    inner = args.inner or (20 if args.shape == "a" else 2)
    n = src.n
    g = torch.Generator(device="cuda").manual_seed(7)
    nk = int(pmd.frame_counts(src.len, frame_max).sum().item())
    keys = torch.randint(-2**31, 2**31 - 1, (nk,), dtype=torch.int32, device="cuda", generator=g)
    wire = pmd.frame_batch(src, frame_max, op=2, compressed=True, keys=keys)
    cap = src.len.clone()
    out_off = pmd.slot_offsets(cap)
    out = torch.zeros(int(out_off[-1].item() + cap[-1].item()) + 16, dtype=torch.uint8, device="cuda")
    state = pmd.rd_state(n)

    def unframe():
        return pmd.unframe_batch(wire, cap, pmd.ROLE_SERVER, state=state, out=out, out_off=out_off)

    u = unframe()
    torch.cuda.synchronize()
    ok = bool((u.event == pmd.EV_MESSAGE).all() and (u.status == 0).all() and torch.equal(u.out.len, src.len)
              and torch.equal(u.consumed, wire.len) and not state.any())
    # the gathered bytes are the payloads (slots and payloads both start at multiples of 16)
    sample = range(0, n, max(1, n // 64))
    ok = ok and all(torch.equal(out[int(out_off[i]):int(out_off[i]) + int(cap[i])],
                                src.data[int(src.off[i]):int(src.off[i]) + int(cap[i])]) for i in sample)
    # yardstick: the mask pass over the same bytes where the frame pass left them
    mkeys = keys[:n].contiguous()
    payload = int(src.len.to(torch.int64).sum().item())
    wire_bytes = int(wire.len.to(torch.int64).sum().item())
    # the timed calls go to the C ABI with every buffer allocated beforehand,
    # so that the short kernels of shape (a) are not hidden behind the
    # wrapper's allocations
    L, P, S = pmd.lib(), pmd._ptr, pmd._stream_handle(None)
    code = torch.empty(n, dtype=torch.int16, device="cuda")
    ua = (pmd.ROLE_SERVER, 1, 16 << 20, P(wire.data), P(wire.off), P(wire.len), n, P(state), P(out), P(out_off),
          P(cap), P(u.out.len), P(u.op), P(u.compressed), P(u.event), P(u.status), P(u.consumed), P(u.ctl),
          P(u.ctl_len), P(code), S)
    ma = (P(out), P(out_off), P(cap), n, P(mkeys), None, S)

    def unframe_c():
        assert L.bpmd_unframe_batch(*ua) == 0

    def mask_c():
        assert L.bpmd_mask_batch(*ma) == 0

    tu = timed(unframe_c, args.warmup, args.repeats, inner)
    tm = timed(mask_c, args.warmup, args.repeats, inner)
    gib = lambda ms: payload / (ms * 1e-3) / 2**30  # noqa: E731
    print(json.dumps({"shape": args.shape, "what": what, "ok": ok, "entries": n, "frames": nk,
                      "payload_bytes": payload, "wire_bytes": wire_bytes,
                      "unframe_ms": {"median": tu[0], "min": tu[1], "max": tu[2]},
                      "mask_ms": {"median": tm[0], "min": tm[1], "max": tm[2]},
                      "unframe_GiBps": round(gib(tu[0]), 2), "mask_GiBps": round(gib(tm[0]), 2),
                      "unframe_over_mask": round(tm[0] / tu[0], 3),
                      "warmup": args.warmup, "repeats": args.repeats, "inner": inner,
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
