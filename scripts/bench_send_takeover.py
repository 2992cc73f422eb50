"""Time of the chained send call for context-takeover connections
(bpmd_send_takeover_batch) on one GPU, server role, against the host chain it
replaces (pmd.TakeoverDeflater.deflate, then pmd.frame_batch, a final
synchronise) on the same messages in the same run:

    python scripts/bench_send_takeover.py --shape a   64 Ki connections, 1 KiB JSON text messages (config C1's
                                                      message), level 6, window_bits 15
    python scripts/bench_send_takeover.py --shape b   4 Ki connections, 16 KiB JSON text messages
    ... --no-slide                                    the same calls with every position put back between the
                                                      timed units, so that no buffer ever slides

Every connection sends a cycle of `--cycle` messages again and again, all of
them compressed.  A timed unit is one whole cycle of back-to-back calls.
Connection buffers hold two times 4 KiB, one message and one more cycle;
positions start staggered over the calls between two slides of a connection,
so in steady state every call slides its share of the buffers.  Both paths
slide by the same rule at the same capacity and frame at 4 KiB.

bpmd_send_takeover_batch (the C call, every buffer pre-allocated) is timed
with HIP events around a unit and with a host clock around a unit and a final
synchronise; the chain waits inside, so it is timed with the host clock only.
The paths alternate `--blocks` times in one run, each figure the median of
`--repeats` units after `--warmup` untimed ones, per call; the yardstick's own
spread is max/min of its repeated medians.  One JSON line per run."""
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
from beast_amd import pmd, synth  # noqa: E402

WBITS, LEVEL, FRAME_MAX = 15, 6, 4096
K = pmd.TakeoverDeflater.HIST
STREAMS = 4096   # distinct connection streams, dealt to the connections so that neighbours differ


def make_batches(n, size, cycle, dev):
    """batches[k]: message k of every connection's cycle"""
    raw, off, _ = synth.make_batch("json", np.full(STREAMS * cycle, size, dtype=np.uint32), seed=0xC1)
    deal = (np.arange(n, dtype=np.int64) * 2654435761) % STREAMS
    out = []
    for k in range(cycle):
        texts = np.stack([raw[int(off[k * STREAMS + s]):int(off[k * STREAMS + s]) + size] for s in range(STREAMS)])
        data = np.concatenate([texts[deal].reshape(-1), np.zeros(16, np.uint8)])
        out.append(pmd.Batch.from_arrays(data, np.arange(n, dtype=np.int64) * size, np.full(n, size, np.int32),
                                         device=dev))
    torch.cuda.synchronize()
    return out


def units(fn, reset, warmup, repeats, cycle, events):
    """median time per call of `repeats` units of `cycle` calls; reset() runs untimed before each"""
    for _ in range(warmup):
        reset()
        for k in range(cycle):
            fn(k)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        reset()
        torch.cuda.synchronize()
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(cycle):
                fn(k)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / cycle)
        else:
            t0 = time.perf_counter()
            for k in range(cycle):
                fn(k)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / cycle)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["a", "b"], required=True)
    ap.add_argument("--conns", type=int, default=0)
    ap.add_argument("--cycle", type=int, default=0)
    ap.add_argument("--no-slide", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--blocks", type=int, default=3, help="alternations of the two paths")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    n = args.conns or (65536 if args.shape == "a" else 4096)
    size = 1024 if args.shape == "a" else 16384
    cycle = args.cycle or (8 if args.shape == "a" else 4)
    what = f"{n} connections, JSON text messages of {size} B, all compressed at level {LEVEL} with kept context " \
        f"(cycle of {cycle}), frames of {FRAME_MAX} B, server role, window_bits {WBITS}" + \
        (", positions reset: no slides" if args.no_slide else "")
    batches = make_batches(n, size, cycle, dev)

    # ---- both paths' connection buffers: two times K, one message, one more cycle
    old = pmd.TakeoverDeflater(n, level=LEVEL, window_bits=WBITS, max_msg=size * (cycle + 1), device=dev)
    slot = old.slot
    period = (slot - K) // size                       # calls between two slides of a connection
    pos0 = K + (torch.arange(n, device=dev) % (1 if args.no_slide else period)) * size
    buf = torch.zeros_like(old.buf)
    pos = pos0.to(torch.int32)
    old.pos.copy_(pos0)
    L, P, S = pmd._send_tk_lib(), pmd._ptr, pmd._stream_handle(None)
    zc = (pmd.upper_bound(size) + 15) // 16 * 16
    z = torch.zeros(n * zc + 16, dtype=torch.uint8, device=dev)
    z_off = torch.arange(n, dtype=torch.int64, device=dev) * zc
    z_cap = torch.full((n,), zc, dtype=torch.int32, device=dev)
    wire_cap = n * int(L.bpmd_send_wire_bound(size, FRAME_MAX, 0, 1, 1))
    wire = torch.zeros(wire_cap + 16, dtype=torch.uint8, device=dev)
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    z_len, w_len, status = i32(), i32(), i32()
    w_off = torch.zeros(n, dtype=torch.int64, device=dev)
    comp = torch.zeros(n, dtype=torch.uint8, device=dev)
    op = torch.ones(n, dtype=torch.uint8, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    work = torch.zeros(int(L.bpmd_send_takeover_work_bytes(n)), dtype=torch.uint8, device=dev)
    cfg = pmd._Cfg(LEVEL, WBITS, 4, 0, 0)

    def send_c(k):
        b = batches[k]
        assert L.bpmd_send_takeover_batch(
            ctypes.byref(cfg), P(b.data), P(b.off), P(b.len), n, pmd.ROLE_SERVER, 0, 1, FRAME_MAX, size, P(op), None,
            P(buf), P(old.base), slot, P(pos), P(z), P(z_off), P(z_cap), P(z_len), None, None, P(wire), wire_cap,
            P(w_off), P(w_len), P(comp), P(status), P(total), P(work), S) == 0

    def chain(k):
        d = old.deflate(batches[k])
        return d, pmd.frame_batch(d.out, FRAME_MAX, op=1, compressed=True)

    def reset():
        if args.no_slide:
            pos.copy_(pos0)
            old.pos.copy_(pos0)

    # ---- one cycle of both, checked: statuses, positions, and every wire byte against the other path
    ok = True
    for k in range(cycle):
        send_c(k)
        d, w = chain(k)
        torch.cuda.synchronize()
        tot = int(total.item())
        checks = {"status": not status.any() and not d.status.any(), "compressed": bool(comp.all()),
                  "same_pos": torch.equal(pos.to(torch.int64), old.pos), "same_buf": torch.equal(buf, old.buf),
                  "same_len": torch.equal(w_len, w.len.to(torch.int32)), "same_off": torch.equal(w_off, w.off),
                  "same_wire": torch.equal(wire[:tot], w.data[:tot])}
        if not all(bool(v) for v in checks.values()):
            ok = False
            print("failed checks in call", k, [x for x, v in checks.items() if not v], file=sys.stderr)

    meds = {"takeover_batch_events": [], "takeover_batch_host": [], "chain_host": []}
    for _ in range(args.blocks):
        meds["takeover_batch_events"].append(units(send_c, reset, args.warmup, args.repeats, cycle, True))
        meds["takeover_batch_host"].append(units(send_c, reset, args.warmup, args.repeats, cycle, False))
        meds["chain_host"].append(units(chain, reset, args.warmup, args.repeats, cycle, False))
    torch.cuda.synchronize()
    ok = ok and not status.any() and bool((w_len != 0).all())   # the timed calls kept sending
    mid = {k: float(np.median(v)) for k, v in meds.items()}
    print(json.dumps({"shape": args.shape, "what": what, "ok": bool(ok), "connections": n, "slot_bytes": slot,
                      "calls_between_slides": period, "sliding_share_per_call": 0.0 if args.no_slide else round(1 / period, 4),
                      "wire_bytes_per_call": int(total.item()), "message_bytes_per_call": n * size, "warmup": args.warmup,
                      "repeats": args.repeats, "calls_per_unit": cycle, "medians_ms_per_call": meds,
                      "yardstick_spread": round(max(meds["chain_host"]) / min(meds["chain_host"]), 4),
                      "chain_over_takeover_batch_host": round(mid["chain_host"] / mid["takeover_batch_host"], 4),
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
