"""Time of the chained receive call for context-takeover connections
(bpmd_receive_takeover_batch) on one GPU, server role, against the chain it
replaces (pmd.unframe_batch, a host-side pick of the compressed entries,
pmd.TakeoverInflater.inflate, pmd.utf8_check_batch, a final synchronise) on
the same wire bytes in the same run:

    python scripts/bench_receive_takeover.py --shape a   64 Ki connections, 1 KiB JSON text messages (config C1's
                                                         message), level 6 with kept context, one masked frame each
    python scripts/bench_receive_takeover.py --shape b   4 Ki connections, 16 KiB JSON text messages
    ... --no-slide                                       the same calls with every position put back between the
                                                         timed units, so that no window ever slides

Every connection receives a cycle of `--cycle` messages deflated by one kept
CPython deflater (the first copies from nothing, the others from those before
them in the cycle), again and again, at window_bits 15.  A timed unit is one
whole cycle of back-to-back calls.  Connection buffers hold two windows, one
message and one more cycle; positions start staggered over the calls between
two slides of a connection, so in steady state every call slides its share of
the windows.  Both paths slide by the same rule at the same capacity.

bpmd_receive_takeover_batch (the C call, every buffer pre-allocated) is timed
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
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beast_amd import pmd, synth  # noqa: E402

WBITS = 15
W = 1 << WBITS
STREAMS = 4096   # distinct connection streams, dealt to the connections so that neighbours differ


def make_wires(n, size, cycle, dev):
    """wires[k]: message k of every connection's cycle, framed and masked; texts[k][s]: stream s's message"""
    raw, off, _ = synth.make_batch("json", np.full(STREAMS * cycle, size, dtype=np.uint32), seed=0xC1)
    texts = [[bytes(raw[int(off[k * STREAMS + s]):int(off[k * STREAMS + s]) + size]) for s in range(STREAMS)]
             for k in range(cycle)]
    pls = [[None] * STREAMS for _ in range(cycle)]
    for s in range(STREAMS):
        z = zlib.compressobj(6, zlib.DEFLATED, -WBITS, 8)
        for k in range(cycle):
            p = z.compress(texts[k][s]) + z.flush(zlib.Z_SYNC_FLUSH)
            pls[k][s] = np.frombuffer(p[:-4], np.uint8)
    deal = (np.arange(n, dtype=np.int64) * 2654435761) % STREAMS
    g = torch.Generator(device="cuda").manual_seed(7)
    wires, gathered = [], 0
    for k in range(cycle):
        lens = np.array([len(pls[k][s]) for s in deal], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]])
        data = np.concatenate([pls[k][s] for s in deal] + [np.zeros(16, np.uint8)])
        b = pmd.Batch.from_arrays(data, off, lens.astype(np.int32), device=dev)
        keys = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device=dev, generator=g)
        wires.append(pmd.frame_batch(b, 1 << 20, op=1, compressed=True, keys=keys))
        gathered = max(gathered, int(lens.max()))
    torch.cuda.synchronize()
    return wires, texts, deal, gathered


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
    what = f"{n} connections, JSON text messages of {size} B, level 6 with kept context (cycle of {cycle}), " \
        f"one masked frame each, window_bits {WBITS}" + (", positions reset: no slides" if args.no_slide else "")
    wires, texts, deal, out_cap = make_wires(n, size, cycle, dev)
    msg_max = 16 << 20

    # ---- both paths' connection buffers: two windows, one message, one more cycle
    old = pmd.TakeoverInflater(n, window_bits=WBITS, max_msg=size * (cycle + 1), device=dev)
    slot = old.slot
    period = (slot - W) // size                       # calls between two slides of a connection
    pos0 = W + (torch.arange(n, device=dev) % (1 if args.no_slide else period)) * size
    buf = torch.zeros_like(old.buf)
    pos = pos0.to(torch.int32)
    old.pos.copy_(pos0)
    st_new, st_old = pmd.rd_state(n, dev), pmd.rd_state(n, dev)
    stride = (out_cap + 15) // 16 * 16
    out_off = torch.arange(n, dtype=torch.int64, device=dev) * stride
    out_new = torch.zeros(n * stride + 16, dtype=torch.uint8, device=dev)
    out_old = torch.zeros_like(out_new)
    ocap = torch.full((n,), out_cap, dtype=torch.int32, device=dev)
    mcap = torch.full((n,), size, dtype=torch.int32, device=dev)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)  # noqa: E731
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    out_len, status, consumed, msg_len = i32(), i32(), i32(), i32()
    opc, comp, event, ctl_len, ctl = u8(n), u8(n), u8(n), u8(n), u8(n, pmd.CTL_SLOT)
    code = torch.zeros(n, dtype=torch.int16, device=dev)
    msg_off = torch.zeros(n, dtype=torch.int64, device=dev)
    L, P, S = pmd._recv_tk_lib(), pmd._ptr, pmd._stream_handle(None)
    work = u8(int(L.bpmd_receive_takeover_work_bytes(n)))
    cfg = pmd._Cfg(0, WBITS, 8, 0, 0)

    def recv_c(k):
        w = wires[k]
        assert L.bpmd_receive_takeover_batch(
            ctypes.byref(cfg), pmd.ROLE_SERVER, msg_max, P(w.data), P(w.off), P(w.len), n, P(st_new), P(out_new),
            P(out_off), P(ocap), P(out_len), P(opc), P(comp), P(event), P(status), P(consumed), P(ctl), P(ctl_len),
            P(code), P(buf), P(old.base), slot, P(pos), P(mcap), P(msg_off), P(msg_len), P(work), S) == 0

    def chain(k):
        u = pmd.unframe_batch(wires[k], out_cap, pmd.ROLE_SERVER, msg_max=msg_max, state=st_old, out=out_old,
                              out_off=out_off)
        st = u.status.clone()
        done = (u.event == pmd.EV_MESSAGE) & (u.status == 0)
        zi = torch.nonzero(done & (u.compressed != 0)).flatten()     # the host-side pick: waits for the frame pass
        res = None
        if zi.numel():
            res = old.inflate(pmd.Batch(u.out.data, u.out.off[zi].contiguous(), u.out.len[zi].contiguous()), size,
                              conn=zi)
            st[zi] = res.status
            ti = torch.nonzero((res.status == 0) & (u.op[zi] == 1)).flatten()
            if ti.numel():
                v = pmd.utf8_check_batch(pmd.Batch(old.buf, res.out.off[ti].contiguous(), res.out.len[ti].contiguous()))
                st[zi[ti]] = torch.where(v != 0, pmd.BAD_FRAME_PAYLOAD, 0).to(torch.int32)
        return u, st, res

    def reset():
        if args.no_slide:
            pos.copy_(pos0)
            old.pos.copy_(pos0)

    # ---- one cycle of both, checked: statuses, lengths, a sample of the messages, and each other
    ok, checks = True, {}
    sample = list(range(0, n, max(1, n // 64)))
    for k in range(cycle):
        recv_c(k)
        u, st, res = chain(k)
        torch.cuda.synchronize()
        checks = {"status": not status.any(), "event": bool((event == pmd.EV_MESSAGE).all()),
                  "same_status": torch.equal(status, st), "msg_len": bool((msg_len == size).all()),
                  "same_off": res is not None and torch.equal(msg_off, res.out.off),
                  "same_pos": torch.equal(pos.to(torch.int64), old.pos),
                  "messages": all(bytes(buf[int(msg_off[c]):int(msg_off[c]) + size].cpu().numpy()) == texts[k][deal[c]]
                                  for c in sample)}
        if not all(bool(v) for v in checks.values()):
            ok = False
            print("failed checks in call", k, [x for x, v in checks.items() if not v], file=sys.stderr)

    meds = {"takeover_batch_events": [], "takeover_batch_host": [], "chain_host": []}
    for _ in range(args.blocks):
        meds["takeover_batch_events"].append(units(recv_c, reset, args.warmup, args.repeats, cycle, True))
        meds["takeover_batch_host"].append(units(recv_c, reset, args.warmup, args.repeats, cycle, False))
        meds["chain_host"].append(units(chain, reset, args.warmup, args.repeats, cycle, False))
    torch.cuda.synchronize()
    ok = ok and not status.any() and bool((msg_len == size).all())   # the timed calls kept decoding
    mid = {k: float(np.median(v)) for k, v in meds.items()}
    wire_bytes = int(sum(int(w.len.to(torch.int64).sum().item()) for w in wires) / cycle)
    print(json.dumps({"shape": args.shape, "what": what, "ok": bool(ok), "connections": n, "slot_bytes": slot,
                      "calls_between_slides": period, "sliding_share_per_call": 0.0 if args.no_slide else round(1 / period, 4),
                      "wire_bytes_per_call": wire_bytes, "message_bytes_per_call": n * size, "warmup": args.warmup,
                      "repeats": args.repeats, "calls_per_unit": cycle, "medians_ms_per_call": meds,
                      "yardstick_spread": round(max(meds["chain_host"]) / min(meds["chain_host"]), 4),
                      "chain_over_takeover_batch_host": round(mid["chain_host"] / mid["takeover_batch_host"], 4),
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
