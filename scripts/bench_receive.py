"""Time of the batch receive side in one chained call (bpmd_receive_batch) on
one GPU, server role, against the chain it replaces (pmd.receive_batch:
unframe, pick the entries on the host, read_batch, utf8_check_batch) on the
same wire bytes in the same run:

    python scripts/bench_receive.py --shape a   64 Ki JSON text messages of 4 KiB (bench.py C2's messages),
                                                compressed, one masked frame each
    python scripts/bench_receive.py --shape b   16 Ki messages of 64 KiB random bytes, compressed, masked 4 KiB frames
    python scripts/bench_receive.py --shape c   shape a's messages sent uncompressed: nothing is inflated, which
                                                shows what the inflate launch over all n entries costs with nothing to do

bpmd_receive_batch is timed with HIP events around `--inner` back-to-back
calls and with a host clock around one call and a final synchronise;
pmd.receive_batch waits inside, so it is timed with the host clock only.  The
two alternate `--blocks` times in one run, each figure the median of
`--repeats` rounds after `--warmup` untimed ones; the yardstick's own spread is
max/min of its repeated medians.  One JSON line per run."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from beast_amd import pmd, synth  # noqa: E402
from scripts.bench_send import shape_b, timed, timed_host  # noqa: E402


def shape_json(n):
    lens = np.full(n, bench.MSG_BYTES, dtype=np.uint32)
    raw, off, ln = synth.make_batch("json", lens, seed=bench.SEED_C2)
    return pmd.Batch.from_arrays(raw, off, ln)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["a", "b", "c"], required=True)
    ap.add_argument("--msgs", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=0)
    ap.add_argument("--blocks", type=int, default=3, help="alternations of the two paths")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if args.shape == "b":
        src, frame_max, what = shape_b(args.msgs or 16384)
        op, compress = 2, True
    else:
        src = shape_json(args.msgs or 65536)
        frame_max, op, compress = 1 << 20, 1, args.shape == "a"
        what = f"{src.n} JSON text messages of {bench.MSG_BYTES} B, " + \
            ("compressed, one masked frame each" if compress else "uncompressed, one masked frame each")
    inner = args.inner or (2 if args.shape == "b" else 20)
    n, dev = src.n, src.data.device

    # ---- the wire: the send side's output, client role
    fb, _ = pmd.send_bounds(src.len, frame_max, True, compress, False)
    g = torch.Generator(device="cuda").manual_seed(7)
    keys = torch.randint(-2**31, 2**31 - 1, (int(fb.sum().item()),), dtype=torch.int32, device=dev, generator=g)
    sent = pmd.send_batch(src, pmd.ROLE_CLIENT, pmd_on=compress, frag=False, frame_max=frame_max, op=op, keys=keys)
    torch.cuda.synchronize()
    assert not sent.status.any()
    wire = sent.wire
    gathered_len = sent.deflated.out.len if compress else src.len
    del sent

    # ---- buffers of both paths: gathered slots as the payloads need, message slots as the messages do
    out_cap = gathered_len.clone()
    out_off = pmd.slot_offsets(out_cap)
    out = torch.zeros(int(out_off[-1].item() + out_cap[-1].item()) + 16, dtype=torch.uint8, device=dev)
    msg_cap, msg_off = src.len, src.off
    msg = torch.zeros_like(src.data)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)  # noqa: E731
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    out_len, status, consumed, msg_len = i32(), i32(), i32(), i32()
    opc, comp, event, ctl_len, ctl = u8(n), u8(n), u8(n), u8(n), u8(n, pmd.CTL_SLOT)
    code = torch.zeros(n, dtype=torch.int16, device=dev)
    L, P, S = pmd._recv_lib(), pmd._ptr, pmd._stream_handle(None)
    work = u8(int(L.bpmd_receive_work_bytes(n)))
    cfg = pmd._Cfg(0, 15, 8, 0, 0)
    msg_max = 16 << 20
    pmd.inflate_reserve(int(gathered_len.sum().item()), int(src.len.sum().item()), n)

    def recv_c():
        assert L.bpmd_receive_batch(ctypes.byref(cfg), pmd.ROLE_SERVER, 1, msg_max, P(wire.data), P(wire.off),
                                    P(wire.len), n, None, P(out), P(out_off), P(out_cap), P(out_len), P(opc), P(comp),
                                    P(event), P(status), P(consumed), P(ctl), P(ctl_len), P(code), P(msg), P(msg_off),
                                    P(msg_cap), P(msg_len), P(work), S) == 0

    def parent():
        return pmd.receive_batch(wire, out_cap, msg_cap, pmd.ROLE_SERVER, msg_max=msg_max, out=out, out_off=out_off)

    recv_c()
    ref = parent()
    torch.cuda.synchronize()
    total = int(src.off[-1].item() + src.len[-1].item())
    checks = {"status": not status.any(), "event": bool((event == pmd.EV_MESSAGE).all()),
              "same_status": torch.equal(status, ref.status), "same_event": torch.equal(event, ref.event),
              "msg_len": torch.equal(msg_len, src.len), "compressed": bool((comp != 0).all()) == compress}
    if compress:
        checks["messages"] = torch.equal(msg[:total], src.data[:total])
        checks["chain_messages"] = ref.inflated is not None and torch.equal(ref.inflated.out.len, src.len)
    else:   # the messages stay in their gathered slots
        j = torch.arange(int(src.len[-1].item()), device=dev)
        checks["messages"] = torch.equal(out[out_off[-1] + j], src.data[src.off[-1] + j])
        checks["chain_messages"] = ref.inflated is None
    ok = all(bool(v) for v in checks.values())
    if not ok:
        print("failed checks:", [k for k, v in checks.items() if not v], file=sys.stderr)

    meds = {"receive_batch_events": [], "receive_batch_host": [], "chain_host": []}
    for _ in range(args.blocks):
        meds["receive_batch_events"].append(timed(recv_c, args.warmup, args.repeats, inner))
        meds["receive_batch_host"].append(timed_host(recv_c, args.warmup, args.repeats))
        meds["chain_host"].append(timed_host(parent, args.warmup, args.repeats))
    torch.cuda.synchronize()
    mid = {k: float(np.median(v)) for k, v in meds.items()}
    wire_bytes = int(wire.len.to(torch.int64).sum().item())
    print(json.dumps({"shape": args.shape, "what": what, "ok": ok, "messages": n, "wire_bytes": wire_bytes,
                      "message_bytes": int(src.len.to(torch.int64).sum().item()), "warmup": args.warmup,
                      "repeats": args.repeats, "inner": inner, "medians_ms": meds,
                      "yardstick_spread": round(max(meds["chain_host"]) / min(meds["chain_host"]), 4),
                      "chain_over_receive_batch_host": round(mid["chain_host"] / mid["receive_batch_host"], 4),
                      "receive_batch_wire_GiBps_events": round(wire_bytes / (mid["receive_batch_events"] * 1e-3) / 2**30,
                                                               2),
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
