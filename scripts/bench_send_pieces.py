"""Time of the chained send call for messages in pieces (bpmd_send_pieces_batch)
on one GPU, server role, in one run against

  * the host chain it replaces, per piece: pmd.TakeoverDeflater.deflate, the
    marker 00 00 FF FF appended behind a non-final piece's payload (an index
    scatter), pmd.frame_batch, a final synchronise;
  * bpmd_send_takeover_batch on the same inputs with every piece final, so that
    the state and marker steps get a price of their own.

    python scripts/bench_send_pieces.py --shape a   64 Ki connections, pieces of 1 KiB of JSON text, level 6,
                                                    window_bits 15
    python scripts/bench_send_pieces.py --shape b   4 Ki connections, pieces of 16 KiB

Every connection sends messages of four pieces again and again (fin on every
fourth call), all compressed.  A timed unit is one message: four back-to-back
calls.  Buffers, slides, staggered start positions and the timing protocol are
scripts/bench_send_takeover.py's: HIP events around a unit and a host clock
around a unit and a final synchronise for the C calls (every buffer
pre-allocated), the host clock for the chain, which waits inside; the paths
alternate `--blocks` times, each figure the median of `--repeats` units after
`--warmup` untimed ones, per call.  One JSON line per run."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from beast_amd import pmd  # noqa: E402
from bench_send_takeover import make_batches, units  # noqa: E402

WBITS, LEVEL, FRAME_MAX, PIECES = 15, 6, 4096, 4
K = pmd.TakeoverDeflater.HIST


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["a", "b"], required=True)
    ap.add_argument("--conns", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--blocks", type=int, default=3, help="alternations of the paths")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    n = args.conns or (65536 if args.shape == "a" else 4096)
    size = 1024 if args.shape == "a" else 16384
    what = f"{n} connections, messages of {PIECES} pieces of {size} B of JSON text, all compressed at level {LEVEL} " \
        f"with kept context, frames of {FRAME_MAX} B, server role, window_bits {WBITS}"
    batches = make_batches(n, size, PIECES, dev)

    old = pmd.TakeoverDeflater(n, level=LEVEL, window_bits=WBITS, max_msg=size * (PIECES + 1), device=dev)
    slot = old.slot
    period = (slot - K) // size                       # calls between two slides of a connection
    pos0 = K + (torch.arange(n, device=dev) % period) * size
    old.pos.copy_(pos0)
    L, P, S = pmd._send_pc_lib(), pmd._ptr, pmd._stream_handle(None)
    zc = (pmd.upper_bound(size) + 4 + 15) // 16 * 16
    z_off = torch.arange(n, dtype=torch.int64, device=dev) * zc
    z_cap = torch.full((n,), zc, dtype=torch.int32, device=dev)
    wire_cap = n * int(L.bpmd_send_piece_wire_bound(size, FRAME_MAX, 0, 1, 1, 0))
    op = torch.ones(n, dtype=torch.uint8, device=dev)
    fins = [torch.full((n,), int(k == PIECES - 1), dtype=torch.uint8, device=dev) for k in range(PIECES)]
    cfg = pmd._Cfg(LEVEL, WBITS, 4, 0, 0)
    work = torch.zeros(int(L.bpmd_send_pieces_work_bytes(n)), dtype=torch.uint8, device=dev)

    class Side:   # one C path's connections and outputs
        def __init__(self):
            self.buf = torch.zeros_like(old.buf)
            self.pos = pos0.to(torch.int32)
            self.state = pmd.wr_state(n, dev)
            self.z = torch.zeros(n * zc + 16, dtype=torch.uint8, device=dev)
            self.wire = torch.zeros(wire_cap + 16, dtype=torch.uint8, device=dev)
            i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
            self.z_len, self.w_len, self.status = i32(), i32(), i32()
            self.w_off = torch.zeros(n, dtype=torch.int64, device=dev)
            self.comp = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.total = torch.zeros(1, dtype=torch.int64, device=dev)

    pc, pf, tk = Side(), Side(), Side()    # pieces; pieces, every one final; the takeover call

    def pieces_call(s, k, fin):
        b = batches[k]
        assert L.bpmd_send_pieces_batch(
            ctypes.byref(cfg), P(b.data), P(b.off), P(b.len), n, pmd.ROLE_SERVER, 0, 1, FRAME_MAX, size, P(op), None,
            fin, None, P(s.state), P(s.buf), P(old.base), slot, P(s.pos), P(s.z), P(z_off), P(z_cap), P(s.z_len), None,
            None, P(s.wire), wire_cap, P(s.w_off), P(s.w_len), P(s.comp), P(s.status), P(s.total), P(work), S) == 0

    def send_pieces(k):
        pieces_call(pc, k, P(fins[k]))

    def send_final(k):
        pieces_call(pf, k, None)

    def send_takeover(k):
        b, s = batches[k], tk
        assert L.bpmd_send_takeover_batch(
            ctypes.byref(cfg), P(b.data), P(b.off), P(b.len), n, pmd.ROLE_SERVER, 0, 1, FRAME_MAX, size, P(op), None,
            P(s.buf), P(old.base), slot, P(s.pos), P(s.z), P(z_off), P(z_cap), P(s.z_len), None, None, P(s.wire),
            wire_cap, P(s.w_off), P(s.w_len), P(s.comp), P(s.status), P(s.total), P(work), S) == 0

    marker = torch.tensor([0, 0, 0xFF, 0xFF], dtype=torch.uint8, device=dev)
    four = torch.arange(4, device=dev)

    def chain(k):
        d = old.deflate(batches[k])
        out = d.out
        if k != PIECES - 1:    # the marker behind every payload; deflate's slots are upper_bound(len) bytes
            at = (out.off + out.len.to(torch.int64))[:, None] + four[None, :]
            out.data[at.reshape(-1)] = marker.repeat(n)
            out = pmd.Batch(out.data, out.off, out.len + 4)
        return d, out, pmd.frame_batch(out, FRAME_MAX, op=1, compressed=True)

    # ---- one message of every path, checked: statuses, positions, payloads, and every wire byte against
    # the chain's but the first byte of a frame, where frame_batch writes a whole message's flags
    ok = True
    for k in range(PIECES):
        send_pieces(k), send_final(k), send_takeover(k)
        d, out, w = chain(k)
        torch.cuda.synchronize()
        tot = int(pc.total.item())
        frames = torch.clamp((out.len.to(torch.int64) + FRAME_MAX - 1) // FRAME_MAX, min=1)
        starts = torch.cat([pc.w_off + f * (FRAME_MAX + 4) for f in range(int(frames.max().item()))
                            ])[torch.cat([frames > f for f in range(int(frames.max().item()))])]
        same = pc.wire[:tot] == w.data[:tot]
        same[starts] = True
        b0 = pc.wire[pc.w_off]
        want_b0 = (0x41 if k == 0 else 0x00) | (0x80 if k == PIECES - 1 else 0)
        one = frames == 1
        checks = {"status": not pc.status.any() and not pf.status.any() and not tk.status.any() and not d.status.any(),
                  "compressed": bool(pc.comp.all()),
                  "same_pos": torch.equal(pc.pos.to(torch.int64), old.pos) and torch.equal(pf.pos, tk.pos),
                  "same_buf": torch.equal(pc.buf, old.buf) and torch.equal(pf.buf, tk.buf),
                  "same_len": torch.equal(pc.w_len, w.len.to(torch.int32)) and torch.equal(pc.z_len, out.len),
                  "same_off": torch.equal(pc.w_off, w.off), "same_wire_but_flags": bool(same.all()),
                  "flags": bool(((b0 & 0x7F) == (want_b0 & 0x7F)).all()) and
                  bool(((b0[one] & 0x80) == (want_b0 & 0x80)).all()),
                  "final_equals_takeover": torch.equal(pf.wire, tk.wire) and torch.equal(pf.w_len, tk.w_len)}
        if not all(bool(v) for v in checks.values()):
            ok = False
            print("failed checks in call", k, [x for x, v in checks.items() if not v], file=sys.stderr)
    ok = ok and int(pc.state[:, 0].sum()) == 0

    names = {"pieces_events": (send_pieces, True), "pieces_host": (send_pieces, False),
             "chain_host": (chain, False), "pieces_all_final_events": (send_final, True),
             "takeover_batch_events": (send_takeover, True), "pieces_all_final_host": (send_final, False),
             "takeover_batch_host": (send_takeover, False)}
    meds = {k: [] for k in names}
    for _ in range(args.blocks):
        for name, (fn, ev) in names.items():
            meds[name].append(units(fn, lambda: None, args.warmup, args.repeats, PIECES, ev))
    torch.cuda.synchronize()
    ok = ok and not pc.status.any() and bool((pc.w_len != 0).all()) and not pf.status.any() and not tk.status.any()
    mid = {k: float(np.median(v)) for k, v in meds.items()}
    print(json.dumps({"shape": args.shape, "what": what, "ok": bool(ok), "connections": n, "slot_bytes": slot,
                      "calls_between_slides": period, "wire_bytes_last_call": int(pc.total.item()),
                      "piece_bytes_per_call": n * size, "warmup": args.warmup, "repeats": args.repeats,
                      "calls_per_unit": PIECES, "medians_ms_per_call": meds,
                      "yardstick_spread": round(max(meds["chain_host"]) / min(meds["chain_host"]), 4),
                      "chain_over_pieces_host": round(mid["chain_host"] / mid["pieces_host"], 4),
                      "pieces_all_final_over_takeover_events":
                          round(mid["pieces_all_final_events"] / mid["takeover_batch_events"], 4),
                      "takeover_spread": round(max(meds["takeover_batch_events"]) / min(meds["takeover_batch_events"]), 4),
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
