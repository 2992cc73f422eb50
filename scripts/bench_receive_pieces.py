"""Time of the chained receive call that hands messages over in pieces
(bpmd_receive_pieces_batch) on one GPU, server role, against
bpmd_receive_takeover_batch on the same whole-message wire bytes in the same
run (scripts/bench_receive_takeover.py's inputs and protocol):

    python scripts/bench_receive_pieces.py --shape a   64 Ki connections, 1 KiB JSON text messages, level 6 with
                                                       kept context, one masked frame each
    python scripts/bench_receive_pieces.py --shape b   4 Ki connections, 16 KiB JSON text messages
    ... --piece 1536                                   instead of a message per call, every connection's wire handed
                                                       over 1 536 bytes per call (Beast's default read buffer) into
                                                       slots of 1 540 bytes

A timed unit is one cycle of `--cycle` messages; with --piece a unit is the
same cycle in ceil(wire / piece) calls per message.  Both calls are timed
with HIP events and with a host clock around a unit and a final synchronise,
alternating `--blocks` times, each figure the median of `--repeats` units per
message.  The takeover call keeps positions reset between units (no slides):
this compares decoders, not window maintenance.  One JSON line per run, with
the device bytes each call holds per connection."""
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
import bench_receive_takeover as TK  # noqa: E402
from beast_amd import pmd  # noqa: E402

WBITS, W = TK.WBITS, TK.W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["a", "b"], required=True)
    ap.add_argument("--conns", type=int, default=0)
    ap.add_argument("--cycle", type=int, default=0)
    ap.add_argument("--piece", type=int, default=0, help="wire bytes per call of the piece-split run (0: none)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--blocks", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    n = args.conns or (65536 if args.shape == "a" else 4096)
    size = 1024 if args.shape == "a" else 16384
    cycle = args.cycle or (8 if args.shape == "a" else 4)
    wires, texts, deal, gathered = TK.make_wires(n, size, cycle, dev)
    msg_max = 16 << 20
    P, S = pmd._ptr, pmd._stream_handle(None)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)  # noqa: E731
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    cfg = pmd._Cfg(0, WBITS, 8, 0, 0)

    def outputs():
        return dict(out_len=i32(), status=i32(), consumed=i32(), msg_len=i32(), op=u8(n), comp=u8(n), event=u8(n),
                    ctl_len=u8(n), ctl=u8(n, pmd.CTL_SLOT), code=torch.zeros(n, dtype=torch.int16, device=dev))

    # ---- the takeover call: two windows and one message per connection, a gathered slot of the longest payload
    LT = pmd._recv_tk_lib()
    slot = (2 * W + size + 15) // 16 * 16
    t_buf = u8(n * slot + 16)
    t_base = torch.arange(n, dtype=torch.int64, device=dev) * slot
    t_pos, t_state = i32(), pmd.rd_state(n, dev)
    stride = (gathered + 15) // 16 * 16
    t_out, t_out_off = u8(n * stride + 16), torch.arange(n, dtype=torch.int64, device=dev) * stride
    t_ocap, t_mcap = torch.full((n,), gathered, dtype=torch.int32, device=dev), torch.full((n,), size, dtype=torch.int32, device=dev)
    t_msg_off, t_work, to = torch.zeros(n, dtype=torch.int64, device=dev), u8(int(LT.bpmd_receive_takeover_work_bytes(n))), outputs()

    def takeover(k):
        w = wires[k]
        assert LT.bpmd_receive_takeover_batch(
            ctypes.byref(cfg), pmd.ROLE_SERVER, msg_max, P(w.data), P(w.off), P(w.len), n, P(t_state), P(t_out),
            P(t_out_off), P(t_ocap), P(to["out_len"]), P(to["op"]), P(to["comp"]), P(to["event"]), P(to["status"]),
            P(to["consumed"]), P(to["ctl"]), P(to["ctl_len"]), P(to["code"]), P(t_buf), P(t_base), slot, P(t_pos),
            P(t_mcap), P(t_msg_off), P(to["msg_len"]), P(t_work), S) == 0

    # ---- the pieces call: the two states, a gathered slot and a message slot per connection
    LP = pmd._recv_pc_lib()
    zb = int(LP.bpmd_receive_pieces_zstate_bytes())
    p_state, p_z = pmd.rd_piece_state(n, dev), u8(n * zb)
    piece = args.piece
    ocap = (piece if piece else gathered) + 4
    pstride = (ocap + 15) // 16 * 16
    p_out, p_out_off = u8(n * pstride + 16), torch.arange(n, dtype=torch.int64, device=dev) * pstride
    p_msg, p_msg_off = u8(n * size + 16), torch.arange(n, dtype=torch.int64, device=dev) * size
    p_ocap, p_mcap = torch.full((n,), ocap, dtype=torch.int32, device=dev), torch.full((n,), size, dtype=torch.int32, device=dev)
    p_work, po = u8(int(LP.bpmd_receive_pieces_work_bytes(n))), outputs()

    def pieces_call(data, off, ln):
        assert LP.bpmd_receive_pieces_batch(
            ctypes.byref(cfg), pmd.ROLE_SERVER, 1, msg_max, P(data), P(off), P(ln), n, P(p_state), P(p_z), P(p_out),
            P(p_out_off), P(p_ocap), P(po["out_len"]), P(po["op"]), P(po["comp"]), P(po["event"]), P(po["status"]),
            P(po["consumed"]), P(po["ctl"]), P(po["ctl_len"]), P(po["code"]), P(p_msg), P(p_msg_off), P(p_mcap),
            P(po["msg_len"]), P(p_work), S) == 0

    def whole(k):
        w = wires[k]
        pieces_call(w.data, w.off, w.len)

    # the piece split: call j of message k hands over bytes [j * piece, (j + 1) * piece) of every connection's
    # frame; with a slot of piece + 4 every call takes all it is given, so the offsets are known beforehand
    split = []
    if piece:
        for w in wires:
            steps = (int(w.len.max().item()) + piece - 1) // piece
            l64 = w.len.to(torch.int64)
            split.append([(w.data, (w.off + j * piece).contiguous(),
                           torch.clamp(l64 - j * piece, 0, piece).to(torch.int32)) for j in range(steps)])

    def in_pieces(k):
        for data, off, ln in split[k]:
            pieces_call(data, off, ln)

    def reset_t():
        t_pos.zero_()

    def reset_p():   # a new connection: the timed cycle starts from nothing, as the first one did
        p_state.zero_()
        p_z.zero_()

    # ---- one cycle of each, checked against the messages and each other
    sample = list(range(0, n, max(1, n // 64)))
    ok = True
    reset_t(), reset_p()
    for k in range(cycle):
        takeover(k)
        torch.cuda.synchronize()
        good = not to["status"].any() and bool((to["event"] == pmd.EV_MESSAGE).all())
        if not piece:
            whole(k)
            torch.cuda.synchronize()
            good = (good and not po["status"].any() and bool((po["event"] == pmd.EV_MESSAGE).all()) and
                    bool((po["msg_len"] == size).all()) and torch.equal(po["consumed"], to["consumed"]) and
                    all(bytes(p_msg[c * size:(c + 1) * size].cpu().numpy()) == texts[k][deal[c]] for c in sample))
        if not good:
            ok = False
            print("failed checks in call", k, file=sys.stderr)
    if piece:
        # a message takes ceil(longest wire / piece) calls, a connection with a shorter wire fewer: each is judged
        # at its own last non-empty piece, where its message must end; an empty piece behind it takes and
        # delivers nothing and asks for more
        reset_p()
        for k in range(cycle):
            got = [b""] * len(sample)
            last = (wires[k].len.to(torch.int64) + piece - 1) // piece - 1
            for j, (data, off, ln) in enumerate(split[k]):
                pieces_call(data, off, ln)
                torch.cuda.synchronize()
                ends, empty = last == j, ln == 0
                checks = {"status": not po["status"].any(), "consumed": torch.equal(po["consumed"], ln),
                          "message at the last piece": bool((po["event"][ends] == pmd.EV_MESSAGE).all()),
                          "need_more elsewhere": bool((po["event"][~ends] == pmd.EV_NEED_MORE).all()),
                          "nothing from an empty piece": not po["msg_len"][empty].any() and not po["out_len"][empty].any()}
                for name, good in checks.items():
                    if not good:
                        ok = False
                        print("failed check in message", k, "piece", j, ":", name, file=sys.stderr)
                ml = po["msg_len"].cpu().tolist()
                for a, c in enumerate(sample):
                    got[a] += bytes(p_msg[c * size:c * size + ml[c]].cpu().numpy())
            if not all(got[a] == texts[k][deal[c]] for a, c in enumerate(sample)):
                ok = False
                print("failed check in message", k, ": reassembled bytes", file=sys.stderr)

    new = "split" if piece else "pieces"     # with --piece the slot is piece + 4 bytes: no whole message fits a call
    meds = {k: [] for k in ("takeover_events", "takeover_host", new + "_events", new + "_host")}
    for _ in range(args.blocks):
        for name, fn, rs in [("takeover", takeover, reset_t), (new, in_pieces if piece else whole, reset_p)]:
            meds[name + "_events"].append(TK.units(fn, rs, args.warmup, args.repeats, cycle, True))
            meds[name + "_host"].append(TK.units(fn, rs, args.warmup, args.repeats, cycle, False))
    torch.cuda.synchronize()
    ok = ok and not to["status"].any() and not po["status"].any()
    mid = {k: float(np.median(v)) for k, v in meds.items()}
    wire_bytes = int(sum(int(w.len.to(torch.int64).sum().item()) for w in wires) / cycle)
    res = {"shape": args.shape, "ok": bool(ok), "connections": n, "message_bytes": size, "cycle": cycle,
           "wire_bytes_per_message_call": wire_bytes, "warmup": args.warmup, "repeats": args.repeats,
           "medians_ms_per_message": meds,
           "yardstick_spread": round(max(meds["takeover_events"]) / min(meds["takeover_events"]), 4),
           new + "_over_takeover_events": round(mid[new + "_events"] / mid["takeover_events"], 3),
           new + "_over_takeover_host": round(mid[new + "_host"] / mid["takeover_host"], 3),
           new + "_GiB_per_s_inflated": round(n * size / mid[new + "_events"] * 1e3 / 2**30, 3),
           "takeover_GiB_per_s_inflated": round(n * size / mid["takeover_events"] * 1e3 / 2**30, 3),
           "device_bytes_per_connection": {
               "pieces": {"zstate": zb, "state": 32, "out_slot": pstride, "msg_slot": size,
                          "total": zb + 32 + pstride + size},
               "takeover": {"buffer_2W_plus_message": slot, "gathered_slot": stride, "state": 16,
                            "total": slot + stride + 16}},
           "device": torch.cuda.get_device_name(0)}
    if piece:
        res.update({"piece": piece, "calls_per_message": [len(s) for s in split]})
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
