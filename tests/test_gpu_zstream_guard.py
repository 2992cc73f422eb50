"""GPU: the per-stream inflate kernels inside their rooms.

The host side copies back only a call's out_used bytes, so a store past
out + cap never shows through the C ABI: in the arena (pmd_stream.hip
inflate_batch, regions packed at 256-byte granularity) it lands in padding
or, in a batch of several, in another connection's output.  The
kernel also reads its input 16 bytes at a time, up to 15 bytes past
in + n_in; in the arena those bytes are left over from earlier batches.

Here zstream_write_batch_kernel and zstream_write_kernel are launched
directly (bpmd_internal_zstream_write_batch / bpmd_internal_zstream_write) on
torch device memory laid out by the test: every input followed by 64 bytes of
poison, every output room of exactly `cap` bytes followed by 256 guard bytes.
32 streams (the plans of the lockstep tests, tests/zstream_cases.py
mixed_plans, with rooms that include 0, 1, 255, 256, 257, 258, 512 and 65536)
advance call by call exactly as bpmd_inflate_stream_write advances them.  For
a poison of 0x00 and of 0xFF: every call's status, in_used, out_used,
data_type, published and output bytes equal the oracle's, out_used <= cap,
and no guard byte (nor any input or poison byte) changes.

The fresh State image comes from the kernel source's host build
(tests/model/zstream_host.py: same zstream.h), so no struct offset is
restated here.  CPU mirror: tests/test_zstream_host.py."""
import ctypes
import struct

import numpy as np
import pytest

from oracle import oracle as O
from tests import zstream_cases as Z

pytestmark = pytest.mark.gpu

K, R = 32, 40
ROOMS = [0, 1, 255, 256, 257, 258, 512, 65536, 4096, 300, 7]
GUARD, SLACK, CANARY = 256, 64, 0xA5
UNSET = 12345   # drive()'s data_type before the call: still there when done() did not run


def up(x, a):
    return (x + a - 1) & ~(a - 1)


def _lib():
    from beast_amd import pmd
    L = pmd.lib()
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.bpmd_internal_zstream_write_batch.argtypes = [vp, ctypes.c_uint32, vp]
    L.bpmd_internal_zstream_write.argtypes = [vp, vp, u64, vp, u64, ctypes.c_int, vp, vp]
    assert L.bpmd_init() == 0
    return L


def _plans():
    named = Z.mixed_plans(R, 0, ROOMS) + Z.mixed_plans(R, 1, ROOMS)
    assert len(named) == K
    plans = [p for _, p in named]
    want = [Z.oracle_records(p) for p in plans]
    rooms = {c[1] for p in plans for c in p[2]}
    assert rooms >= {0, 1, 255, 256, 257, 258, 512, 65536}, sorted(rooms)
    return named, plans, want


def _fresh_states(plans):
    """[K, stride] uint8: each stream's State after reset(windowBits)."""
    from tests.model import zstream_host as H
    HL = H.lib()
    nbytes = HL.zs_host_state_bytes()
    stride = up(nbytes + 64, 256)
    img = np.zeros((len(plans), stride), dtype=np.uint8)
    for i, (_, wbits, _) in enumerate(plans):
        buf = ctypes.create_string_buffer(nbytes)
        HL.zs_host_reset(buf, wbits)
        img[i, :nbytes] = np.frombuffer(buf.raw, dtype=np.uint8)
    return img


def _run(poison, batched):
    import torch
    L = _lib()
    named, plans, want = _plans()
    dev = torch.device("cuda")
    states = torch.from_numpy(_fresh_states(plans)).to(dev)
    arena = torch.empty(16 << 20, dtype=torch.uint8, device=dev)
    sbase, stride, base = states.data_ptr(), states.shape[1], arena.data_ptr()
    assert sbase % 256 == 0 and base % 256 == 0
    hs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pos = [0] * K
    seen_caps = set()
    for r in range(R):
        # this round's calls, as bpmd_inflate_stream_write makes them
        cs = []
        for i, (stream, _, calls) in enumerate(plans):
            cut, room, flush = calls[r]
            cut = max(cut, pos[i])
            n = cut - pos[i]
            cs.append((stream[pos[i]:cut], min(room, 1040 * n + 8192), flush))
        # [ZCall K][Result K][input, poison]...[room, guard]...
        res_at = up(64 * K, 256)
        o = up(res_at + 64 * K, 256)
        in_at, out_at = [], []
        for data, _, _ in cs:
            in_at.append(o)
            o = up(o + len(data) + SLACK, 16)
        o = up(o, 256)
        ins_end = o
        for _, cap, _ in cs:
            out_at.append(o)
            o += cap + GUARD
        total = o
        assert total <= arena.numel()
        img = np.full(total, CANARY, dtype=np.uint8)
        for i, (data, cap, flush) in enumerate(cs):
            img[in_at[i]:in_at[i] + len(data)] = np.frombuffer(data, dtype=np.uint8)
            img[in_at[i] + len(data):in_at[i] + len(data) + SLACK] = poison
            img[64 * i:64 * i + 64] = np.frombuffer(
                struct.pack("<QQQQQQi12x", sbase + stride * i, base + in_at[i], len(data), base + out_at[i], cap,
                            base + res_at + 64 * i, flush), dtype=np.uint8)
            assert in_at[i] % 16 == 0 and in_at[i] + len(data) + SLACK <= ins_end and out_at[i] + cap + GUARD <= total
        arena[:total].copy_(torch.from_numpy(img))
        if batched:
            assert L.bpmd_internal_zstream_write_batch(base, K, hs) == 0
        else:
            for i, (data, cap, flush) in enumerate(cs):
                assert L.bpmd_internal_zstream_write(sbase + stride * i, base + in_at[i], len(data), base + out_at[i],
                                                     cap, flush, base + res_at + 64 * i, hs) == 0
        torch.cuda.synchronize()
        back = arena[:total].cpu().numpy()
        # nothing but results and rooms was written
        assert np.array_equal(back[:res_at], img[:res_at]) and np.array_equal(back[res_at + 64 * K:ins_end],
                                                                              img[res_at + 64 * K:ins_end]), r
        for i, (data, cap, flush) in enumerate(cs):
            in_used, out_used, ec, data_type, published, _ = struct.unpack_from("<QQiiii", back, res_at + 64 * i)
            w = want[i][r]
            tag = (named[i][0], "stream", i, "round", r, "n", len(data), "cap", cap, "flush", flush)
            guard = back[out_at[i] + cap:out_at[i] + cap + GUARD]
            assert (guard == CANARY).all(), (tag, "guard bytes changed at", np.nonzero(guard != CANARY)[0][:8])
            assert published in (0, 1) and out_used <= cap and in_used <= len(data), (tag, in_used, out_used)
            assert ec == w[0], (tag, O.ERRORS.get(ec, ec), O.ERRORS[w[0]])
            assert published == (w[5] != UNSET), (tag, published)
            if published:
                assert (in_used, out_used, data_type) == (w[1], w[3], w[5]), (tag, in_used, out_used, data_type, w[1:6])
                pos[i] += in_used
            else:
                assert w[1] == 0 and w[3] == 0
            assert back[out_at[i]:out_at[i] + out_used].tobytes() == w[8][:out_used], (tag, "bytes")
            seen_caps.add(cap)
    assert seen_caps >= {0, 1, 255, 256, 257, 258, 512, 65536}, sorted(seen_caps)


@pytest.mark.parametrize("poison", [0x00, 0xFF])
def test_batch_kernel_stays_inside_its_rooms(poison):
    """zstream_write_batch_kernel, 32 workgroups per launch, 40 launches."""
    _run(poison, batched=True)


@pytest.mark.parametrize("poison", [0x00, 0xFF])
def test_single_call_kernel_stays_inside_its_rooms(poison):
    """zstream_write_kernel, one launch per call, the same plans and guards."""
    _run(poison, batched=False)


def test_plans_reach_bad_and_done_mode():
    """(the oracle's side: calls made to failed and to finished inflaters are
    among those compared above)"""
    _, _, want = _plans()
    eos = O.ERROR_CODES["end_of_stream"]
    assert sum(Z.calls_after(w, Z.is_error) for w in want) >= 8
    assert sum(Z.calls_after(w, lambda st: st == eos) for w in want) >= 8
