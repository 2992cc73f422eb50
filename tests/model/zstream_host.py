"""Host build of the per-stream inflate kernel's own code (test
infrastructure).

beast_amd/csrc/pmd_zstream.hip runs Beast's inflate_stream state machine as
wave-uniform code (zstream_run) with lane-strided bulk loops.  With
BPMD_ZSTREAM_HOST and one-lane meanings of the HIP intrinsics (lane 0,
WAVE = 1, readfirstlane = identity) that same source text is plain C++; the
wave-cooperative table builder is replaced by the serial builder it is
slot-for-slot equal to (huff_table.h; the equality is tests/test_gpu_tables.py).
This module compiles it for the host (tests/cpp/inflate_reader_backend.cpp:
the kernel source under tests/cpp/zstream_shim.h, behind the library's own
call protocol, beast_amd/csrc/inflate_reader.h) so the CPU suite can check
every write()'s z_params against the oracle without a GPU.  It is not the
oracle and not a product path.
"""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "beast_amd", "csrc")
CPP = os.path.join(HERE, "..", "cpp")
BACKEND = os.path.join(CPP, "inflate_reader_backend.cpp")
BUILD = os.path.join(HERE, "_build")
LIB = os.path.join(BUILD, "libzstream_host.so")
CXX = os.environ.get("BPMD_HOST_CXX", "g++")
_L = None


def build():
    os.makedirs(BUILD, exist_ok=True)
    deps = [BACKEND, os.path.join(CPP, "zstream_shim.h"), __file__] + [
        os.path.join(CSRC, f) for f in ("pmd_zstream.hip", "zstream.h", "huff_table.h", "inflate_reader.h", "status.h")]
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= max(os.path.getmtime(d) for d in deps):
        return LIB
    cmd = [CXX, "-O1", "-g", *os.environ.get("ZS_HOST_FLAGS", "").split(), "-std=c++17", "-fPIC", "-shared",
           "-o", LIB, BACKEND]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("host build of pmd_zstream.hip failed:\n" + r.stderr)
    return LIB


def lib():
    global _L
    if _L is None:
        L = ctypes.CDLL(build())
        vp = ctypes.c_void_p
        L.zs_host_state_bytes.restype = ctypes.c_size_t
        L.zs_host_reset.argtypes = [vp, ctypes.c_int]
        L.bpmd_inflate_stream_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.bpmd_inflate_stream_write.argtypes = [vp, vp, ctypes.c_int]
        L.bpmd_inflate_stream_reset.argtypes = [vp, ctypes.c_int]
        L.bpmd_inflate_stream_clear.argtypes = [vp]
        L.bpmd_stream_destroy.argtypes = [vp]
        L.irb_poison.argtypes = [vp, ctypes.c_int]
        L.irb_calls.argtypes = [vp, ctypes.POINTER(ctypes.c_uint)]
        L.irb_calls.restype = ctypes.c_ulonglong
        _L = L
    return _L


class HostInflater:
    """The host build behind the library's own call protocol
    (inflate_reader.h), called as tests/test_gpu_zstream.py's GpuInflater
    calls the device build."""

    def __init__(self, wbits=15):
        self.L = lib()
        self.h = ctypes.c_void_p()
        assert self.L.bpmd_inflate_stream_create(wbits, ctypes.byref(self.h)) == 0

    def write(self, zs, flush):
        r = self.L.bpmd_inflate_stream_write(self.h, ctypes.byref(zs), flush)
        assert r >= 0, f"C ABI error {r}"
        return r

    def reset(self, wbits=15):
        assert self.L.bpmd_inflate_stream_reset(self.h, wbits) == 0

    def clear(self):
        assert self.L.bpmd_inflate_stream_clear(self.h) == 0

    def close(self):
        self.L.bpmd_stream_destroy(self.h)


class GuardedHostInflater(HostInflater):
    """HostInflater with the call's buffers watched (the backend's step): 64
    canary bytes after out + cap that no call may change, and the 64 bytes
    after in + n_in (the staging loads read up to 15 of them) filled with
    `poison`, on which no result may depend."""
    total_calls = 0

    def __init__(self, wbits=15, poison=0x5A):
        super().__init__(wbits)
        self.L.irb_poison(self.h, poison)

    def write(self, zs, flush):
        n, room = zs.avail_in, zs.avail_out
        bad = ctypes.c_uint()
        before = self.L.irb_calls(self.h, None)
        r = self.L.bpmd_inflate_stream_write(self.h, ctypes.byref(zs), flush)
        assert self.L.irb_calls(self.h, ctypes.byref(bad)) == before + 1
        assert not bad.value & 1, ("out_used over the room", n, room, flush)
        assert not bad.value & 2, ("store past out + cap", n, room, flush)
        assert not bad.value & 4, ("store past in + n_in", n, room, flush)
        assert r >= 0, f"C ABI error {r}"
        return r

    def close(self):
        GuardedHostInflater.total_calls += self.L.irb_calls(self.h, None)
        super().close()
