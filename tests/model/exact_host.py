"""Host build of the exact-mode deflater (test infrastructure): compiles
tests/cpp/exact_host_backend.cpp -- beast_amd/csrc/deflate_exact_core.h under
the one-lane meanings of tests/cpp/exact_shim.h, in arrays sized by
exact_plan.h -- with clang++, so the CPU suite can check the deflater's
decisions against the oracle.  Not the oracle, not a product path."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "beast_amd", "csrc")
CPP = os.path.join(HERE, "..", "cpp")
BACKEND = os.path.join(CPP, "exact_host_backend.cpp")
DEPS = [BACKEND, os.path.join(CPP, "exact_shim.h"), __file__] + [
    os.path.join(CSRC, f) for f in ("deflate_exact_core.h", "exact_plan.h", "send_plan.h", "status.h")]
BUILD = os.path.join(HERE, "_build")
LIB = os.path.join(BUILD, "libexact_host.so")
CLANG = os.environ.get("BPMD_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
_L = None


def build():
    os.makedirs(BUILD, exist_ok=True)
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= max(map(os.path.getmtime, DEPS)):
        return LIB
    # a per-process name and an atomic rename: parallel test workers (pytest -n)
    # may build at once, and one must never load a half-written library
    tmp = "%s.%d.tmp" % (LIB, os.getpid())
    subprocess.run([CLANG, "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-function", BACKEND, "-o", tmp], check=True)
    os.replace(tmp, LIB)
    return LIB


def lib():
    global _L
    if _L is None:
        _L = ctypes.CDLL(build())
        _L.dx_host.restype = ctypes.c_int32
        _L.dx_host.argtypes = [ctypes.c_int] * 4 + [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                                   ctypes.c_int]
    return _L


def deflate(msg: bytes, level=6, wbits=15, mem=4, strategy=0, cap=None, tier=None):
    """(status, payload): status 0, or 1 (need_buffers) as the kernel reports.  tier 0, 1, 2: in arrays of
    exactly that tier's sizes; None: the workspace tier's, whatever the length."""
    if cap is None:
        cap = len(msg) + ((len(msg) + 7) >> 3) + ((len(msg) + 63) >> 6) + 11
    out = ctypes.create_string_buffer(max(cap, 1))
    r = lib().dx_host(level, wbits, mem, strategy, msg, len(msg), out, cap, -1 if tier is None else tier)
    assert r >= -1, ("not this tier's message", len(msg), mem, tier, r)
    return (1, b"") if r < 0 else (0, out.raw[:r])
