#!/usr/bin/env python3
"""Digest of the machine code the build emits, one line per csrc/*.hip:

    file  sha256(.text)  sha256(.rodata)

of the device code object (--host: of the host object).  Two compiles of one
source differ as whole files (symbol names carry a per-compile id); these two
sections do not, and .rodata holds the kernel descriptors (register counts,
LDS sizes).  Equal listings before and after a source change mean the change
emitted the same kernels.  CPU only.

    python scripts/codeobj_digest.py <tree root> [--prof] [--host] [extra flags]
"""
import concurrent.futures as cf
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from beast_amd.build import ARCH, CXXFLAGS, HIPCC, SRC_FLAGS  # noqa: E402

LLVM = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "lib", "llvm", "bin")


def digest(csrc, src, flags, host, tmp):
    stem = os.path.join(tmp, src[:-4])
    obj = stem + ".o"
    side = "--cuda-host-only" if host else "--cuda-device-only"
    subprocess.run([HIPCC, *CXXFLAGS, *SRC_FLAGS.get(src, []), *flags, side, "-c",
                    os.path.join(csrc, src), "-o", obj], check=True)
    if not host:
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                        f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}", f"--input={obj}",
                        f"--output={stem}.co"], check=True)
        obj = stem + ".co"
    out = [src]
    for sec in (".text", ".rodata"):
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", f"--only-section={sec}",
                        obj, stem + sec], check=True)
        with open(stem + sec, "rb") as f:
            out.append(hashlib.sha256(f.read()).hexdigest())
    return "  ".join(out)


def main(argv):
    root, flags = argv[0], [a for a in argv[1:] if a not in ("--prof", "--host")]
    if "--prof" in argv:
        flags.insert(0, "-DBPMD_PROF")
    csrc = os.path.join(root, "beast_amd", "csrc")
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(max_workers=16) as ex:
        for line in ex.map(lambda s: digest(csrc, s, flags, "--host" in argv, tmp), srcs):
            print(line)


if __name__ == "__main__":
    main(sys.argv[1:])
