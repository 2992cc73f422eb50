#!/usr/bin/env python3
"""Digest of the machine code the build emits, one line per csrc/*.hip:

    file  sha256(.text)  sha256(.rodata)

of the device code object (--host: of the host object).  Two compiles of one
source differ as whole files (symbol names carry a per-compile id); these two
sections do not, and .rodata holds the kernel descriptors (register counts,
LDS sizes).  Equal listings before and after a source change mean the change
emitted the same kernels.  CPU only.

Removing a kernel from a unit changes the unit's .text, so --kernels lists
the device functions one by one instead:

    file  function  sha256(instructions)  sha256(descriptor)

from the unit's device assembly, cut at each function's .type / .size.  The
instructions are the function's lines without comments, its local labels
numbered from zero in order of appearance (the compiler numbers them by the
function's position in the unit); the descriptor is its .amdhsa_kernel block
and resource symbols (VGPRs, SGPRs, LDS, scratch).  Neither depends on what
else the unit holds.  A function in both listings with equal digests is the
same function.

    python scripts/codeobj_digest.py <tree root> [--prof] [--host | --kernels] [unit.hip ...] [extra flags]
"""
import concurrent.futures as cf
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from beast_amd.build import ARCH, CXXFLAGS, HIPCC, SRC_FLAGS  # noqa: E402

LLVM = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "lib", "llvm", "bin")
MODES = ("--prof", "--host", "--kernels")


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


LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def functions(asm):
    """{function: (instruction lines, descriptor lines)} of a device assembly listing."""
    out, body, labels, in_desc = {}, None, {}, False
    for raw in asm.splitlines():
        line = raw.split(";", 1)[0].strip()
        m = re.match(r"\.type\s+(\S+),@function", line)
        res = re.match(r"\.set (\S+)\.\w+,", line)   # resource symbols, after .size
        if m:
            body, labels = ([], []), {}
            out[m.group(1)] = body
        elif line.startswith(".size"):
            body = None
        elif res and res.group(1) in out:
            out[res.group(1)][1].append(line)
        elif not line or body is None:
            pass
        elif line.startswith(".amdhsa_kernel") or line.startswith(".end_amdhsa_kernel"):
            in_desc = line.startswith(".amdhsa_kernel")
        elif in_desc:
            body[1].append(line)
        elif not line.startswith((".Lfunc_end", ".section", ".text", ".p2align")):
            body[0].append(LOCAL.sub(lambda l: ".L%d" % labels.setdefault(l.group(0), len(labels)), line))
    return out


def kernel_digests(csrc, src, flags, tmp):
    asm = os.path.join(tmp, src[:-4] + ".s")
    subprocess.run([HIPCC, *CXXFLAGS, *SRC_FLAGS.get(src, []), *flags, "-w", "--cuda-device-only", "-S",
                    os.path.join(csrc, src), "-o", asm], check=True)
    with open(asm) as f:
        fns = functions(f.read())
    sha = lambda lines: hashlib.sha256("\n".join(lines).encode()).hexdigest()  # noqa: E731
    # (a library template's name runs to thousands of characters)
    short = lambda n: n if len(n) <= 100 else n[:84] + "~" + hashlib.sha256(n.encode()).hexdigest()[:15]  # noqa: E731
    return "\n".join("  ".join((src, short(n), sha(c), sha(d))) for n, (c, d) in sorted(fns.items()))


def main(argv):
    root, rest = argv[0], [a for a in argv[1:] if a not in MODES]
    flags = [a for a in rest if not a.endswith(".hip")]
    if "--prof" in argv:
        flags.insert(0, "-DBPMD_PROF")
    csrc = os.path.join(root, "beast_amd", "csrc")
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    srcs = [s for s in srcs if s in rest] or srcs
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(max_workers=16) as ex:
        if "--kernels" in argv:
            one = lambda s: kernel_digests(csrc, s, flags, tmp)  # noqa: E731
        else:
            one = lambda s: digest(csrc, s, flags, "--host" in argv, tmp)  # noqa: E731
        for line in ex.map(one, srcs):
            print(line)


if __name__ == "__main__":
    main(sys.argv[1:])
