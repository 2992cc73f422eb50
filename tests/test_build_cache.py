"""build.py's object cache: an object is reused only when it is newer than its
source and the headers AND was built by the same command line (kept in
<obj>.cmd).  Compiles nothing: files in tmp_path, the decision function alone."""
import os

from beast_amd import build

CMD = ["hipcc", "-O3", "-DBPMD_RING=8192", "-c", "a.hip", "-o", "a.o"]


def _tree(tmp_path, cmd=CMD):
    src, hdr, obj = (str(tmp_path / n) for n in ("a.hip", "a.h", "a.o"))
    for p, t in ((src, 1000), (hdr, 1000), (obj, 2000)):
        open(p, "w").close()
        os.utime(p, (t, t))
    if cmd is not None:
        with open(obj + ".cmd", "w") as f:
            f.write("\n".join(cmd))
    return src, hdr, obj


def test_same_command_fresh_object_is_reused(tmp_path):
    src, hdr, obj = _tree(tmp_path)
    assert not build._stale(obj, src, os.path.getmtime(hdr), list(CMD))


def test_changed_flag_recompiles(tmp_path):
    src, hdr, obj = _tree(tmp_path)
    other = [a.replace("8192", "4096") for a in CMD]
    assert build._stale(obj, src, os.path.getmtime(hdr), other)
    assert build._stale(obj, src, os.path.getmtime(hdr), CMD[:2] + CMD[3:])
    assert build._stale(obj, src, os.path.getmtime(hdr), CMD + ["-DBPMD_PROF"])


def test_missing_sidecar_recompiles(tmp_path):
    src, hdr, obj = _tree(tmp_path, cmd=None)
    assert build._stale(obj, src, os.path.getmtime(hdr), CMD)


def test_missing_object_recompiles(tmp_path):
    src, hdr, obj = _tree(tmp_path)
    os.remove(obj)
    assert build._stale(obj, src, os.path.getmtime(hdr), CMD)


def test_newer_source_or_header_recompiles(tmp_path):
    src, hdr, obj = _tree(tmp_path)
    os.utime(src, (3000, 3000))
    assert build._stale(obj, src, os.path.getmtime(hdr), CMD)
    os.utime(src, (1000, 1000))
    assert not build._stale(obj, src, os.path.getmtime(hdr), CMD)
    os.utime(hdr, (3000, 3000))
    assert build._stale(obj, src, os.path.getmtime(hdr), CMD)
