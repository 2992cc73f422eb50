"""The lane kernel's list of coded runs (beast_amd/csrc/hdr_list.h) on the
CPU: tests/cpp/hdr_list_main.cpp checks the fit rule over every (entries,
coded symbols) pair and list placement against the walk over every symbol."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BUILD = os.path.join(CPP, "_build")


def test_fit_rule_and_list_placement():
    os.makedirs(BUILD, exist_ok=True)
    src, out = os.path.join(CPP, "hdr_list_main.cpp"), os.path.join(BUILD, "hdr_list_main")
    hdr = os.path.join(ROOT, "beast_amd", "csrc", "hdr_list.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
