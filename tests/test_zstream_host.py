"""CPU check of the per-stream inflate kernel's own logic
(beast_amd/csrc/pmd_zstream.hip, zstream_run) and of the library's call
protocol in front of it (beast_amd/csrc/inflate_reader.h), compiled for the
host by tests/model/zstream_host.py: every write()'s status, z_params and output
bytes must equal the oracle's restatement of Beast's inflate_stream.  The
GPU build of the same code runs the same cases in tests/test_gpu_zstream.py."""
import os
import subprocess

import pytest

from tests import zstream_cases as Z
from tests.model import zstream_host as H


def make(wbits):
    return H.HostInflater(wbits)


@pytest.mark.parametrize("kind", ["json", "binary", "random"])
@pytest.mark.parametrize("level,mem", [(1, 4), (6, 4), (9, 9), (6, 1)])
def test_connection_random_cuts(kind, level, mem):
    Z.case_connection_random_cuts(make, kind, level, mem)


def test_foreign_encoder_connection():
    Z.case_foreign_payloads(make)


@pytest.mark.parametrize("hpar", ["1", "0"])
def test_code_length_loops(hpar, monkeypatch):
    """The dynamic header's code lengths: hdr_par's windows (default) and the
    serial loop (BPMD_ZSTREAM_HPAR=0) against the oracle, under random cuts,
    input a byte at a time, the KATs and corrupted headers."""
    monkeypatch.setenv("BPMD_ZSTREAM_HPAR", hpar)
    Z.case_connection_random_cuts(make, "json", 8, 4)
    Z.case_byte_at_a_time_input(make)
    Z.case_kat_split(make, every_cut=False)
    Z.case_errors(make)


def test_output_room_one_byte():
    Z.case_output_room_one_byte(make, n_calls=1500)


def test_byte_at_a_time_input():
    Z.case_byte_at_a_time_input(make)


def test_flush_mix():
    Z.case_flush_mix(make)


def test_flush_trees_kat():
    Z.case_flush_trees_kat(make)


def test_kat_split():
    Z.case_kat_split(make)


def test_small_window():
    Z.case_small_window(make)


def test_end_of_stream():
    Z.case_end_of_stream(make)


def test_stored_blocks():
    Z.case_stored_blocks(make)


def test_errors():
    """(with the calls a connection makes after the error: BAD mode)"""
    Z.case_errors(make)


def test_reset_between_streams():
    Z.case_reset_between_streams(make)


def test_argument_checks():
    Z.case_argument_checks(make)


def test_output_over_four_mib():
    Z.case_output_over_four_mib(lambda w: H.GuardedHostInflater(w, 0xFF))


def test_protocol_header_needs_no_hip():
    """inflate_reader.h compiles with plain g++, warnings on, and includes beast_pmd.h, zstream.h and
    the standard library only."""
    header = os.path.join(H.CSRC, "inflate_reader.h")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include",
                        header, os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    deps = subprocess.run(["g++", "-std=c++17", "-MM", "-x", "c++", header], capture_output=True, text=True, check=True)
    names = {os.path.basename(p) for p in deps.stdout.replace("\\\n", " ").split()[1:]}
    assert names == {"inflate_reader.h", "beast_pmd.h", "zstream.h"}, names


@pytest.mark.parametrize("poison", [0x00, 0x5A, 0xFF])
def test_calls_stay_inside_their_buffers(poison):
    """The kernel contract the batcher's packing relies on (pmd_stream.hip
    inflate_batch; the 64-lane build: tests/test_gpu_zstream_guard.py): no
    store at or past out + cap (64 canary bytes there stay as they were) and
    results that do not depend on the bytes after in + n_in, which the
    16-byte staging loads read (the oracle's records whatever they hold)."""
    def guarded(wbits):
        return H.GuardedHostInflater(wbits, poison)

    before = H.GuardedHostInflater.total_calls
    Z.case_connection_random_cuts(guarded, "json", 6, 4)
    Z.case_connection_random_cuts(guarded, "random", 1, 4)
    Z.case_flush_mix(guarded)
    Z.case_stored_blocks(guarded)
    Z.case_errors(guarded)
    Z.case_small_window(guarded)
    assert H.GuardedHostInflater.total_calls - before > 1000   # the guards were in place


def test_lockstep_plans_every_call():
    """The plans of the GPU lockstep and guard tests (Z.mixed_plans), every
    call made whatever the status, guarded, against the oracle."""
    for R, seed in ((100, 0), (40, 0), (40, 1)):
        for name, (stream, wbits, calls) in Z.mixed_plans(R, seed):
            Z.compare(lambda w: H.GuardedHostInflater(w, 0xFF), stream, calls, wbits=wbits, label=name, stop=False)


def test_issue3028_one_byte_reads():
    msg = Z.issue3028_message()
    from oracle import oracle as O
    pays = O.pmd_deflate_stream([msg] * 3, 8, 15, 4)
    res = Z.ws_replay(make, [[p] for p in pays], size=1)
    assert all(r == (msg, 0) for r in res)


def test_issue1630_packets():
    from oracle import oracle as O
    frames = Z.issue1630_frames()
    res = Z.ws_replay(make, [[p] for _, p in frames], size=4096)
    for got, st in res:
        assert st == 0 and O.utf8_check(got) == 0
