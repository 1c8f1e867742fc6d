"""zs::Carve, the scratch layout of the device stages
(zeroskip_amd/csrc/zscrc_carve.h), on the CPU: a stand-alone program
(tests/c/carve.cpp) carves pieces of mixed types, counts and alignments, zero
counts among them, on a NULL base and on a buffer of exactly the bytes the NULL
run gave, and checks that both runs give the same bytes(), that every piece is
aligned as asked, that the pieces are disjoint and in order and that the last
one ends at bytes().  The program is built with the address and
undefined-behaviour sanitizers and runs as its own process; nothing is
preloaded and nothing of it is loaded into python.  No GPU."""
import subprocess

from tests import cprog

program = cprog.program_fixture("carve")


def test_sanitizers_are_linked(program):
    """The build with -fsanitize=address,undefined succeeded (without it the
    run below still checks every offset, but sees no write outside the buffer)."""
    assert program[1]


def test_null_base_and_buffer_agree(program):
    r = subprocess.run([program[0]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.startswith("ok 7 cases")


def test_a_write_past_the_carved_bytes_is_seen(program):
    """The buffer is exactly bytes() long: one byte more fails the sanitized run."""
    assert program[1]
    r =subprocess.run([program[0], "overrun"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, (r.stdout[-500:], r.stderr[-3000:])
