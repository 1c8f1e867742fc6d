"""zs::Buf, zs::ScopedBuf and zs::reserve_all, the owners of the host
library's device and pinned memory (zeroskip_amd/csrc/zscrc_buf.h), on the CPU:
a stand-alone program (tests/c/devbuf.cpp) instantiates them with a malloc
backend that logs every allocation and free and can fail the k-th allocation,
and checks when the backend is called, the order free-then-allocate, the bytes
each site's slack gives against the site's earlier expression, the state after
a failed allocation, the order in which a call's buffers leave their scope, and
the group helper with a failure at every position.  The program is built with
the address and undefined-behaviour sanitizers and runs as its own process;
nothing is preloaded and nothing of it is loaded into python.  No GPU."""
import re
import subprocess

from tests import cprog

program = cprog.program_fixture("devbuf")


def test_sanitizers_are_linked(program):
    """The build with -fsanitize=address,undefined succeeded (without it the
    run below still checks every call and size, but sees no write outside a
    buffer, no use after a free and no leak)."""
    assert program[1]


def test_buffers_follow_the_rule_and_nothing_is_left(program):
    r = subprocess.run([program[0]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert re.fullmatch(r"ok [1-9]\d* checks, 0 live\n", r.stdout), r.stdout[-500:]
