"""The stand-alone C++ programs of tests/c/ that check the device stages'
host-side arithmetic: one build recipe.  A program is built with the address
and undefined-behaviour sanitizers and runs as its own process; nothing is
preloaded and nothing of it is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def program_fixture(name):
    """The module-scoped `program` fixture of a test module: (exe, sanitized)
    of tests/c/<name>.cpp, built without the sanitizers only where the build
    with them fails.  Use as `program = cprog.program_fixture("carve")`."""
    src = os.path.join(ROOT, "tests", "c", name + ".cpp")

    @pytest.fixture(scope="module")
    def program(tmp_path_factory):
        exe = str(tmp_path_factory.mktemp(name) / name)
        base = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", src, "-o", exe]
        r = subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:],
                           capture_output=True, text=True)
        sanitized = r.returncode == 0
        if not sanitized:
            print("sanitizer build failed, building without:\n" + r.stderr[-2000:])
            subprocess.run(base, check=True)
        return exe, sanitized

    return program
