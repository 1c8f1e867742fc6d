"""libzscrc's host side from eight threads at once (tests/c/thread_race.c):
the drop-in CRCs, crc32c_combine / zscrc_shift, the zeroskip parsers on the
reference-written fixtures and the diagnostics, started behind a barrier so
the library's lazily built state is first reached by several threads
together, while one thread flips the process-global tuners.  Every thread
must compute what one thread alone computes.

Plain: the driver against the in-tree libzscrc.so.  ThreadSanitizer: the
library's host objects rebuilt with the host-only thread sanitizer flag
(tools/asan_fuzz.sh's recipe; the kernels' objects as build() left them) and linked
into the driver -- a stand-alone program on the CPU, the sanitizer's runtime
linked statically, nothing preloaded, no GPU call."""
import glob
import json
import os
import shutil
import subprocess

import pytest

from oracle import zs_format as zf
from zeroskip_amd import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ref_format")
FILES = ["active_clean.zs", "active_corrupt.zs", "active_stale.zs", "active_longkey.zs", "packed.zs",
         "repack1/reference_out.zs", "repack2/reference_out.zs"]
SRC = os.path.join(ROOT, "tests", "c", "thread_race.c")
PKG = os.path.join(ROOT, "zeroskip_amd")
HIPCC = "/opt/rocm/bin/hipcc"
CLANG = "/opt/rocm/llvm/bin/clang"
HOST_OBJS = ["zscrc_api", "zscrc_zs", "zscrc_consistent", "zscrc_gf2", "zscrc_cpu", "zscrc_pack", "zscrc_files",
             "zscrc_repack", "zscrc_cpass", "zscrc_fill", "zscrc_scratch"]
KERNEL_OBJS = ["zscrc_kernels", "zscrc_walk"]
# the driver makes no device call; this keeps the process off every GPU whatever it links
NO_GPU = {"ZSCRC_GPU_MIN": "0", "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = tmp_path_factory.mktemp("race_images")
    (d / "dotzsdb").write_bytes(zf.dotzsdb_bytes(4096, b"00010203-0405-0607-0809-0a0b0c0d0e0f\0", 8))
    return [os.path.join(FIX, f) for f in FILES] + [str(d / "dotzsdb")]


def _check(out):
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-4000:])
    rep = json.loads(out.stdout)
    assert rep["mismatches"] == 0 and rep["threads"] == 8 and rep["rounds"] >= 200


def test_threads_agree(images, tmp_path):
    exe = tmp_path / "thread_race"
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
                           "-L", os.path.dirname(LIB_PATH), "-lzscrc", f"-Wl,-rpath,{os.path.dirname(LIB_PATH)}",
                           "-o", str(exe)])
    out = subprocess.run([str(exe), *images], capture_output=True, text=True, timeout=300,
                         env={**os.environ, **NO_GPU})
    _check(out)


def test_threads_under_thread_sanitizer(images, tmp_path):
    if not glob.glob("/opt/rocm/llvm/lib/clang/*/lib/linux/libclang_rt.tsan*"):
        pytest.skip("/opt/rocm/llvm has no libclang_rt.tsan")
    w = tmp_path / "zeroskip_amd"
    w.mkdir()
    shutil.copytree(os.path.join(PKG, "csrc"), w / "csrc")
    shutil.copy(os.path.join(PKG, "Makefile"), w / "Makefile")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    # host code only, on every compiler line: the device code objects are plain gfx950
    san = "-Xarch_host -fsanitize=thread -fno-omit-frame-pointer -g"
    subprocess.check_call(
        ["make", "-s", "-j8",
         "HIPFLAGS=-O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Xarch_host -fsanitize=thread "
         "-Xarch_host -fno-omit-frame-pointer",
         f"CC={CLANG}", f"CFLAGS=-O1 -fPIC -std=gnu11 {san}", f"CXX={CLANG}++ {san}",
         *[f"build/{o}.o" for o in HOST_OBJS]], cwd=w)
    # the kernels' objects unsanitized, as build() left them; built plainly where a checkout has none
    for o in KERNEL_OBJS:
        have = os.path.join(PKG, "build", o + ".o")
        if os.path.exists(have):
            shutil.copy(have, w / "build" / (o + ".o"))
    subprocess.check_call(["make", "-s", "-j2", *[f"build/{o}.o" for o in KERNEL_OBJS]], cwd=w)
    exe = tmp_path / "thread_race_tsan"
    drv = tmp_path / "thread_race.o"
    subprocess.check_call([CLANG, "-O1", "-Wall", "-Werror", *san.split(), "-I", str(tmp_path / "include"), "-c", SRC,
                           "-o", str(drv)])
    subprocess.check_call([*f"{HIPCC} --offload-arch=gfx950 -Xarch_host -fsanitize=thread".split(), str(drv),
                           *[str(w / "build" / (o + ".o")) for o in HOST_OBJS + KERNEL_OBJS], "-lpthread",
                           "-o", str(exe)])
    out = subprocess.run([str(exe), *images], capture_output=True, text=True, timeout=600,
                         env={**os.environ, **NO_GPU, "TSAN_OPTIONS": "halt_on_error=1:exitcode=66"})
    assert "ThreadSanitizer" not in out.stderr, out.stderr[-6000:]
    _check(out)
