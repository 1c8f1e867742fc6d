"""bench.py --gpus N never measures fewer GPUs than asked: without a launcher
it starts torchrun itself (one rank per GPU, 127.0.0.1) before anything
touches a GPU; a WORLD_SIZE that disagrees with --gpus is an error.  CPU only
(BENCH_LAUNCH_DRYRUN prints the launch instead of running it)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e,
                          capture_output=True, text=True, timeout=120)


def test_gpus_without_launcher_spawns_torchrun():
    p = _run(["--gpus", "4", "--steps", "3", "--warmup", "1"], BENCH_LAUNCH_DRYRUN="1")
    assert p.returncode == 0, p.stderr
    cmd = json.loads(p.stdout.strip().splitlines()[-1])["launch"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == [os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "3", "--warmup", "1"][-6:]


def test_world_size_mismatch_is_an_error():
    p = _run(["--gpus", "4"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert p.returncode != 0 and "WORLD_SIZE=2" in (p.stderr + p.stdout)


def test_dump_outputs_writes_float64_within_the_limit(tmp_path):
    """--dump-outputs DIR: one DIR/<name>.npy per array, float64 (exact for
    32-bit CRCs), per-rank names with more than one rank, at most 64 MB."""
    import argparse
    import numpy as np
    import pytest
    import bench
    crc = np.array([0, 1, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    args = argparse.Namespace(dump_outputs=str(tmp_path / "d"))
    bench.dump_outputs(args, 1, 0, {"crc": crc})
    got = np.load(tmp_path / "d" / "crc.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.uint32), crc)
    bench.dump_outputs(args, 2, 1, {"crc": crc})
    assert (tmp_path / "d" / "crc_rank1.npy").exists()
    assert bench.DUMP_MAX_BYTES == 64 << 20
    with pytest.raises(SystemExit):
        bench.dump_outputs(args, 1, 0, {"big": np.zeros((64 << 20) // 8 + 1, dtype=np.uint32)})


def test_full_and_dump_outputs_are_options():
    p = _run(["--help"])
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
    p = _run(["--steps", "0"])
    assert p.returncode != 0 and "--steps" in p.stderr


def test_traffic_only_for_its_own_kernel():
    """a PMC traffic record is reported only on the line of the
    kernel it was measured on (profiles/pmc_traffic.json is keyed by config
    and names its kernel)."""
    import json
    import bench
    rec = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    for cfg in ("config2", "config3", "config4", "config5"):
        assert cfg in rec and rec[cfg]["kernel"] and rec[cfg]["bytes_per_launch"] > 0, cfg
        assert os.path.exists(os.path.join(ROOT, rec[cfg]["record"])), rec[cfg]["record"]
        t, src = bench.traffic_for(cfg, rec[cfg]["kernel"])
        assert t == rec[cfg]["bytes_per_launch"]
        t, src = bench.traffic_for(cfg, rec[cfg]["kernel"] + "+another_kernel")
        assert t is None and "not reported" in src
