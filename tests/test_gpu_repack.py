"""The packed-file writer (zscrc_pack_*, the repack output path of
src/zeroskip-packed.c:384-473) against the format oracle: byte-for-byte equal
files, records-region and pointer-section CRCs computed on the GPU."""
import os

import numpy as np
import pytest

from oracle import oracle
from oracle import zs_format as zf
from tests.images import UUID, UUIDSTR
from tests.pack_cases import records as _records
from zeroskip_amd import repack, zsfile
from zeroskip_amd._lib import ZscrcError, stats

pytestmark = pytest.mark.gpu


def _pack(path, recs, chunk=0, start=2, end=9):
    before = stats()
    with repack.Packer(str(path), UUID, start, end, chunk_bytes=chunk) as p:
        for k, v in recs:
            p.add(k, v)
    after = stats()
    assert after[3] - before[3] >= p.report["region_bytes"], "records region not checksummed on the GPU"
    return p.report, open(path, "rb").read()


@pytest.mark.parametrize("chunk", [0, 4096, 65536 + 4096])
def test_pack_matches_oracle_short(gpu, tmp_path, chunk):
    recs = _records(3000, 5)
    rep, img = _pack(tmp_path / "p", recs, chunk)
    want = zf.packed_file(recs, UUID, 2, 9)
    assert img == want
    assert rep["records"] == len(recs) and rep["file_bytes"] == len(want)
    assert rep["region_crc"] == oracle.crc32c_hw(0, want[40:40 + rep["region_bytes"]])
    r = zsfile.verify_image(img, zsfile.PACKED)
    assert r["walk_rc"] == 0 and r["n_commits"] == 2 and r["n_bad"] == 0


def test_pack_batch_api(gpu, tmp_path):
    """zscrc_pack_add_batch (Packer.add_many / add_arrays) writes the same
    bytes as per-record adds: deletes, empty values, shared value bytes."""
    recs = _records(3000, 6)
    recs[10] = (recs[10][0], b"")
    want = zf.packed_file(recs, UUID, 2, 9)
    with repack.Packer(str(tmp_path / "m"), UUID, 2, 9, chunk_bytes=8192) as p:
        p.add_many(recs[:1000])
        p.add_many(recs[1000:])
    assert open(tmp_path / "m", "rb").read() == want
    # values sharing bytes: record i -> the same 40 bytes at offset 8 * (i % 5)
    vals = np.arange(80, dtype=np.uint8)
    keys = [b"k%07d" % i for i in range(500)]
    kb = np.frombuffer(b"".join(keys), dtype=np.uint8)
    koff = np.arange(500, dtype=np.uint64) * 8
    klen = np.full(500, 8, np.uint64)
    voff = (np.arange(500, dtype=np.uint64) % 5) * 8
    voff[7] = ~np.uint64(0)
    vlen = np.full(500, 40, np.uint64)
    with repack.Packer(str(tmp_path / "a"), UUID, 2, 9) as p:
        p.add_arrays(kb, koff, klen, vals, voff, vlen)
    recs2 = [(k, None if i == 7 else vals[8 * (i % 5):8 * (i % 5) + 40].tobytes()) for i, k in enumerate(keys)]
    assert open(tmp_path / "a", "rb").read() == zf.packed_file(recs2, UUID, 2, 9)


@pytest.mark.parametrize("chunk", [0, 1 << 20])
def test_pack_long_commit_long_records(gpu, tmp_path, chunk):
    """Records region above 16 MiB (long commit), a 17 MiB value (long value
    record), a 70,000-byte key (long key record), an empty value."""
    recs = _records(2500, 9, maxval=9000)
    big = np.random.default_rng(1).integers(0, 256, (17 << 20) + 3, dtype=np.uint8).tobytes()
    recs.insert(100, (b"%016d" % 700 + b"+big", big))
    recs.insert(200, (b"%016d" % 1400 + b"+long-key" + b"q" * 70000, b"v" * 33))
    recs.insert(300, (b"%016d" % 2100 + b"+empty", b""))
    rep, img = _pack(tmp_path / "p", recs, chunk)
    want = zf.packed_file(recs, UUID, 2, 9)
    assert rep["region_bytes"] > zf.MAX_SHORT_VAL_LEN
    assert img == want
    chk = zf.packed_check(img)
    assert all(c["ok"] for c in chk)
    assert chk[1]["stored"] == rep["commit_crc"] and chk[0]["stored"] == rep["final_crc"]


def test_pack_empty(gpu, tmp_path):
    rep, img = _pack(tmp_path / "p", [])
    assert img == zf.packed_file([], UUID, 2, 9)
    assert rep["records"] == 0 and rep["region_bytes"] == 0


def _dotzsdb(path, curidx):
    with open(path / ".zsdb", "wb") as fh:
        fh.write(zf.dotzsdb_bytes(4096, UUIDSTR.encode() + b"\0", curidx))


def test_repack_dir_finalised_files(gpu, tmp_path):
    """zsdb_repack branch 1 over a DB directory (zscrc_zs_repack): finalised
    files merged (newest record of a key wins, deletes kept), one packed
    file out, the sources unlinked, .zsdb rewritten -- byte for byte the
    format oracle's."""
    rng = np.random.default_rng(3)
    images = []
    for idx in range(3, 8):
        w = zf.FileWriter(UUID, idx=idx)
        for t in range(200):
            k = b"%016d" % int(rng.integers(0, 500))
            if t % 17 == 3:
                w.remove(k)
            else:
                w.add(k, rng.integers(0, 256, int(rng.integers(0, 400)), dtype=np.uint8).tobytes())
            w.commit()
        images.append(w.image())
        with open(tmp_path / f"zeroskip-{UUIDSTR}-{idx}-{idx}", "wb") as fh:
            fh.write(images[-1])
    # an active file and an older packed file stay as they are
    (tmp_path / f"zeroskip-{UUIDSTR}-8").write_bytes(zf.FileWriter(UUID, idx=8).image())
    old = zf.packed_file(_records(50, 1), UUID, 0, 2)
    (tmp_path / f"zeroskip-{UUIDSTR}-0-2").write_bytes(old)
    _dotzsdb(tmp_path, 8)
    before = stats()
    rep = repack.repack_dir(str(tmp_path))
    assert stats()[3] - before[3] >= rep["pack"]["region_bytes"]
    want = zf.packed_file(zf.repack_finalised(images), UUID, 3, 7)
    out = tmp_path / f"zeroskip-{UUIDSTR}-3-7"
    assert rep["branch"] == 1 and rep["path"] == str(out) and (rep["startidx"], rep["endidx"]) == (3, 7)
    assert open(out, "rb").read() == want
    assert rep["records_out"] == len(zf.repack_finalised(images)) and rep["records_in"] == 1000
    assert sorted(os.listdir(tmp_path)) == sorted([".zsdb", f"zeroskip-{UUIDSTR}-0-2", f"zeroskip-{UUIDSTR}-3-7",
                                                   f"zeroskip-{UUIDSTR}-8"])
    assert open(tmp_path / ".zsdb", "rb").read() == zf.dotzsdb_bytes(4096, UUIDSTR.encode() + b"\0", 8)


def test_repack_dir_packed_files(gpu, tmp_path):
    """zsdb_repack branch 2 (src/zeroskip.c:1510-1565): no finalised files,
    three packed files -> the first two of the reference's pflist (the two
    newest) merged by its packed-files iterator (the older of the two wins a
    key in both; a winning delete drops the key), byte for byte against the
    format oracle; a long records region (long commit) on the way."""
    rng = np.random.default_rng(8)

    def recs(n, lo, hi, vmax):
        out = {}
        for _ in range(n):
            k = b"%016d" % int(rng.integers(lo, hi))
            out[k] = None if rng.integers(0, 9) == 0 else rng.integers(0, 256, int(rng.integers(0, vmax)),
                                                                     dtype=np.uint8).tobytes()
        return sorted(out.items())
    files = {(0, 3): recs(400, 0, 900, 300), (4, 7): recs(3000, 300, 40000, 14000), (8, 9): recs(600, 0, 5000, 500)}
    imgs = {}
    for (s_, e_), r in files.items():
        imgs[(s_, e_)] = zf.packed_file(r, UUID, s_, e_)
        (tmp_path / f"zeroskip-{UUIDSTR}-{s_}-{e_}").write_bytes(imgs[(s_, e_)])
    _dotzsdb(tmp_path, 10)
    rep = repack.repack_dir(str(tmp_path))
    want = zf.packed_file(zf.repack_packed(imgs[(4, 7)], imgs[(8, 9)]), UUID, 4, 9)
    out = tmp_path / f"zeroskip-{UUIDSTR}-4-9"
    assert rep["branch"] == 2 and rep["files_merged"] == 2 and rep["path"] == str(out)
    assert open(out, "rb").read() == want
    assert rep["pack"]["region_bytes"] > zf.MAX_SHORT_VAL_LEN
    assert sorted(os.listdir(tmp_path)) == sorted([".zsdb", f"zeroskip-{UUIDSTR}-0-3", f"zeroskip-{UUIDSTR}-4-9"])
    r = zsfile.verify_image(open(out, "rb").read(), zsfile.PACKED)
    assert r["n_bad"] == 0 and r["n_commits"] == 2
    # nothing left to pack: branch 0, .zsdb still rewritten
    rep2 = repack.repack_dir(str(tmp_path))
    assert rep2["branch"] == 2            # 0-3 and 4-9 are two packed files
    rep3 = repack.repack_dir(str(tmp_path))
    assert rep3["branch"] == 0 and len([f for f in os.listdir(tmp_path) if f.startswith("zeroskip")]) == 1


def test_packer_abort_removes_file(gpu, tmp_path):
    """an exception inside the Packer context writes no commits and removes
    the partial file (the reference xunlinks it, zeroskip-packed.c:465-466)"""
    path = tmp_path / "partial"
    with pytest.raises(RuntimeError):
        with repack.Packer(str(path), UUID, 1, 2) as p:
            p.add(b"a" * 16, b"x" * 100)
            raise RuntimeError("interrupted")
    assert not path.exists()


def test_repack_dir_single_finalised_file(gpu, tmp_path):
    """One finalise followed by a repack: the output name
    zeroskip-<uuid>-<i>-<i> is the source's own.  The packed file replaces the
    finalised file (written under a temporary name, renamed after the source
    is unmapped); nothing is lost, the output is not unlinked."""
    rng = np.random.default_rng(12)
    w = zf.FileWriter(UUID, idx=4)
    for t in range(300):
        w.add(b"%016d" % int(rng.integers(0, 200)), rng.integers(0, 256, 100, dtype=np.uint8).tobytes())
        w.commit()
    img = w.image()
    name = f"zeroskip-{UUIDSTR}-4-4"
    (tmp_path / name).write_bytes(img)
    (tmp_path / f"zeroskip-{UUIDSTR}-5").write_bytes(zf.FileWriter(UUID, idx=5).image())
    _dotzsdb(tmp_path, 5)
    rep = repack.repack_dir(str(tmp_path))
    assert rep["branch"] == 1 and rep["path"] == str(tmp_path / name) and (rep["startidx"], rep["endidx"]) == (4, 4)
    want = zf.packed_file(zf.repack_finalised([img]), UUID, 4, 4)
    assert open(tmp_path / name, "rb").read() == want
    assert sorted(os.listdir(tmp_path)) == sorted([".zsdb", name, f"zeroskip-{UUIDSTR}-5"])
    r = zsfile.verify_image(want, zsfile.PACKED)
    assert r["n_bad"] == 0 and r["n_commits"] == 2


def test_repack_dir_lock_held(gpu, tmp_path):
    """A held .zsdb.lock (another writer inside zs_dotzsdb_update_begin /
    _end) makes repack refuse with ZSCRC_EBUSY and touch nothing; the lock
    is released (removed) by a repack that ran."""
    w = zf.FileWriter(UUID, idx=1)
    w.add(b"k" * 16, b"v" * 40)
    w.commit()
    (tmp_path / f"zeroskip-{UUIDSTR}-1-1").write_bytes(w.image())
    _dotzsdb(tmp_path, 2)
    (tmp_path / ".zsdb.lock").write_bytes(b"held")
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(ZscrcError, match="status -5"):
        repack.repack_dir(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == before
    assert (tmp_path / ".zsdb.lock").read_bytes() == b"held"
    os.unlink(tmp_path / ".zsdb.lock")
    rep = repack.repack_dir(str(tmp_path))
    assert rep["branch"] == 1 and not (tmp_path / ".zsdb.lock").exists()
    # a repack that fails after taking the lock (bad .zsdb) releases it
    (tmp_path / ".zsdb").write_bytes(b"\0" * 61)
    with pytest.raises(ZscrcError):
        repack.repack_dir(str(tmp_path))
    assert not (tmp_path / ".zsdb.lock").exists()


def test_repack_dir_rename_failure_releases_lock(gpu, tmp_path, monkeypatch):
    """a repack whose final .zsdb rename fails (fault injected,
    ZSCRC_FAULT=dotzsdb_rename) reports an error and leaves no .zsdb.lock
    behind, so the next update can take it; the old .zsdb is untouched."""
    for i in (1, 2):
        w = zf.FileWriter(UUID, idx=i)
        w.add(b"k%015d" % i, b"v" * 40)
        w.commit()
        (tmp_path / f"zeroskip-{UUIDSTR}-{i}-{i}").write_bytes(w.image())
    _dotzsdb(tmp_path, 3)
    old = (tmp_path / ".zsdb").read_bytes()
    monkeypatch.setenv("ZSCRC_FAULT", "dotzsdb_rename")
    with pytest.raises(ZscrcError):
        repack.repack_dir(str(tmp_path))
    assert not (tmp_path / ".zsdb.lock").exists()
    assert (tmp_path / ".zsdb").read_bytes() == old
    monkeypatch.delenv("ZSCRC_FAULT")
    # the lock is free: the next repack takes it (only the packed output
    # zeroskip-<uuid>-1-2 is left: nothing to merge, .zsdb rewritten)
    rep = repack.repack_dir(str(tmp_path))
    assert rep["branch"] == 0 and not (tmp_path / ".zsdb.lock").exists()
    assert (tmp_path / f"zeroskip-{UUIDSTR}-1-2").exists()


@pytest.mark.parametrize("seed", range(6))
def test_random_repack_finalised(gpu, tmp_path, seed):
    """zsdb_repack branch 1 on random DBs: 1-7 finalised files of random
    transactions (binary keys of 1-40 bytes from a small key space so keys
    repeat across files, values of 0-5,000 bytes, deletes, several records
    per commit): the packed file byte for byte the format oracle's merge."""
    rng = np.random.default_rng(100 + seed)
    keys = [bytes(rng.integers(0, 256, int(rng.integers(1, 41)), dtype=np.uint8)) for _ in range(300)]
    nfiles = int(rng.integers(1, 8))
    images = []
    for idx in range(3, 3 + nfiles):
        w = zf.FileWriter(UUID, idx=idx)
        for t in range(int(rng.integers(0, 120))):
            k = keys[int(rng.integers(0, len(keys)))]
            if rng.random() < 0.1:
                w.remove(k)
            else:
                w.add(k, rng.integers(0, 256, int(rng.choice([0, 10, 300, 5000])), dtype=np.uint8).tobytes())
            if rng.random() < 0.4:
                w.commit()
        w.commit()
        images.append(w.image())
        with open(tmp_path / f"zeroskip-{UUIDSTR}-{idx}-{idx}", "wb") as fh:
            fh.write(images[-1])
    last = 3 + nfiles
    (tmp_path / f"zeroskip-{UUIDSTR}-{last}").write_bytes(zf.FileWriter(UUID, idx=last).image())
    _dotzsdb(tmp_path, last)
    rep = repack.repack_dir(str(tmp_path))
    want_recs = zf.repack_finalised(images)
    out = tmp_path / f"zeroskip-{UUIDSTR}-3-{last - 1}"
    assert rep["branch"] == 1 and rep["path"] == str(out), rep
    assert open(out, "rb").read() == zf.packed_file(want_recs, UUID, 3, last - 1), seed
    assert rep["records_out"] == len(want_recs)


@pytest.mark.parametrize("seed", range(6))
def test_random_repack_packed(gpu, tmp_path, seed):
    """zsdb_repack branch 2 on random pairs of packed files: binary keys of
    1-40 bytes from one key space (overlapping between the files), values of
    0-5,000 bytes, deletes on both sides -- the merged file byte for byte the
    format oracle's packed-files merge (the older wins a key in both, a
    winning delete drops it)."""
    rng = np.random.default_rng(200 + seed)
    keys = [bytes(rng.integers(0, 256, int(rng.integers(1, 41)), dtype=np.uint8)) for _ in range(500)]

    def recs(n):
        out = {}
        for _ in range(n):
            k = keys[int(rng.integers(0, len(keys)))]
            out[k] = None if rng.random() < 0.1 else rng.integers(
                0, 256, int(rng.choice([0, 10, 300, 5000])), dtype=np.uint8).tobytes()
        return sorted(out.items())
    a, b = zf.packed_file(recs(int(rng.integers(0, 400))), UUID, 2, 4), zf.packed_file(
        recs(int(rng.integers(0, 400))), UUID, 5, 8)
    (tmp_path / f"zeroskip-{UUIDSTR}-2-4").write_bytes(a)
    (tmp_path / f"zeroskip-{UUIDSTR}-5-8").write_bytes(b)
    _dotzsdb(tmp_path, 9)
    rep = repack.repack_dir(str(tmp_path))
    out = tmp_path / f"zeroskip-{UUIDSTR}-2-8"
    assert rep["branch"] == 2 and rep["files_merged"] == 2 and rep["path"] == str(out), rep
    assert open(out, "rb").read() == zf.packed_file(zf.repack_packed(a, b), UUID, 2, 8), seed
