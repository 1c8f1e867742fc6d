"""Repack output on the GPU: packed zeroskip files written through
libzscrc's packed-file writer (include/zscrc.h, zscrc_pack_*).

The writer mirrors the reference's repack output path
(zs_packed_file_new_from_memtree, src/zeroskip-packed.c:384-473, and
zs_packed_file_new_from_packed_files, :617-742): header, records in key order,
records-region commit, pointer section, final commit.  Every byte of the
records region and of the pointer section is checksummed on the GPU while the
host writes the file.  ``repack_dir`` runs zsdb_repack (src/zeroskip.c:
1419-1571) over a DB directory in ONE call into the library
(zscrc_zs_repack, zeroskip_amd/csrc/zscrc_repack.cpp): record listing, the
key merge (finalised files, or the reference's two packed files), the
writer, the unlinks and the .zsdb rewrite are all C++.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._lib import check, lib

FSYNC = 1  # ZSCRC_PACK_FSYNC


class PackReport(ctypes.Structure):
    _fields_ = [("records", ctypes.c_uint64), ("region_bytes", ctypes.c_uint64),
                ("file_bytes", ctypes.c_uint64), ("region_crc", ctypes.c_uint32),
                ("pointers_crc", ctypes.c_uint32), ("commit_crc", ctypes.c_uint32),
                ("final_crc", ctypes.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Packer:
    """with Packer(path, uuid, startidx, endidx) as p: p.add(key, value); ...
    Keys must be added in key order; value None writes a delete record."""

    def __init__(self, path: str, uuid: bytes, startidx: int = 0, endidx: int = 0,
                 chunk_bytes: int = 0, fsync: bool = False):
        assert len(uuid) == 16
        self._h = ctypes.c_void_p()
        check(lib().zscrc_pack_open(ctypes.byref(self._h), os.fsencode(path), bytes(uuid), startidx, endidx,
                                    chunk_bytes, FSYNC if fsync else 0), "zscrc_pack_open")
        self.report: dict | None = None

    def add(self, key, value=None) -> None:
        k = np.frombuffer(key, dtype=np.uint8) if isinstance(key, (bytes, bytearray, memoryview)) else key
        if value is None:
            check(lib().zscrc_pack_add(self._h, k.ctypes.data, k.nbytes, None, 0), "zscrc_pack_add")
            return
        v = np.frombuffer(value, dtype=np.uint8) if isinstance(value, (bytes, bytearray, memoryview)) else value
        # a zero-length value still needs a non-NULL pointer (NULL = delete)
        vp = v.ctypes.data if v.nbytes else ctypes.addressof(_EMPTY)
        check(lib().zscrc_pack_add(self._h, k.ctypes.data, k.nbytes, vp, v.nbytes), "zscrc_pack_add")

    def add_many(self, records) -> None:
        """(key, value-or-None) pairs in key order, one library call
        (zscrc_pack_add_batch): keys and values packed into two blobs."""
        records = list(records)
        if not records:
            return
        klen = np.fromiter((len(k) for k, _ in records), dtype=np.uint64, count=len(records))
        koff = np.zeros(len(records), dtype=np.uint64)
        np.cumsum(klen[:-1], out=koff[1:])
        kblob = np.frombuffer(b"".join(k for k, _ in records) or b"\0", dtype=np.uint8)
        vlen = np.fromiter((0 if v is None else len(v) for _, v in records), dtype=np.uint64, count=len(records))
        voff = np.zeros(len(records), dtype=np.uint64)
        np.cumsum(vlen[:-1], out=voff[1:])
        voff[[i for i, (_, v) in enumerate(records) if v is None]] = ~np.uint64(0)
        vblob = np.frombuffer(b"".join(v for _, v in records if v is not None) or b"\0", dtype=np.uint8)
        self.add_arrays(kblob, koff, klen, vblob, voff, vlen)

    def add_arrays(self, kblob, koff, klen, vblob, voff, vlen) -> None:
        """Records i = kblob[koff[i]:+klen[i]] -> vblob[voff[i]:+vlen[i]]
        (voff[i] == 2**64-1: a delete; vblob None: all deletes), numpy arrays,
        no copies (values may share bytes)."""
        n = len(koff)
        koff, klen = np.ascontiguousarray(koff, np.uint64), np.ascontiguousarray(klen, np.uint64)
        kblob = np.ascontiguousarray(kblob).view(np.uint8)
        assert len(klen) == n and (n == 0 or int((koff + klen).max()) <= kblob.nbytes)
        vp = op = lp = None
        if vblob is not None:
            vblob = np.ascontiguousarray(vblob).view(np.uint8)
            voff, vlen = np.ascontiguousarray(voff, np.uint64), np.ascontiguousarray(vlen, np.uint64)
            live = voff != ~np.uint64(0)
            assert len(voff) == n and len(vlen) == n
            assert not live.any() or int((voff[live] + vlen[live]).max()) <= vblob.nbytes
            vp, op, lp = vblob.ctypes.data, voff.ctypes.data, vlen.ctypes.data
        check(lib().zscrc_pack_add_batch(self._h, kblob.ctypes.data, koff.ctypes.data, klen.ctypes.data,
                                         vp, op, lp, n), "zscrc_pack_add_batch")

    def close(self) -> dict:
        if self._h:
            rep = PackReport()
            h, self._h = self._h, ctypes.c_void_p()
            check(lib().zscrc_pack_close(h, ctypes.byref(rep)), "zscrc_pack_close")
            self.report = rep.as_dict()
        return self.report

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            self.close()
        elif self._h:
            # an exception mid-packing: no commits, the partial file removed
            h, self._h = self._h, ctypes.c_void_p()
            lib().zscrc_pack_abort(h)


_EMPTY = ctypes.c_uint8(0)


class RepackReport(ctypes.Structure):
    """zscrc_repack_report (include/zscrc.h)."""
    _fields_ = [("branch", ctypes.c_int32), ("startidx", ctypes.c_uint32), ("endidx", ctypes.c_uint32),
                ("files_merged", ctypes.c_uint64), ("records_in", ctypes.c_uint64),
                ("records_out", ctypes.c_uint64), ("dotzsdb_crc", ctypes.c_uint32), ("pack", PackReport),
                ("list_s", ctypes.c_double), ("merge_s", ctypes.c_double), ("write_s", ctypes.c_double),
                ("total_s", ctypes.c_double), ("path", ctypes.c_char * 4096)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("pack", "path")}
        d["pack"] = self.pack.as_dict()
        d["path"] = self.path.decode()
        return d


REFERENCE_COMPAT = 2  # ZSCRC_REPACK_REFERENCE_COMPAT


def repack_dir(dbdir: str, threads: int = 0, fsync: bool = False, reference_compat: bool = False) -> dict:
    """zsdb_repack over a DB directory (zscrc_zs_repack): branch 1 merges the
    finalised files, branch 2 the reference's two packed files; returns the
    report (branch 0: nothing to pack).  reference_compat: branch 2 writes the
    reference's bytes including its loss of records after a delete
    (src/zeroskip-iterator.c:258-259; include/zscrc.h)."""
    rep = RepackReport()
    flags = (FSYNC if fsync else 0) | (REFERENCE_COMPAT if reference_compat else 0)
    check(lib().zscrc_zs_repack(os.fsencode(dbdir), flags, threads, ctypes.byref(rep)), "zscrc_zs_repack")
    return rep.as_dict()


class PackOpts(ctypes.Structure):
    """zscrc_pack_opts (include/zscrc.h); 0 = the default."""
    _fields_ = [("tile_bytes", ctypes.c_uint64)]


PACK_RES_WORDS = 8  # ZSCRC_PACK_RES_WORDS
PACK_OVERFLOW = 3  # ZSCRC_ZS_OVERFLOW in res[0]


def device_pack_bound(n: int, sum_key_len: int, sum_val_len: int) -> int:
    """An upper bound on the packed file's size from the record lister's
    res[1], res[4], res[5] (zscrc_device_pack_bound); 0 if it wraps."""
    return lib().zscrc_device_pack_bound(n, sum_key_len, sum_val_len)


def device_pack_scratch_bytes(n: int, tile_bytes: int = 0) -> int:
    """zscrc_device_pack_scratch_bytes; 0 = a bad option."""
    return lib().zscrc_device_pack_scratch_bytes(n, ctypes.byref(PackOpts(tile_bytes)))


def device_pack(d_src, recs, uuid: bytes, startidx: int = 0, endidx: int = 0, out=None, tile_bytes: int = 0,
                scratch=None):
    """The packed file of a device-resident record list, written on the GPU
    (zscrc_device_pack): (image, res).  d_src: the uint8 device tensor the
    records' offsets point into; recs: an int64 [n, 4] device tensor (key_off,
    key_len, val_off or -1 for a delete, val_len) such as
    zsfile.device_records returns, sliced to its count; records are written in
    the order given.  res: int64 device tensor [code (0 written, 3 the file
    does not fit `out`, -1 a record outside d_src), n or the first bad index,
    file_bytes, region_bytes, region_crc, pointers_crc, commit_crc, final_crc].
    out=None: a sizing call, one read of res[2] (the wrapper's only
    synchronisation) and an output of exactly that size; image is None when a
    record is bad.  out given (a 16-byte aligned uint8 device tensor): one
    asynchronous call on the current stream, image = out (file_bytes of it are
    the file when res[0] == 0).  scratch: a 16-byte aligned uint8 tensor of
    device_pack_scratch_bytes(n) bytes (default: the library's own)."""
    import torch

    assert len(uuid) == 16
    dev = d_src.device
    n = int(recs.shape[0])
    assert recs.dtype == torch.int64 and recs.is_contiguous() and (n == 0 or recs.shape[1] == 4)
    res = torch.empty(PACK_RES_WORDS, dtype=torch.int64, device=dev)
    opts = PackOpts(tile_bytes)
    src_bytes = d_src.numel() * d_src.element_size()

    def call(o):
        cap = 0 if o is None else o.numel() * o.element_size()
        with torch.cuda.device(dev):
            check(lib().zscrc_device_pack(
                d_src.data_ptr() if src_bytes else None, src_bytes, recs.data_ptr() if n else None, n, bytes(uuid),
                startidx, endidx, o.data_ptr() if cap else None, cap, res.data_ptr(),
                None if scratch is None else scratch.data_ptr(), ctypes.byref(opts), 0,
                torch.cuda.current_stream(dev).cuda_stream), "zscrc_device_pack")

    if out is not None:
        call(out)
        return out, res
    call(None)
    code, _, file_bytes = (int(v) for v in res[:3].cpu())
    if code != PACK_OVERFLOW:
        return None, res
    out = torch.empty(file_bytes, dtype=torch.uint8, device=dev)
    call(out)
    return out, res


class MergeList(ctypes.Structure):
    """zscrc_merge_list (include/zscrc.h)."""
    _fields_ = [("d_recs", ctypes.c_void_p), ("n", ctypes.c_uint64), ("base", ctypes.c_uint64)]


class MergeOpts(ctypes.Structure):
    """zscrc_merge_opts (include/zscrc.h); 0 = the default."""
    _fields_ = [("tile_records", ctypes.c_uint32)]


MERGE_RES_WORDS = 8  # ZSCRC_MERGE_RES_WORDS
MERGE_DROP_DELETES = 1  # ZSCRC_MERGE_DROP_DELETES


def device_merge_scratch_bytes(n_total: int, tile_records: int = 0) -> int:
    """zscrc_device_merge_scratch_bytes; 0 = a bad option or too many records."""
    return lib().zscrc_device_merge_scratch_bytes(n_total, ctypes.byref(MergeOpts(tile_records)))


def device_merge(d_src, lists, drop_deletes: bool = False, out=None, tile_records: int = 0, scratch=None):
    """Device-resident record lists merged by key on the GPU
    (zscrc_device_merge): (recs, res).  d_src: the uint8 device tensor the
    rebased offsets point into; lists: a sequence of (recs, base), recs an
    int64 [n, 4] device tensor such as zsfile.device_records returns, sliced
    to its count, base added to its offsets.  A later record of a key wins
    (later in its list, or in a later list); drop_deletes: a winning delete is
    dropped instead of kept.  recs: the winners in key order, rebased, a list
    device_pack takes over the same d_src.  res: int64 device tensor [code (0,
    3 more winners than `out` holds, -1 a record outside d_src), winners or
    the first bad sequence number, records in, deletes kept, sum of key
    lengths, sum of value lengths, records superseded, deletes dropped].
    out=None: a sizing call, one read of res[1] (the wrapper's only
    synchronisation) and an output of exactly that size; recs is None when a
    record is bad.  out given (an int64 [cap, 4] device tensor): one
    asynchronous call on the current stream, recs = out (res[1] rows of it
    are the list when res[0] == 0).  scratch: a 16-byte aligned uint8 tensor
    of device_merge_scratch_bytes(n_total) bytes (default: the library's own)."""
    import torch

    dev = d_src.device
    lists = list(lists)
    arr = (MergeList * max(len(lists), 1))()
    for j, (recs, base) in enumerate(lists):
        n = int(recs.shape[0])
        assert recs.dtype == torch.int64 and recs.is_contiguous() and (n == 0 or recs.shape[1] == 4)
        arr[j].d_recs, arr[j].n, arr[j].base = (recs.data_ptr() if n else None), n, base
    res = torch.empty(MERGE_RES_WORDS, dtype=torch.int64, device=dev)
    opts = MergeOpts(tile_records)
    src_bytes = d_src.numel() * d_src.element_size()

    def call(o):
        cap = 0 if o is None else o.numel() // 4
        with torch.cuda.device(dev):
            check(lib().zscrc_device_merge(
                d_src.data_ptr() if src_bytes else None, src_bytes, arr, len(lists),
                o.data_ptr() if cap else None, cap, res.data_ptr(),
                None if scratch is None else scratch.data_ptr(), ctypes.byref(opts),
                MERGE_DROP_DELETES if drop_deletes else 0, torch.cuda.current_stream(dev).cuda_stream),
                "zscrc_device_merge")

    if out is not None:
        call(out)
        return out, res
    call(None)
    code, n_out = (int(v) for v in res[:2].cpu())
    if code < 0:
        return None, res
    out = torch.empty((n_out, 4), dtype=torch.int64, device=dev)
    if n_out:
        call(out)
    return out, res


def device_repack(d_arena, images, kinds, uuid: bytes, startidx: int, endidx: int, drop_deletes: bool):
    """A repack of device-resident file images without an image byte or a key
    crossing PCIe: the record lists (one zsfile.device_records_multi call
    when every image is active or finalised, else zsfile.device_records per
    image), device_merge, device_pack -> (file, report).  images: (offset, size) pairs into the
    uint8 device tensor d_arena in load order (branch 1 of zsdb_repack: the
    finalised files oldest first, drop_deletes False; branch 2: the newer
    packed file first and the older last, drop_deletes True); kinds: each
    image's zsfile kind.  file: the packed file as a uint8 device tensor.
    report: records_in, records_out, superseded, deletes_dropped, file_bytes
    and pack (device_pack's result words as a list).  The host reads the
    lister's totals (per image: its record count, only where a packed file is
    among them), the winners' count and the file's size."""
    from . import zsfile

    images, kinds = list(images), list(kinds)
    lists = []
    if images and all(kind in (zsfile.ACTIVE, zsfile.FINALISED) for kind in kinds):
        # every image has a chain: one call lists them all as one list over the arena
        recs, rows, tot = zsfile.device_records_multi(d_arena, images)
        t = [int(v) for v in tot.cpu()]
        if t[7]:
            for (off, _), row in zip(images, rows[:, 0].cpu().tolist()):
                if row != zsfile.END:
                    raise ValueError("image at %d does not list: code %d" % (off, row))
        lists.append((recs[:t[1]], 0))
    else:
        for (off, size), kind in zip(images, kinds):
            recs, res = zsfile.device_records(d_arena[off:off + size], kind)
            code, n = (int(v) for v in res[:2].cpu())
            if code not in (0, zsfile.END):
                raise ValueError("image at %d does not list: code %d" % (off, code))
            lists.append((recs[:n], off))
    import torch

    # room for every record in: one merge, no sizing call
    n_in = sum(int(r.shape[0]) for r, _ in lists)
    merged, mres = device_merge(d_arena, lists, drop_deletes=drop_deletes,
                                out=torch.empty((n_in, 4), dtype=torch.int64, device=d_arena.device))
    m = [int(v) for v in mres.cpu()]
    if m[0] != 0:
        raise ValueError("record %d lies outside the arena" % m[1])
    image, pres = device_pack(d_arena, merged[:m[1]], uuid, startidx, endidx)
    p = [int(v) for v in pres.cpu()]
    if image is None:
        raise ValueError("record %d lies outside the arena" % p[1])
    return image, {"records_in": m[2], "records_out": m[1], "superseded": m[6], "deletes_dropped": m[7],
                   "file_bytes": p[2], "pack": p}


def records(image, kind: int):
    """(key_off, key_len, val_off, val_len) uint64 arrays of a file image's
    records (zscrc_zs_records); val_off == 2**64-1 marks a delete."""
    a = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray))
                             else image)
    cap = a.nbytes // 32 + 16
    while True:
        out = np.empty((cap, 4), np.uint64)
        n = ctypes.c_size_t()
        rc = lib().zscrc_zs_records(a.ctypes.data, a.nbytes, kind, out.ctypes.data, cap, ctypes.byref(n))
        if rc == 3:                              # ZSCRC_ZS_OVERFLOW
            cap = n.value
            continue
        if rc < 0:
            check(rc, "zscrc_zs_records")
        return out[:n.value].T.copy(), rc
