"""zeroskip file images: walk, span descriptors and GPU commit verification.

Python view of include/zscrc.h Part 3 (zeroskip_amd/csrc/zscrc_zs.cpp).  The
walk follows the reference (src/zeroskip-record.c:283-331); each commit's CRC
(span + host-order trailer words, src/zeroskip-file.c:253-350) is recomputed
and compared on the GPU.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._lib import LEN_UNBOUNDED, check, lib

END, STOPPED, TRUNCATED, OVERFLOW, BADSIG = 0, 1, 2, 3, 4
ACTIVE, FINALISED, PACKED = 0, 1, 2


class Report(ctypes.Structure):
    _fields_ = [("header_rc", ctypes.c_int), ("header_stored", ctypes.c_uint32),
                ("header_computed", ctypes.c_uint32), ("walk_rc", ctypes.c_int),
                ("end_off", ctypes.c_uint64), ("n_commits", ctypes.c_uint64),
                ("n_bad", ctypes.c_uint64), ("first_bad", ctypes.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _host(image):
    a = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray, memoryview)) else image)
    return a, a.ctypes.data, a.nbytes


def walk(image):
    """(span_off, span_len, rc, end_off) of every commit of an active or
    finalised file image."""
    a, p, n = _host(image)
    cap = n // 8 + 1
    off = np.empty(cap, np.uint64)
    ln = np.empty(cap, np.uint64)
    nc = ctypes.c_size_t()
    end = ctypes.c_uint64()
    rc = lib().zscrc_zs_walk(p, n, off.ctypes.data, ln.ctypes.data, cap, ctypes.byref(nc),
                             ctypes.byref(end))
    if rc < 0:
        check(rc, "zscrc_zs_walk")
    return off[:nc.value], ln[:nc.value], rc, end.value


def packed_spans(image):
    a, p, n = _host(image)
    off = np.empty(2, np.uint64)
    ln = np.empty(2, np.uint64)
    rc = lib().zscrc_zs_packed_spans(p, n, off.ctypes.data, ln.ctypes.data)
    return off, ln, rc


def header_crc(image):
    a, p, n = _host(image)
    st, cp = ctypes.c_uint32(), ctypes.c_uint32()
    rc = lib().zscrc_zs_header_crc(p, n, ctypes.byref(st), ctypes.byref(cp))
    return rc, st.value, cp.value


def dotzsdb_crc(image):
    a, p, n = _host(image)
    st, cp = ctypes.c_uint32(), ctypes.c_uint32()
    rc = lib().zscrc_zs_dotzsdb_crc(p, n, ctypes.byref(st), ctypes.byref(cp))
    return rc, st.value, cp.value


def verify_image(image, kind: int = ACTIVE) -> dict:
    """Header on the CPU, every commit on the current GPU (synchronous)."""
    a, p, n = _host(image)
    rep = Report()
    check(lib().zscrc_zs_verify_image(p, n, kind, ctypes.byref(rep)), "zscrc_zs_verify_image")
    return rep.as_dict()


class WalkOpts(ctypes.Structure):
    """zscrc_walk_opts (include/zscrc.h)."""
    _fields_ = [("block_bytes", ctypes.c_uint64), ("tile_bytes", ctypes.c_uint64)]


WALK_SERIAL = 1  # ZSCRC_WALK_SERIAL
WALK_RES_WORDS = 6  # ZSCRC_WALK_RES_WORDS
WALK_NONE = -1  # res[5] as int64 (UINT64_MAX): no one-lane continuation


def walk_scratch_bytes(size: int, block_bytes: int = 0, tile_bytes: int = 0) -> int:
    """zscrc_device_walk_scratch_bytes; 0 = bad options."""
    return lib().zscrc_device_walk_scratch_bytes(size, ctypes.byref(WalkOpts(block_bytes, tile_bytes)))


def device_walk(d_image: torch.Tensor, cap: int | None = None, block_bytes: int = 0, tile_bytes: int = 0,
                serial: bool = False, out: tuple | None = None, scratch: torch.Tensor | None = None):
    """The walk of a device-resident image on the GPU (zscrc_device_walk),
    asynchronous on the current stream: (span_off, span_len, res) int64 device
    tensors -- `cap` entries each (default size // 8 + 1, the most an image
    can hold) of which the first min(res[1], cap) are written, and res =
    [result code, commits, end_off, longest span, shortest span, offset the
    one-lane walk took over at or -1].  Equal to walk() of the same bytes.
    out: preallocated (span_off, span_len, res) to write into; scratch: a
    16-byte aligned uint8 tensor of walk_scratch_bytes() bytes (default: the
    library's own, stream-ordered)."""
    size = d_image.numel() * d_image.element_size()
    dev = d_image.device
    if cap is None:
        cap = size // 8 + 1
    if out is None:
        out = (torch.empty(max(cap, 1), dtype=torch.int64, device=dev),
               torch.empty(max(cap, 1), dtype=torch.int64, device=dev),
               torch.empty(WALK_RES_WORDS, dtype=torch.int64, device=dev))
    off, ln, res = out
    assert off.numel() >= cap and ln.numel() >= cap and res.numel() >= WALK_RES_WORDS
    opts = WalkOpts(block_bytes, tile_bytes)
    with torch.cuda.device(dev):
        check(lib().zscrc_device_walk(
            d_image.data_ptr(), size, off.data_ptr(), ln.data_ptr(), cap, res.data_ptr(),
            None if scratch is None else scratch.data_ptr(), ctypes.byref(opts), WALK_SERIAL if serial else 0,
            torch.cuda.current_stream(dev).cuda_stream), "zscrc_device_walk")
    return off, ln, res


def verify_device_image(d_image: torch.Tensor, kind: int = ACTIVE) -> dict:
    """verify_image() for a device-resident image (zscrc_device_verify_image):
    the walk and every commit CRC on the GPU, only the header (and a packed
    file's few locating words) copied to the host.  Synchronous."""
    size = d_image.numel() * d_image.element_size()
    rep = Report()
    with torch.cuda.device(d_image.device):
        check(lib().zscrc_device_verify_image(d_image.data_ptr(), size, kind, ctypes.byref(rep),
                                              torch.cuda.current_stream(d_image.device).cuda_stream),
              "zscrc_device_verify_image")
    return rep.as_dict()


RECORDS_RES_WORDS = 12  # ZSCRC_RECORDS_RES_WORDS
DELETED = -1  # val_off of a delete record as int64 (ZSCRC_ZS_DELETED, UINT64_MAX)


def records_scratch_bytes(size: int, kind: int = ACTIVE, block_bytes: int = 0, tile_bytes: int = 0) -> int:
    """zscrc_device_records_scratch_bytes; 0 = bad options or kind."""
    return lib().zscrc_device_records_scratch_bytes(size, kind, ctypes.byref(WalkOpts(block_bytes, tile_bytes)))


def device_records(d_image: torch.Tensor, kind: int = ACTIVE, cap: int | None = None, block_bytes: int = 0,
                   tile_bytes: int = 0, serial: bool = False, out: tuple | None = None,
                   scratch: torch.Tensor | None = None):
    """The key / value and delete records of a device-resident image, listed
    on the GPU (zscrc_device_records), asynchronous on the current stream:
    (recs, res) int64 device tensors.  recs is [cap, 4] -- key_off, key_len,
    val_off (DELETED for a delete record), val_len -- of which the first
    min(res[1], cap) rows are written; the default cap is size // 24 + 1, the
    most an image can hold (no record is shorter than 24 bytes).  res =
    [result code, records, end offset (packed: the pointer section's offset),
    deletes, sum of key lengths, sum of value lengths, longest key, longest
    value, offset a one-lane loop took over at or -1, 0, 0, 0].  Equal to
    repack.records() of the same bytes.  out: preallocated (recs, res) to
    write into; scratch: a 16-byte aligned uint8 tensor of
    records_scratch_bytes() bytes (default: the library's own, stream-ordered)."""
    size = d_image.numel() * d_image.element_size()
    dev = d_image.device
    if cap is None:
        cap = size // 24 + 1
    if out is None:
        out = (torch.empty((max(cap, 1), 4), dtype=torch.int64, device=dev),
               torch.empty(RECORDS_RES_WORDS, dtype=torch.int64, device=dev))
    recs, res = out
    assert recs.numel() >= 4 * cap and res.numel() >= RECORDS_RES_WORDS
    opts = WalkOpts(block_bytes, tile_bytes)
    with torch.cuda.device(dev):
        check(lib().zscrc_device_records(
            d_image.data_ptr(), size, kind, recs.data_ptr() if recs.numel() else None, cap, res.data_ptr(),
            None if scratch is None else scratch.data_ptr(), ctypes.byref(opts), WALK_SERIAL if serial else 0,
            torch.cuda.current_stream(dev).cuda_stream), "zscrc_device_records")
    return recs, res


class LogOpts(ctypes.Structure):
    """zscrc_log_opts (include/zscrc.h); 0 = the default."""
    _fields_ = [("tile_bytes", ctypes.c_uint64), ("prev_crc", ctypes.c_uint32)]


LOG_FINALISE = 1  # ZSCRC_LOG_FINALISE
LOG_RES_WORDS = 8  # ZSCRC_LOG_RES_WORDS
_LOG_NAMES = ("code", "n", "end", "written", "commits", "long_commits", "last_crc", "stored_crc")


def device_log_bound(n: int, n_commits: int, sum_key_len: int, sum_val_len: int) -> int:
    """An upper bound on the end offset of a log written from its header
    (zscrc_device_log_bound): 40 + 54 n + 24 n_commits + the sums; 0 if it wraps."""
    return lib().zscrc_device_log_bound(n, n_commits, sum_key_len, sum_val_len)


def device_log_scratch_bytes(n: int, n_tx: int, tile_bytes: int = 0) -> int:
    """zscrc_device_log_scratch_bytes (one transaction a record: n_tx = n); 0 = a
    bad option or a count above the limit."""
    return lib().zscrc_device_log_scratch_bytes(n, n_tx, ctypes.byref(LogOpts(tile_bytes, 0)))


def _log_result(res, image, new_recs, span_off, span_len) -> dict:
    """The result words by name (res: uint64 host words) around the outputs."""
    d = {k: int(v) for k, v in zip(_LOG_NAMES, res)}
    d["code"] = int(np.int64(res[0]))
    if d["code"] == -1:  # bad input: [1] the first bad record, [2] the first bad table entry, or -1
        d["bad_record"], d["bad_tx"] = int(np.int64(res[1])), int(np.int64(res[2]))
        d["n"] = d["end"] = 0
    ok = d["code"] == 0
    nc = d["commits"] if ok else 0
    d["image"] = image[:d["end"]] if ok and image is not None else None
    d["new_recs"] = new_recs if ok else None
    d["span_off"] = span_off[:nc] if ok and span_off is not None else None
    d["span_len"] = span_len[:nc] if ok and span_len is not None else None
    return d


def device_log(d_src: torch.Tensor, recs: torch.Tensor, tx_end: torch.Tensor | None = None, uuid: bytes = bytes(16),
               startidx: int = 0, endidx: int = 0, out: torch.Tensor | None = None, at: int = 0, finalise: bool = False,
               prev_crc: int = 0, tile_bytes: int = 0, new_recs: bool = False, spans: bool = False,
               scratch: torch.Tensor | None = None) -> dict:
    """A batch of puts and deletes appended to an active log image on the GPU
    (zscrc_device_log): what zsdb_add / zsdb_remove / zsdb_commit write, commit
    CRCs included.  d_src: the uint8 device tensor the records' offsets point
    into; recs: int64 [n, 4] device tensor (key_off, key_len, val_off or DELETED,
    val_len); tx_end: int64 device tensor of exclusive transaction ends
    (non-decreasing, the last one n; an empty tensor = no transaction), None =
    one transaction a record.  at = 0: a new image, header from uuid, startidx,
    endidx; at >= 40 (a multiple of 8): appended at that offset of `out`.
    finalise: the stale-register finalise commit behind the last transaction
    (hashed from prev_crc where the call has no transaction).  out: a 16-byte
    aligned uint8 device tensor, the image's base; None: one of at +
    device_log_bound() bytes from the torch sums of the lengths (one more
    read-back).  Returns a dict: image (out cut to the end offset; None unless
    code == 0), res (the int64 device words) and its words by name -- code (0
    written, 3 does not fit out, -1 bad input: then bad_record / bad_tx, -1 =
    none), n, end, written, commits, long_commits, last_crc (what a later call
    passes as prev_crc), stored_crc -- read back once, as device_pack reads its
    size; new_recs ([n, 4], what device_records lists for the written bytes) and
    span_off / span_len (one per commit: verify_commits' input) when asked for.
    scratch: a 16-byte aligned uint8 tensor of device_log_scratch_bytes() bytes
    (default: the library's own, stream-ordered)."""
    dev = d_src.device
    n = int(recs.shape[0])
    assert recs.dtype == torch.int64 and recs.is_contiguous() and (n == 0 or recs.shape[1] == 4)
    assert at != 0 or len(uuid) == 16
    n_tx = 0 if tx_end is None else int(tx_end.numel())
    assert tx_end is None or (tx_end.dtype == torch.int64 and tx_end.is_contiguous())
    nc = (n if tx_end is None else n_tx) + (1 if finalise else 0)
    if out is None:
        # a delete's val_len is ignored by the writer
        vlen = torch.where(recs[:, 2] == DELETED, 0, recs[:, 3]) if n else None
        sums = torch.stack((recs[:, 1].sum(), vlen.sum())).cpu() if n else (0, 0)
        bound = device_log_bound(n, nc, int(sums[0]) & (2**64 - 1), int(sums[1]) & (2**64 - 1))
        assert bound, "the size bound wraps"
        out = torch.empty(bound + (at - 40 if at else 0), dtype=torch.uint8, device=dev)
    cap = out.numel() * out.element_size()
    res = torch.empty(LOG_RES_WORDS, dtype=torch.int64, device=dev)
    nr = torch.empty((max(n, 1), 4), dtype=torch.int64, device=dev) if new_recs else None
    so = torch.empty(max(nc, 1), dtype=torch.int64, device=dev) if spans else None
    sl = torch.empty(max(nc, 1), dtype=torch.int64, device=dev) if spans else None
    src_bytes = d_src.numel() * d_src.element_size()
    opts = LogOpts(tile_bytes, prev_crc)
    with torch.cuda.device(dev):
        check(lib().zscrc_device_log(
            d_src.data_ptr() if src_bytes else None, src_bytes, recs.data_ptr() if n else None, n,
            None if tx_end is None else (tx_end.data_ptr() if n_tx else res.data_ptr()), n_tx,
            bytes(uuid), startidx, endidx, out.data_ptr() if cap else None, cap, at,
            None if nr is None else nr.data_ptr(), None if so is None else so.data_ptr(),
            None if sl is None else sl.data_ptr(), res.data_ptr(),
            None if scratch is None else scratch.data_ptr(), ctypes.byref(opts), LOG_FINALISE if finalise else 0,
            torch.cuda.current_stream(dev).cuda_stream), "zscrc_device_log")
    d = _log_result(res.cpu().numpy().view(np.uint64), out, None if nr is None else nr[:n], so, sl)
    d["res"] = res
    return d


def log(src, recs, tx_end=None, uuid: bytes = bytes(16), startidx: int = 0, endidx: int = 0, out=None, at: int = 0,
        finalise: bool = False, prev_crc: int = 0, tile_bytes: int = 0, new_recs: bool = False,
        spans: bool = False) -> dict:
    """device_log in host memory (zscrc_zs_log, one thread, no device): the same
    image, words and optional outputs as numpy arrays for the same bytes.  src:
    bytes or a uint8 array; recs [n, 4] uint64 or int64; tx_end: a sequence of
    exclusive ends or None; out: a writable uint8 array (the image's base) or
    None for one of at + device_log_bound() bytes."""
    s, sp, sn = _host(src)
    r = np.ascontiguousarray(recs).view(np.uint64).reshape(-1, 4)
    n = len(r)
    te = None if tx_end is None else np.ascontiguousarray(tx_end, dtype=np.uint64).reshape(-1)
    n_tx = 0 if te is None else len(te)
    nc = (n if te is None else n_tx) + (1 if finalise else 0)
    if out is None:
        with np.errstate(over="ignore"):
            vlen = np.where(r[:, 2] == np.uint64(2**64 - 1), np.uint64(0), r[:, 3])  # a delete's is ignored
            bound = device_log_bound(n, nc, int(r[:, 1].sum(dtype=np.uint64)), int(vlen.sum(dtype=np.uint64)))
        assert bound, "the size bound wraps"
        out = np.zeros(bound + (at - 40 if at else 0), np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable
    res = np.zeros(LOG_RES_WORDS, np.uint64)
    nr = np.zeros((max(n, 1), 4), np.uint64) if new_recs else None
    so = np.zeros(max(nc, 1), np.uint64) if spans else None
    sl = np.zeros(max(nc, 1), np.uint64) if spans else None
    opts = LogOpts(tile_bytes, prev_crc)
    check(lib().zscrc_zs_log(sp if sn else None, sn, r.ctypes.data if n else None, n,
                             None if te is None else (te.ctypes.data if n_tx else res.ctypes.data), n_tx,
                             bytes(uuid), startidx, endidx, out.ctypes.data if out.nbytes else None, out.nbytes, at,
                             None if nr is None else nr.ctypes.data, None if so is None else so.ctypes.data,
                             None if sl is None else sl.ctypes.data, res.ctypes.data, ctypes.byref(opts),
                             LOG_FINALISE if finalise else 0), "zscrc_zs_log")
    d = _log_result(res, out, None if nr is None else nr[:n], so, sl)
    d["res"] = res
    return d


class WalkImage(ctypes.Structure):
    """zscrc_walk_image (include/zscrc.h): bytes [off, off + size) of an arena."""
    _fields_ = [("off", ctypes.c_uint64), ("size", ctypes.c_uint64)]


WALK_ROW_WORDS = 8  # ZSCRC_WALK_ROW_WORDS
WALK_TOT_WORDS = 4  # ZSCRC_WALK_TOT_WORDS
WALK_MULTI_MAX = 1 << 20  # ZSCRC_WALK_MULTI_MAX


def _walk_images(images):
    """[(off, size)] as a zscrc_walk_image array (one entry's room for none)."""
    images = list(images)
    arr = (WalkImage * max(len(images), 1))()
    for j, (off, size) in enumerate(images):
        arr[j].off, arr[j].size = off, size
    return arr, len(images)


def walk_multi_scratch_bytes(images, block_bytes: int = 0, tile_bytes: int = 0) -> int:
    """zscrc_device_walk_multi_scratch_bytes for images = [(off, size)];
    0 = bad arguments."""
    arr, k = _walk_images(images)
    return lib().zscrc_device_walk_multi_scratch_bytes(arr, k, ctypes.byref(WalkOpts(block_bytes, tile_bytes)))


def device_walk_multi(d_arena: torch.Tensor, images, cap: int | None = None, block_bytes: int = 0,
                      tile_bytes: int = 0, out: tuple | None = None, scratch: torch.Tensor | None = None):
    """The walk of the k images [(off, size)] of a device-resident arena in
    one call (zscrc_device_walk_multi), asynchronous on the current stream:
    (span_off, span_len, span_img, rows, tot) device tensors -- int64, int64,
    int32 of `cap` entries each (default sum of size // 8 + 1), of which the
    first min(tot[1], cap) are written: image 0's commits, then image 1's
    ..., span_off as offsets into the arena; rows int64 (k, 8): [result code,
    commits, end_off, longest span, shortest span, offset the one-lane walk
    took over at or -1, index of the image's first span, 0], image-relative;
    tot int64: [OVERFLOW or 0, commits of all images, longest span, shortest
    span].  Each image's part equals walk() of its bytes.
    out: preallocated (span_off, span_len, span_img, rows, tot); scratch: a
    16-byte aligned uint8 tensor of walk_multi_scratch_bytes() bytes (default:
    the library's own, stream-ordered)."""
    size = d_arena.numel() * d_arena.element_size()
    dev = d_arena.device
    arr, k = _walk_images(images)
    if cap is None:
        cap = sum(arr[j].size // 8 + 1 for j in range(k))
    if out is None:
        out = (torch.empty(max(cap, 1), dtype=torch.int64, device=dev),
               torch.empty(max(cap, 1), dtype=torch.int64, device=dev),
               torch.empty(max(cap, 1), dtype=torch.int32, device=dev),
               torch.empty((max(k, 1), WALK_ROW_WORDS), dtype=torch.int64, device=dev),
               torch.empty(WALK_TOT_WORDS, dtype=torch.int64, device=dev))
    off, ln, img, rows, tot = out
    assert off.numel() >= cap and ln.numel() >= cap and img.numel() >= cap
    assert rows.numel() >= k * WALK_ROW_WORDS and tot.numel() >= WALK_TOT_WORDS
    opts = WalkOpts(block_bytes, tile_bytes)
    with torch.cuda.device(dev):
        check(lib().zscrc_device_walk_multi(
            d_arena.data_ptr(), size, arr, k, off.data_ptr() or None, ln.data_ptr() or None, img.data_ptr() or None,
            cap, rows.data_ptr(), tot.data_ptr(), None if scratch is None else scratch.data_ptr(),
            ctypes.byref(opts), 0, torch.cuda.current_stream(dev).cuda_stream), "zscrc_device_walk_multi")
    return off, ln, img, rows, tot


RECORDS_ROW_WORDS = 12  # ZSCRC_RECORDS_ROW_WORDS
RECORDS_TOT_WORDS = 8  # ZSCRC_RECORDS_TOT_WORDS


def records_multi_scratch_bytes(images, block_bytes: int = 0, tile_bytes: int = 0) -> int:
    """zscrc_device_records_multi_scratch_bytes for images = [(off, size)];
    0 = bad arguments."""
    arr, k = _walk_images(images)
    return lib().zscrc_device_records_multi_scratch_bytes(arr, k, ctypes.byref(WalkOpts(block_bytes, tile_bytes)))


def device_records_multi(d_arena: torch.Tensor, images, cap: int | None = None, block_bytes: int = 0,
                         tile_bytes: int = 0, out: tuple | None = None, scratch: torch.Tensor | None = None):
    """The records of the k active or finalised images [(off, size)] of a
    device-resident arena, listed in one call (zscrc_device_records_multi),
    asynchronous on the current stream: (recs, rows, tot) int64 device
    tensors.  recs is [cap, 4] (default cap: the sum of size // 24 + 1, what
    device_records takes per image) of which the first min(tot[1], cap) rows
    are written: image 0's records, then image 1's ..., key_off and val_off
    (unless DELETED) as offsets into the arena -- one list with base 0 for
    repack.device_merge, and one repack.device_pack takes as it is.  rows (k,
    12), image-relative: device_records' res of that image alone with
    unlimited room (the code is never OVERFLOW; -1 for an image of fewer than
    40 bytes), [9] the index of its first record in recs.  tot: [OVERFLOW or
    0, records of all images, deletes, sum of key lengths, sum of value
    lengths, longest key, longest value, images whose code is not END].
    out: preallocated (recs, rows, tot); scratch: a 16-byte aligned uint8
    tensor of records_multi_scratch_bytes() bytes (default: the library's
    own, stream-ordered)."""
    size = d_arena.numel() * d_arena.element_size()
    dev = d_arena.device
    arr, k = _walk_images(images)
    if cap is None:
        cap = sum(arr[j].size // 24 + 1 for j in range(k))
    if out is None:
        out = (torch.empty((max(cap, 1), 4), dtype=torch.int64, device=dev),
               torch.empty((max(k, 1), RECORDS_ROW_WORDS), dtype=torch.int64, device=dev),
               torch.empty(RECORDS_TOT_WORDS, dtype=torch.int64, device=dev))
    recs, rows, tot = out
    assert recs.numel() >= 4 * cap
    assert rows.numel() >= k * RECORDS_ROW_WORDS and tot.numel() >= RECORDS_TOT_WORDS
    opts = WalkOpts(block_bytes, tile_bytes)
    with torch.cuda.device(dev):
        check(lib().zscrc_device_records_multi(
            d_arena.data_ptr(), size, arr, k, recs.data_ptr() if recs.numel() else None, cap, rows.data_ptr(),
            tot.data_ptr(), None if scratch is None else scratch.data_ptr(), ctypes.byref(opts), 0,
            torch.cuda.current_stream(dev).cuda_stream), "zscrc_device_records_multi")
    return recs, rows, tot


class FindOpts(ctypes.Structure):
    """zscrc_find_opts (include/zscrc.h); 0 = the default."""
    _fields_ = [("splitters", ctypes.c_uint32)]


FIND_RES_WORDS = 8  # ZSCRC_FIND_RES_WORDS
FIND_NONE = -1  # ZSCRC_FIND_NONE as the int64 a hit row holds
FIND_BAD_QUERY = -2  # ZSCRC_FIND_BAD_QUERY
FIND_CHECK_ORDER = 1  # ZSCRC_FIND_CHECK_ORDER
FIND_LEVELS_MAX = 64  # ZSCRC_FIND_LEVELS_MAX
FIND_DEFAULT_SPLITTERS = 1024  # zscrc_find.hip DEF_SPLITTERS: what splitters = 0 means
FIND_GRID_THREADS = 1024 * 256  # zscrc_find.hip GRID_MAX * WG: the search's persistent grid at its largest


def _find_levels(levels, ptr):
    """[(recs, base)] as a zscrc_merge_list array (one entry's room for none);
    ptr(recs): the address of a list's first record."""
    from .repack import MergeList

    levels = list(levels)
    arr = (MergeList * max(len(levels), 1))()
    for j, (recs, base) in enumerate(levels):
        n = int(recs.shape[0])
        assert recs.ndim == 2 and (n == 0 or recs.shape[1] == 4)
        arr[j].d_recs, arr[j].n, arr[j].base = (ptr(recs) if n else None), n, base
    return arr, len(levels)


def device_find_scratch_bytes(k: int, splitters: int = 0) -> int:
    """zscrc_device_find_scratch_bytes; 0 = a bad option or too many levels."""
    return lib().zscrc_device_find_scratch_bytes(k, ctypes.byref(FindOpts(splitters)))


def device_find(d_src: torch.Tensor, levels, d_qsrc: torch.Tensor, queries: torch.Tensor, check_order: bool = False,
                splitters: int = 0, out: tuple | None = None, scratch: torch.Tensor | None = None):
    """A batch of keys looked up in device-resident sorted record lists on the
    GPU (zscrc_device_find), asynchronous on the current stream: (hits, res)
    int64 device tensors.  d_src: the uint8 device tensor the levels' rebased
    offsets point into; levels: a sequence of (recs, base) in priority order,
    recs an int64 [n, 4] device tensor such as repack.device_merge returns or
    device_records gives for a packed image, sliced to its count, its keys
    strictly ascending; d_qsrc: the uint8 device tensor the queries' keys lie
    in; queries: int64 [nq, 4], of which key_off and key_len are read (a
    record list is a query list).  hits [nq, 4]: level (FIND_NONE: no level
    holds the key, FIND_BAD_QUERY: the key lies outside d_qsrc), location (the
    index in that level; not found: the lower bound in the last level),
    val_off rebased or DELETED (a delete is a hit of the first level that
    holds the key), val_len.  res: [code (0, -1 a level record outside d_src
    or, with check_order, a key not above its predecessor's: no hit written),
    nq or the first offending sequence number, hits with a value, deleted,
    not found, bad queries, sum of the values' lengths, 1 = an order
    offence].  splitters: the records sampled per level into the LDS table, a
    power of two up to 2048, 1 = plain bisection, 0 = the default; the result
    never depends on it.  out: preallocated (hits, res); scratch: a 16-byte
    aligned uint8 tensor of device_find_scratch_bytes(k) bytes (default: the
    library's own, stream-ordered)."""
    dev = d_src.device
    arr, k = _find_levels(levels, lambda r: r.data_ptr())
    for recs, _ in levels:
        assert recs.dtype == torch.int64 and recs.is_contiguous()
    nq = int(queries.shape[0])
    assert queries.dtype == torch.int64 and queries.is_contiguous() and (nq == 0 or queries.shape[1] == 4)
    if out is None:
        out = (torch.empty((nq, 4), dtype=torch.int64, device=dev),
               torch.empty(FIND_RES_WORDS, dtype=torch.int64, device=dev))
    hits, res = out
    assert hits.numel() >= 4 * nq and res.numel() >= FIND_RES_WORDS
    src_bytes = d_src.numel() * d_src.element_size()
    q_bytes = d_qsrc.numel() * d_qsrc.element_size()
    opts = FindOpts(splitters)
    with torch.cuda.device(dev):
        check(lib().zscrc_device_find(
            d_src.data_ptr() if src_bytes else None, src_bytes, arr, k, d_qsrc.data_ptr() if q_bytes else None,
            q_bytes, queries.data_ptr() if nq else None, nq, hits.data_ptr() if nq else None, res.data_ptr(),
            None if scratch is None else scratch.data_ptr(), ctypes.byref(opts),
            FIND_CHECK_ORDER if check_order else 0, torch.cuda.current_stream(dev).cuda_stream), "zscrc_device_find")
    return hits, res


def find(src, levels, qsrc, queries, check_order: bool = False):
    """device_find for lists and keys in host memory (zscrc_zs_find, one
    thread, no device): (hits int64 [nq, 4], res int64 [8]) numpy arrays, the
    same words for the same bytes.  src, qsrc: bytes or uint8 arrays; levels:
    (recs, base) with recs [n, 4] uint64 or int64 arrays; queries [nq, 4]."""
    s, sp, sn = _host(src)
    q, qp, qn = _host(qsrc)
    levels = [(np.ascontiguousarray(r).view(np.int64).reshape(-1, 4), b) for r, b in levels]
    arr, k = _find_levels(levels, lambda r: r.ctypes.data)
    qr = np.ascontiguousarray(queries).view(np.int64).reshape(-1, 4)
    nq = len(qr)
    hits = np.empty((nq, 4), np.int64)
    res = np.empty(FIND_RES_WORDS, np.int64)
    check(lib().zscrc_zs_find(sp if sn else None, sn, arr, k, qp if qn else None, qn, qr.ctypes.data if nq else None,
                              nq, hits.ctypes.data if nq else None, res.ctypes.data,
                              FIND_CHECK_ORDER if check_order else 0), "zscrc_zs_find")
    return hits, res


class GatherOpts(ctypes.Structure):
    """zscrc_gather_opts (include/zscrc.h); 0 = the default."""
    _fields_ = [("tile_bytes", ctypes.c_uint64)]


GATHER_RES_WORDS = 8  # ZSCRC_GATHER_RES_WORDS
GATHER_DEFAULT_TILE = 16384  # zscrc_gather.hip DEF_TILE: what tile_bytes = 0 means
GATHER_STAGE = 1024  # zscrc_gather.hip STAGE: the starts a chunk of the copy stages in LDS


def device_gather_scratch_bytes(nq: int, tile_bytes: int = 0) -> int:
    """zscrc_device_gather_scratch_bytes; 0 = a bad tile or too many items."""
    return lib().zscrc_device_gather_scratch_bytes(nq, ctypes.byref(GatherOpts(tile_bytes)))


def device_gather(d_src: torch.Tensor, items: torch.Tensor, cap: int | None = None, crcs: bool = False,
                  tile_bytes: int = 0, out: tuple | None = None, scratch: torch.Tensor | None = None):
    """The values a batch of hits names, copied out of d_src into one dense
    device buffer on the GPU (zscrc_device_gather): (values uint8, offs int64
    [nq + 1], crcs uint32-as-int32 [nq] or None, res int64 [8]) device tensors.
    items: int64 [nq, 4], device_find's hits or a record list (words 0, 2 and
    3 are read: a row carries a value unless word 0 is FIND_NONE or
    FIND_BAD_QUERY or word 2 is DELETED).  Value i is values[offs[i]:offs[i +
    1]], offs[nq] the total: the CSR layout of a jagged tensor.  With cap (the
    bytes of the values buffer) the call is asynchronous on the current
    stream; cap=None makes the sizing call first, reads the one total word
    and allocates.  res: [code (0; 3 = the total exceeds cap: no value byte
    written, offs complete; -1 = a value outside d_src: nothing written), nq
    or the first offending index, items with a value, total bytes, deletes,
    not found, bad queries, the longest value].  crcs: crc32c(0, value i) over
    the gathered bytes.  tile_bytes: the copy's output tile, a power of two 64
    .. 65536, 0 = the default; the result never depends on it.  out:
    preallocated (values, offs, crcs | None, res), values 16-byte aligned;
    scratch: a 16-byte aligned uint8 tensor of device_gather_scratch_bytes(nq)
    bytes (default: the library's own, stream-ordered)."""
    dev = d_src.device
    nq = int(items.shape[0])
    assert items.dtype == torch.int64 and items.is_contiguous() and (nq == 0 or items.shape[1] == 4)
    src_bytes = d_src.numel() * d_src.element_size()
    opts = GatherOpts(tile_bytes)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sp = None if scratch is None else scratch.data_ptr()

    def call(values, vcap, offs, crc, res):
        with torch.cuda.device(dev):
            check(lib().zscrc_device_gather(
                d_src.data_ptr() if src_bytes else None, src_bytes, items.data_ptr() if nq else None, nq,
                values.data_ptr() if values is not None and values.numel() else None, vcap, offs.data_ptr(),
                None if crc is None else crc.data_ptr(), res.data_ptr(), sp, ctypes.byref(opts), 0, stream),
                "zscrc_device_gather")

    if out is not None:
        values, offs, crc, res = out
        assert offs.numel() >= nq + 1 and res.numel() >= GATHER_RES_WORDS and (crc is None or crc.numel() >= nq)
        call(values, values.numel() if cap is None else cap, offs, crc, res)
        return values, offs, crc, res
    offs = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    res = torch.empty(GATHER_RES_WORDS, dtype=torch.int64, device=dev)
    if cap is None:
        call(None, 0, offs, None, res)
        code, total = (int(v) for v in res[[0, 3]].cpu())
        if code == -1:
            return torch.empty(0, dtype=torch.uint8, device=dev), offs, None, res
        cap = total
    values = torch.empty(cap, dtype=torch.uint8, device=dev)
    crc = torch.zeros(nq, dtype=torch.int32, device=dev) if crcs else None  # a total of 0 is a sizing call
    call(values, cap, offs, crc, res)
    return values, offs, crc, res


def gather(src, items, crcs: bool = False, cap: int | None = None):
    """device_gather in host memory (zscrc_zs_gather, one thread, no device):
    (values uint8, offs int64 [nq + 1], crcs uint32 [nq] or None, res int64
    [8]) numpy arrays, the same words for the same bytes.  src: bytes or a
    uint8 array; items [nq, 4] uint64 or int64.  cap: the bytes of the values
    buffer (default: a sizing call first)."""
    s, sp, sn = _host(src)
    it = np.ascontiguousarray(items).view(np.int64).reshape(-1, 4)
    nq = len(it)
    offs = np.empty(nq + 1, np.int64)
    res = np.empty(GATHER_RES_WORDS, np.int64)

    def call(values, vcap, crc):
        check(lib().zscrc_zs_gather(sp if sn else None, sn, it.ctypes.data if nq else None, nq,
                                    values.ctypes.data if values is not None and vcap else None, vcap,
                                    offs.ctypes.data, None if crc is None else crc.ctypes.data, res.ctypes.data),
              "zscrc_zs_gather")

    if cap is None:
        call(None, 0, None)
        if int(res[0]) == -1:
            return np.empty(0, np.uint8), offs, None, res
        cap = int(res[3])
    values = np.empty(cap, np.uint8)
    crc = np.zeros(nq, np.uint32) if crcs else None
    call(values, cap, crc)
    return values, offs, crc, res


def device_get(d_src: torch.Tensor, levels, d_qsrc: torch.Tensor, queries: torch.Tensor, cap: int | None = None,
               crcs: bool = False, check_order: bool = False, splitters: int = 0, tile_bytes: int = 0):
    """A multi-get on the GPU: device_find, then device_gather over its hits,
    in one call: (values, offs, crcs | None, hits, find_res, gather_res).
    With cap the two stages are asynchronous on the current stream; otherwise
    the values buffer is sized from the find's res[6], the sum of the found
    values' lengths -- one 8-byte read.  A find that refuses its levels
    (find_res[0] = -1) leaves the hits unwritten; the gather is then not
    run and values, offs, crcs and gather_res are None."""
    hits, fres = device_find(d_src, levels, d_qsrc, queries, check_order=check_order, splitters=splitters)
    if cap is None:
        code, total = (int(v) for v in fres[[0, 6]].cpu())
        if code != 0:
            return None, None, None, hits, fres, None
        cap = total
    values, offs, crc, gres = device_gather(d_src, hits, cap=cap, crcs=crcs, tile_bytes=tile_bytes)
    return values, offs, crc, hits, fres, gres


class ScanOpts(ctypes.Structure):
    """zscrc_scan_opts (include/zscrc.h); 0 = the default."""
    _fields_ = [("splitters", ctypes.c_uint32)]


SCAN_RES_WORDS = 12  # ZSCRC_SCAN_RES_WORDS
SCAN_KEEP_DELETES = 1  # ZSCRC_SCAN_KEEP_DELETES
SCAN_CHECK_ORDER = 2  # ZSCRC_SCAN_CHECK_ORDER
SCAN_GRID_THREADS = 1024 * 256  # zscrc_scan.hip GRID_MAX * WG: the rank's persistent grid at its largest
SCAN_BLOCK = 1024  # zscrc_scan.hip BLOCK_RECS: the pairs and the slots one workgroup sums and scans


def _scan_flags(keep_deletes: bool, check_order: bool) -> int:
    return (SCAN_KEEP_DELETES if keep_deletes else 0) | (SCAN_CHECK_ORDER if check_order else 0)


def device_scan_scratch_bytes(nq: int, k: int, cand_cap: int, splitters: int = 0) -> int:
    """zscrc_device_scan_scratch_bytes; 0 = a bad option or an argument above its limit."""
    return lib().zscrc_device_scan_scratch_bytes(nq, k, cand_cap, ctypes.byref(ScanOpts(splitters)))


def device_scan(d_src: torch.Tensor, levels, d_qsrc: torch.Tensor, queries: torch.Tensor, keep_deletes: bool = False,
                check_order: bool = False, cap: int | None = None, cand_cap: int | None = None, splitters: int = 0,
                out: tuple | None = None, scratch: torch.Tensor | None = None):
    """A batch of key prefixes scanned in device-resident sorted record lists
    on the GPU (zscrc_device_scan): (rows, offs, seq, res) int64 device
    tensors.  d_src, levels, d_qsrc and queries are device_find's; query i is
    a prefix, and an empty one matches every key.  rows [cap, 4]: for every
    query in turn the records whose key begins with its prefix, in key order,
    each key once from the first level that holds it, rebased as
    repack.device_merge writes them; a key whose winning record is a delete
    is left out unless keep_deletes.  The rows of query i are
    rows[offs[i]:offs[i + 1]], offs[nq] the total; seq [cap]: the winning
    record's sequence number.  res: [code (0; 3 = more rows than cap, or,
    with res[7] = 1, more candidates than cand_cap: nothing written; -1 = a
    level record outside d_src or, with check_order, a key not above its
    predecessor's: nothing written), nq or the first offending sequence
    number, rows, candidates, superseded, winning deletes, bad queries, the
    overflow's or offence's kind, sum of the rows' key lengths, sum of their
    value lengths, 0, 0].  With cap and cand_cap (the candidates the scratch
    has room for) the call is asynchronous on the current stream.  Otherwise
    it reads res and sizes itself: cand_cap starts at the levels' record
    count and the call is made again once with the reported res[3] on a
    candidate overflow; cap=None makes the sizing call first and allocates
    res[2] rows.  splitters: device_find's; the result never depends on it.
    out: preallocated (rows, offs, seq | None, res); scratch: a 16-byte
    aligned uint8 tensor of device_scan_scratch_bytes(nq, k, cand_cap) bytes
    (default: the library's own, stream-ordered)."""
    dev = d_src.device
    arr, k = _find_levels(levels, lambda r: r.data_ptr())
    for recs, _ in levels:
        assert recs.dtype == torch.int64 and recs.is_contiguous()
    nq = int(queries.shape[0])
    assert queries.dtype == torch.int64 and queries.is_contiguous() and (nq == 0 or queries.shape[1] == 4)
    src_bytes = d_src.numel() * d_src.element_size()
    q_bytes = d_qsrc.numel() * d_qsrc.element_size()
    opts = ScanOpts(splitters)
    flags = _scan_flags(keep_deletes, check_order)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sp = None if scratch is None else scratch.data_ptr()

    def call(rows, rcap, offs, seq, res, ccap):
        with torch.cuda.device(dev):
            check(lib().zscrc_device_scan(
                d_src.data_ptr() if src_bytes else None, src_bytes, arr, k, d_qsrc.data_ptr() if q_bytes else None,
                q_bytes, queries.data_ptr() if nq else None, nq,
                rows.data_ptr() if rows is not None and rcap else None, rcap, offs.data_ptr(),
                None if seq is None or not rcap else seq.data_ptr(), res.data_ptr(), sp, ccap, ctypes.byref(opts),
                flags, stream), "zscrc_device_scan")

    if out is not None:
        rows, offs, seq, res = out
        assert offs.numel() >= nq + 1 and res.numel() >= SCAN_RES_WORDS and cand_cap is not None
        cap = int(rows.shape[0]) if cap is None else cap
        assert rows.numel() >= 4 * cap and (seq is None or seq.numel() >= cap)
        call(rows, cap, offs, seq, res, cand_cap)
        return rows, offs, seq, res
    offs = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    res = torch.empty(SCAN_RES_WORDS, dtype=torch.int64, device=dev)

    def alloc(n):
        return torch.empty((n, 4), dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)

    if cap is not None and cand_cap is not None:
        rows, seq = alloc(cap)
        call(rows, cap, offs, seq, res, cand_cap)
        return rows, offs, seq, res
    sized = cand_cap is not None
    if not sized:
        cand_cap = sum(int(r.shape[0]) for r, _ in levels)
    rows, seq = alloc(cap or 0)
    call(rows, cap or 0, offs, seq, res, cand_cap)
    code, nrows, cands, kind = (int(v) for v in res[[0, 2, 3, 7]].cpu())
    if code == 3 and kind == 1 and not sized:
        cand_cap = cands
        call(rows, cap or 0, offs, seq, res, cand_cap)
        code, nrows, cands, kind = (int(v) for v in res[[0, 2, 3, 7]].cpu())
    if cap is None and code == 3 and kind == 0:
        rows, seq = alloc(nrows)
        call(rows, nrows, offs, seq, res, cand_cap)
    return rows, offs, seq, res


def scan(src, levels, qsrc, queries, keep_deletes: bool = False, check_order: bool = False, cap: int | None = None):
    """device_scan for lists and prefixes in host memory (zscrc_zs_scan, one
    thread, no device): (rows int64 [cap, 4], offs int64 [nq + 1], seq int64
    [cap], res int64 [12]) numpy arrays, the same words for the same bytes.
    src, qsrc: bytes or uint8 arrays; levels: (recs, base) with recs [n, 4]
    uint64 or int64 arrays; queries [nq, 4].  cap: the rows the buffer holds
    (default: a sizing call first)."""
    s, sp, sn = _host(src)
    q, qp, qn = _host(qsrc)
    levels = [(np.ascontiguousarray(r).view(np.int64).reshape(-1, 4), b) for r, b in levels]
    arr, k = _find_levels(levels, lambda r: r.ctypes.data)
    qr = np.ascontiguousarray(queries).view(np.int64).reshape(-1, 4)
    nq = len(qr)
    offs = np.empty(nq + 1, np.int64)
    res = np.empty(SCAN_RES_WORDS, np.int64)
    flags = _scan_flags(keep_deletes, check_order)

    def call(rows, seq, rcap):
        check(lib().zscrc_zs_scan(sp if sn else None, sn, arr, k, qp if qn else None, qn,
                                  qr.ctypes.data if nq else None, nq, rows.ctypes.data if rcap else None, rcap,
                                  offs.ctypes.data, seq.ctypes.data if rcap else None, res.ctypes.data, flags),
              "zscrc_zs_scan")

    if cap is None:
        call(None, None, 0)
        cap = int(res[2]) if int(res[0]) != -1 else 0
    rows, seq = np.empty((cap, 4), np.int64), np.empty(cap, np.int64)
    call(rows, seq, cap)
    return rows, offs, seq, res


def device_foreach(d_src: torch.Tensor, levels, d_qsrc: torch.Tensor, queries: torch.Tensor,
                   keep_deletes: bool = False, crcs: bool = False, check_order: bool = False, splitters: int = 0,
                   tile_bytes: int = 0):
    """An ordered iteration on the GPU: device_scan, then device_gather over
    its rows, in one call: (rows, offs, values, value_offs, crcs | None,
    scan_res, gather_res).  Row j of query i, rows[offs[i] + j], has the key
    d_src[key_off:key_off + key_len] and the value values[value_offs[r]:
    value_offs[r + 1]], r its row index -- it is to device_scan what
    device_get is to device_find.  Both stages size themselves from their
    result words.  A scan that refuses its levels (scan_res[0] = -1) writes
    no row; the gather is then not run and values, value_offs, crcs and
    gather_res are None."""
    rows, offs, _, sres = device_scan(d_src, levels, d_qsrc, queries, keep_deletes=keep_deletes,
                                      check_order=check_order, splitters=splitters)
    if int(sres[0].cpu()) != 0:
        return rows, offs, None, None, None, sres, None
    values, voffs, crc, gres = device_gather(d_src, rows, crcs=crcs, tile_bytes=tile_bytes)
    return rows, offs, values, voffs, crc, sres, gres


class NextOpts(ctypes.Structure):
    """zscrc_next_opts (include/zscrc.h); 0 = the default."""
    _fields_ = [("splitters", ctypes.c_uint32), ("max_steps", ctypes.c_uint32)]


NEXT_PAGE = 0  # ZSCRC_NEXT_PAGE
NEXT_END = 1  # ZSCRC_NEXT_END
NEXT_MORE = 2  # ZSCRC_NEXT_MORE
NEXT_BAD = 3  # ZSCRC_NEXT_BAD
NEXT_INCLUSIVE = 1  # ZSCRC_NEXT_INCLUSIVE
NEXT_CHECK_ORDER = 2  # ZSCRC_NEXT_CHECK_ORDER
NEXT_KEEP_DELETES = 4  # ZSCRC_NEXT_KEEP_DELETES
NEXT_RES_WORDS = 12  # ZSCRC_NEXT_RES_WORDS
NEXT_PAGE_MAX = 65536  # zscrc_next_order.h PAGE_MAX


def _next_flags(inclusive: bool, keep_deletes: bool, check_order: bool) -> int:
    return (NEXT_INCLUSIVE if inclusive else 0) | (NEXT_KEEP_DELETES if keep_deletes else 0) | \
        (NEXT_CHECK_ORDER if check_order else 0)


def device_next_scratch_bytes(nq: int, k: int, splitters: int = 0) -> int:
    """zscrc_device_next_scratch_bytes; 0 = a bad option or an argument above its limit."""
    return lib().zscrc_device_next_scratch_bytes(nq, k, ctypes.byref(NextOpts(splitters, 0)))


def device_next(d_src: torch.Tensor, levels, d_qsrc: torch.Tensor, queries: torch.Tensor, page: int = 1,
                inclusive: bool = False, keep_deletes: bool = False, check_order: bool = False, max_steps: int = 0,
                splitters: int = 0, out: tuple | None = None, scratch: torch.Tensor | None = None):
    """The next `page` live keys after every key of a batch in device-resident
    sorted record lists on the GPU (zscrc_device_next), asynchronous on the
    current stream and never reading anything back: (rows [nq, page, 4], seq
    [nq, page], cur [nq, 4], res [12]) int64 device tensors.  d_src, levels,
    d_qsrc and queries are device_find's.  rows[i, :count_i]: the records of
    the keys greater than query i's (inclusive: not smaller), in key order,
    each key once from the first level that holds it, rebased as device_scan
    writes them; a key whose winning record is a delete is left out unless
    keep_deletes.  The slots after them hold [FIND_NONE, 0, 0, 0] and seq -1,
    so rows.view(-1, 4) is a gather list as it stands.  cur[i]: [key_off,
    key_len, count, state]; state NEXT_PAGE (the page is full), NEXT_END (the
    levels ran out), NEXT_MORE (max_steps steps taken, 0 = no limit) or
    NEXT_BAD (the query's key lies outside d_qsrc).  For PAGE and MORE the
    key is the last one a step took, inside d_src: cur is the query list of
    the next call with d_qsrc = d_src and inclusive=False; for END and BAD it
    is [FIND_NONE, 0], a bad query.  res: [code (0; -1 = a level record
    outside d_src or, with check_order, a key not above its predecessor's:
    nothing written), nq or the first offending sequence number, rows, steps,
    superseded, winning deletes, bad queries, 1 = an order offence, sum of the
    rows' key lengths, sum of their value lengths, queries ended END, queries
    ended MORE].  splitters: device_find's; the result never depends on it.
    out: preallocated (rows, seq | None, cur, res); scratch: a 16-byte aligned
    uint8 tensor of device_next_scratch_bytes(nq, k) bytes (default: the
    library's own, stream-ordered)."""
    dev = d_src.device
    arr, k = _find_levels(levels, lambda r: r.data_ptr())
    for recs, _ in levels:
        assert recs.dtype == torch.int64 and recs.is_contiguous()
    nq = int(queries.shape[0])
    assert queries.dtype == torch.int64 and queries.is_contiguous() and (nq == 0 or queries.shape[1] == 4)
    if out is None:
        out = (torch.empty((nq, page, 4), dtype=torch.int64, device=dev),
               torch.empty((nq, page), dtype=torch.int64, device=dev),
               torch.empty((nq, 4), dtype=torch.int64, device=dev),
               torch.empty(NEXT_RES_WORDS, dtype=torch.int64, device=dev))
    rows, seq, cur, res = out
    assert rows.numel() >= 4 * nq * page and (seq is None or seq.numel() >= nq * page) and cur.numel() >= 4 * nq and \
        res.numel() >= NEXT_RES_WORDS
    src_bytes = d_src.numel() * d_src.element_size()
    q_bytes = d_qsrc.numel() * d_qsrc.element_size()
    opts = NextOpts(splitters, max_steps)
    with torch.cuda.device(dev):
        check(lib().zscrc_device_next(
            d_src.data_ptr() if src_bytes else None, src_bytes, arr, k, d_qsrc.data_ptr() if q_bytes else None,
            q_bytes, queries.data_ptr() if nq else None, nq, page, rows.data_ptr() if nq else None,
            seq.data_ptr() if seq is not None and nq else None, cur.data_ptr() if nq else None, res.data_ptr(),
            None if scratch is None else scratch.data_ptr(), ctypes.byref(opts),
            _next_flags(inclusive, keep_deletes, check_order), torch.cuda.current_stream(dev).cuda_stream),
            "zscrc_device_next")
    return rows, seq, cur, res


def next_(src, levels, qsrc, queries, page: int = 1, inclusive: bool = False, keep_deletes: bool = False,
          check_order: bool = False, max_steps: int = 0):
    """device_next for lists and keys in host memory (zscrc_zs_next, one
    thread, no device): (rows int64 [nq, page, 4], seq int64 [nq, page], cur
    int64 [nq, 4], res int64 [12]) numpy arrays, the same words for the same
    bytes.  src, qsrc: bytes or uint8 arrays; levels: (recs, base) with recs
    [n, 4] uint64 or int64 arrays; queries [nq, 4] (a cur of an earlier call
    among them).  The underscore: next is a builtin."""
    s, sp, sn = _host(src)
    q, qp, qn = _host(qsrc)
    levels = [(np.ascontiguousarray(r).view(np.int64).reshape(-1, 4), b) for r, b in levels]
    arr, k = _find_levels(levels, lambda r: r.ctypes.data)
    qr = np.ascontiguousarray(queries).view(np.int64).reshape(-1, 4)
    nq = len(qr)
    rows, seq = np.empty((nq, page, 4), np.int64), np.empty((nq, page), np.int64)
    cur = np.empty((nq, 4), np.int64)
    res = np.empty(NEXT_RES_WORDS, np.int64)
    check(lib().zscrc_zs_next(sp if sn else None, sn, arr, k, qp if qn else None, qn, qr.ctypes.data if nq else None,
                              nq, page, rows.ctypes.data if nq else None, seq.ctypes.data if nq else None,
                              cur.ctypes.data if nq else None, res.ctypes.data, max_steps,
                              _next_flags(inclusive, keep_deletes, check_order)), "zscrc_zs_next")
    return rows, seq, cur, res


def device_fetchnext(d_src: torch.Tensor, levels, d_qsrc: torch.Tensor, queries: torch.Tensor, page: int = 1,
                     inclusive: bool = False, keep_deletes: bool = False, check_order: bool = False,
                     max_steps: int = 0, splitters: int = 0, tile_bytes: int = 0):
    """The next keys with their values on the GPU: device_next, then
    device_gather over its rows for the values and a second gather for the
    keys, in one call: (keys, key_offs, values, value_offs, rows, seq, cur,
    next_res, gather_res).  Slot r = i * page + j is row j of query i: its key
    is keys[key_offs[r]:key_offs[r + 1]], its value values[value_offs[r]:
    value_offs[r + 1]]; a filler slot has neither, a kept delete a key only.
    The key gather reads a view of the rows built with torch, the key words
    in the value words.  It is to device_next what device_foreach is to
    device_scan: the gathers size themselves from their result words.  A
    next that refuses its levels (next_res[0] = -1) writes no row; the gathers
    are then not run and keys, key_offs, values, value_offs and gather_res
    are None."""
    rows, seq, cur, nres = device_next(d_src, levels, d_qsrc, queries, page=page, inclusive=inclusive,
                                       keep_deletes=keep_deletes, check_order=check_order, max_steps=max_steps,
                                       splitters=splitters)
    if int(nres[0].cpu()) != 0:
        return None, None, None, None, rows, seq, cur, nres, None
    items = rows.view(-1, 4)
    values, voffs, _, gres = device_gather(d_src, items, tile_bytes=tile_bytes)
    as_values = torch.stack((items[:, 0], torch.zeros_like(items[:, 0]), items[:, 0], items[:, 1]), dim=1).contiguous()
    keys, koffs, _, _ = device_gather(d_src, as_values, tile_bytes=tile_bytes)
    return keys, koffs, values, voffs, rows, seq, cur, nres, gres


def verify_device_images(d_arena: torch.Tensor, images) -> list:
    """verify_device_image() for the k active or finalised images [(off,
    size)] of a device-resident arena in one call (zscrc_device_verify_images):
    a list of k report dicts, each equal to verify_device_image() of that
    image's bytes alone.  Synchronous."""
    size = d_arena.numel() * d_arena.element_size()
    arr, k = _walk_images(images)
    reps = (Report * max(k, 1))()
    with torch.cuda.device(d_arena.device):
        check(lib().zscrc_device_verify_images(d_arena.data_ptr(), size, arr, k, reps,
                                               torch.cuda.current_stream(d_arena.device).cuda_stream),
              "zscrc_device_verify_images")
    return [reps[j].as_dict() for j in range(k)]


def verify_commits(d_image: torch.Tensor, span_off: torch.Tensor, span_len: torch.Tensor,
                   seed: torch.Tensor | None = None, max_len: int | None = None):
    """Device-resident commit verification: (crc, status) int32 tensors;
    status 1 = stored CRC matches, 0 = mismatch, 2 = no commit record.
    seed (int32, optional): span i's CRC continues from seed[i]
    (zscrc_device_verify_commits_seeded) -- the reference's zero-length
    finalise commit chains from the previous span's CRC.
    max_len (optional): a known bound on the span lengths, e.g. from the host
    walk (zscrc_device_verify_commits_bounded); results never depend on it."""
    n = span_off.numel()
    size = d_image.numel() * d_image.element_size()
    crc = torch.empty(n, dtype=torch.int32, device=d_image.device)
    st = torch.empty(n, dtype=torch.int32, device=d_image.device)
    with torch.cuda.device(d_image.device):
        stream = torch.cuda.current_stream(d_image.device).cuda_stream
        if max_len is not None:
            assert seed is None or (seed.numel() == n and seed.dtype == torch.int32)
            check(lib().zscrc_device_verify_commits_bounded(
                d_image.data_ptr(), size, span_off.data_ptr(), span_len.data_ptr(),
                None if seed is None else seed.data_ptr(), n, max_len, crc.data_ptr(), st.data_ptr(),
                stream), "zscrc_device_verify_commits_bounded")
        elif seed is None:
            check(lib().zscrc_device_verify_commits(
                d_image.data_ptr(), size, span_off.data_ptr(), span_len.data_ptr(), n, crc.data_ptr(),
                st.data_ptr(), stream), "zscrc_device_verify_commits")
        else:
            assert seed.numel() == n and seed.dtype == torch.int32 and seed.device == d_image.device
            check(lib().zscrc_device_verify_commits_seeded(
                d_image.data_ptr(), size, span_off.data_ptr(), span_len.data_ptr(), seed.data_ptr(), n,
                crc.data_ptr(), st.data_ptr(), stream), "zscrc_device_verify_commits_seeded")
    return crc, st


def verify_commits_verdict(d_image: torch.Tensor, span_off: torch.Tensor, span_len: torch.Tensor,
                           seed: torch.Tensor | None = None, max_len: int | None = None, cap: int = 4096,
                           out: tuple | None = None, min_len: int = 0):
    """Device verdict (zscrc_device_verify_commits_verdict): (nbad, bad)
    int64 device tensors -- nbad[0] = commits that do not verify, bad[:min(
    nbad, cap)] their indices in no particular order.  No per-commit output.
    `out`: preallocated (nbad, bad) tensors to reuse.  max_len alone: a bound
    the results never depend on (zscrc_device_verify_commits_verdict); with
    min_len > 0, [min_len, max_len] is a range every span length must lie in
    (zscrc_device_verify_commits_verdict_range: classes outside it get no
    launch)."""
    n = span_off.numel()
    size = d_image.numel() * d_image.element_size()
    dev = d_image.device
    if out is None:
        out = (torch.empty(1, dtype=torch.int64, device=dev), torch.empty(max(cap, 1), dtype=torch.int64, device=dev))
    nbad, bad = out
    assert seed is None or (seed.numel() == n and seed.dtype == torch.int32)
    mx = LEN_UNBOUNDED if max_len is None else max_len
    stream = torch.cuda.current_stream(dev).cuda_stream
    sp = None if seed is None else seed.data_ptr()
    with torch.cuda.device(dev):
        if min_len > 0:
            check(lib().zscrc_device_verify_commits_verdict_range(
                d_image.data_ptr(), size, span_off.data_ptr(), span_len.data_ptr(), sp, n, min_len, mx,
                nbad.data_ptr(), bad.data_ptr(), min(cap, bad.numel()), stream),
                "zscrc_device_verify_commits_verdict_range")
        else:
            check(lib().zscrc_device_verify_commits_verdict(
                d_image.data_ptr(), size, span_off.data_ptr(), span_len.data_ptr(), sp, n, mx,
                nbad.data_ptr(), bad.data_ptr(), min(cap, bad.numel()), stream),
                "zscrc_device_verify_commits_verdict")
    return nbad, bad


def write_commits(d_image: torch.Tensor, span_off: torch.Tensor, span_len: torch.Tensor,
                  max_len: int | None = None, status: bool = False, crc: bool = True):
    """Writer side on the GPU: compute every commit CRC and store it
    big-endian into its commit record in `d_image` (in place).  max_len: a
    known bound on the span lengths (zscrc_device_write_commits_bounded).
    crc=False: the CRCs only go into the image (returns None).
    Returns the CRCs, or (crc, status) with status=True: 1 written, 2 no
    commit record there (nothing written)."""
    n = span_off.numel()
    size = d_image.numel() * d_image.element_size()
    want_crc = crc
    crc = torch.empty(n, dtype=torch.int32, device=d_image.device) if want_crc else None
    st = torch.empty(n, dtype=torch.int32, device=d_image.device) if status else None
    with torch.cuda.device(d_image.device):
        check(lib().zscrc_device_write_commits_bounded(
            d_image.data_ptr(), size, span_off.data_ptr(), span_len.data_ptr(), n,
            LEN_UNBOUNDED if max_len is None else max_len, None if crc is None else crc.data_ptr(),
            None if st is None else st.data_ptr(),
            torch.cuda.current_stream(d_image.device).cuda_stream), "zscrc_device_write_commits_bounded")
    return (crc, st) if status else crc


def commit_crcs(d_image: torch.Tensor, span_off: torch.Tensor, span_len: torch.Tensor,
                max_len: int | None = None, status: bool = False):
    """The writer's commit CRCs out of place (zscrc_device_commit_crcs_bounded):
    an int32 tensor, crc[i] = what zscrc_device_write_commits would store for
    span i; the image is only read.  status=True: (crc, status), 1 a commit
    record is there, 2 none."""
    n = span_off.numel()
    size = d_image.numel() * d_image.element_size()
    crc = torch.empty(n, dtype=torch.int32, device=d_image.device)
    st = torch.empty(n, dtype=torch.int32, device=d_image.device) if status else None
    with torch.cuda.device(d_image.device):
        check(lib().zscrc_device_commit_crcs_bounded(
            d_image.data_ptr(), size, span_off.data_ptr(), span_len.data_ptr(), n,
            LEN_UNBOUNDED if max_len is None else max_len, crc.data_ptr(), None if st is None else st.data_ptr(),
            torch.cuda.current_stream(d_image.device).cuda_stream), "zscrc_device_commit_crcs_bounded")
    return (crc, st) if status else crc


class FillReport(ctypes.Structure):
    """zscrc_fill_report (include/zscrc.h)."""
    _fields_ = [("commits", ctypes.c_uint64), ("no_record", ctypes.c_uint64), ("long_commits", ctypes.c_uint64),
                ("bytes", ctypes.c_uint64), ("desc_bytes", ctypes.c_uint64), ("chunks", ctypes.c_uint64),
                ("staged", ctypes.c_int32), ("threads", ctypes.c_int32), ("h2d_s", ctypes.c_double),
                ("total_s", ctypes.c_double), ("setup_s", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def fill_commits(image, span_off, span_len, max_len: int | None = None, threads: int = 0) -> dict:
    """The commit writer for a HOST image (zscrc_zs_fill_commits): every
    commit CRC computed on the current GPU and stored into `image` in place
    (a writable uint8 numpy array or CPU tensor; pinned memory is copied
    directly, pageable memory through pinned staging).  span_off / span_len:
    sorted, disjoint spans (uint64 numpy arrays or CPU tensors)."""
    if isinstance(image, torch.Tensor):
        assert not image.is_cuda and image.is_contiguous()
        ptr, size = image.data_ptr(), image.numel() * image.element_size()
    else:
        assert image.flags.c_contiguous and image.flags.writeable
        ptr, size = image.ctypes.data, image.nbytes
    o = np.ascontiguousarray(span_off.numpy() if isinstance(span_off, torch.Tensor) else span_off, dtype=np.uint64)
    ln = np.ascontiguousarray(span_len.numpy() if isinstance(span_len, torch.Tensor) else span_len, dtype=np.uint64)
    assert o.shape == ln.shape
    rep = FillReport()
    check(lib().zscrc_zs_fill_commits(ptr, size, o.ctypes.data, ln.ctypes.data, len(o),
                                      LEN_UNBOUNDED if max_len is None else max_len, threads, ctypes.byref(rep)),
          "zscrc_zs_fill_commits")
    return rep.as_dict()


class FilesReport(ctypes.Structure):
    """zscrc_files_report (include/zscrc.h)."""
    _fields_ = [("files", ctypes.c_uint64), ("commits", ctypes.c_uint64), ("bytes", ctypes.c_uint64),
                ("bad_commits", ctypes.c_uint64), ("stale_empty_commits", ctypes.c_uint64),
                ("header_errors", ctypes.c_uint64), ("walk_errors", ctypes.c_uint64),
                ("first_bad_file", ctypes.c_uint64), ("first_bad_off", ctypes.c_uint64),
                ("first_bad_what", ctypes.c_int32), ("threads", ctypes.c_int32), ("staged", ctypes.c_int32),
                ("copy_s", ctypes.c_double), ("verify_tail_s", ctypes.c_double), ("total_s", ctypes.c_double),
                ("devices", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def set_devices(ids) -> None:
    """Device slots of verify_files / consistent (zscrc_set_devices): a list
    of device ids, repeats allowed; None or [] = the default (env
    ZSCRC_DEVICES, else every visible gfx950 device)."""
    ids = list(ids or [])
    arr = (ctypes.c_int * max(1, len(ids)))(*ids)
    check(lib().zscrc_set_devices(arr, len(ids)), "zscrc_set_devices")


def devices() -> list:
    """The device slots a verify_files call would use now."""
    arr = (ctypes.c_int * 64)()
    n = lib().zscrc_files_devices(arr, 64)
    if n < 0:
        check(n, "zscrc_files_devices")
    return list(arr[:n])


def verify_files(images, kinds=None, threads: int = 0) -> dict:
    """End to end from host memory (zscrc_zs_verify_files): every header,
    walk and commit CRC of the given file images (numpy uint8 arrays, bytes
    or memmaps; kinds default ACTIVE), on the current GPU.  Synchronous."""
    arrs = [_host(im)[0] for im in images]
    n = len(arrs)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data if a.nbytes else None for a in arrs])
    sizes = np.array([a.nbytes for a in arrs], np.uint64)
    kk = np.array([ACTIVE] * n if kinds is None else list(kinds), np.int32)
    rep = FilesReport()
    check(lib().zscrc_zs_verify_files(ptrs, sizes.ctypes.data, kk.ctypes.data, n, threads, ctypes.byref(rep)),
          "zscrc_zs_verify_files")
    return rep.as_dict()
