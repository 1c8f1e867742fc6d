"""The host log writer (zscrc_zs_log, zeroskip_amd/csrc/zscrc_log.cpp; the twin
of zscrc_device_log, built from the layout functions the kernels call) against
the format oracle's FileWriter on every case of tests/log_cases.py, byte for
byte, and its result words and optional outputs against the host lister and the
host walk of that image.  Then parity with the reference's own writer: two
active files the reference wrote, listed, and written again.  No GPU."""
import os

import numpy as np
import pytest

from tests import log_cases as lc
from tests import records_images as ri
from tests.images import REF as GOLDEN
from tests.log_cases import check_against_image
from zeroskip_amd import zsfile
from zeroskip_amd._lib import lib

CANARY = 0xA5


def run_host(case, slack=64, tile=0):
    """zsfile.log of the case into a canary-filled image with the prefix in place: (result, buffer)."""
    want = case.want
    out = np.full(len(want) + slack, CANARY, np.uint8)
    out[:case.at] = np.frombuffer(case.prefix, np.uint8)
    d = zsfile.log(case.src, case.recs, case.tx_end, case.uuid, case.startidx, case.endidx, out=out, at=case.at,
                   finalise=case.finalise, prev_crc=case.prev_crc, tile_bytes=tile, new_recs=True, spans=True)
    return d, out


def test_every_small_case():
    cases = lc.small_cases()
    assert len(cases) >= 160
    for case in cases:
        d, out = run_host(case)
        check_against_image(case, d, out.tobytes())
        assert bool((out[len(case.want):] == CANARY).all()), case.name     # nothing at or past the end offset
        assert out[:case.at].tobytes() == case.prefix


@pytest.mark.parametrize("i", range(4))
def test_big_cases(i):
    case = lc.big_cases()[i]
    d, out = run_host(case, slack=16)
    check_against_image(case, d, out.tobytes())
    assert d["long_commits"] == (0 if case.name == "span_16777208" else 1)
    assert bool((out[len(case.want):] == CANARY).all())


def test_sized_by_the_wrapper():
    for case in lc.small_cases()[:12] + lc.appends():
        d = zsfile.log(case.src, case.recs, case.tx_end, case.uuid, case.startidx, case.endidx, at=case.at,
                       finalise=case.finalise, prev_crc=case.prev_crc)
        assert d["code"] == 0 and d["image"][case.at:].tobytes() == case.want[case.at:], case.name


def test_bad_inputs_leave_everything_untouched():
    base, bad = lc.bad_inputs()
    for name, case, cap, head in bad:
        cap = len(base.want) + 64 if cap is None else cap
        out = np.full(cap, CANARY, np.uint8)
        res = np.full(8, 0x77, np.uint64)
        nr = np.full((case.n, 4), 0x5A5A, np.uint64)
        so, sl = np.full(8, 0x5A5A, np.uint64), np.full(8, 0x5A5A, np.uint64)
        te = np.asarray(case.tx_end, np.uint64)
        rc = lib().zscrc_zs_log(np.frombuffer(case.src, np.uint8).ctypes.data, len(case.src), case.recs.ctypes.data,
                                case.n, te.ctypes.data if len(te) else res.ctypes.data, len(te), case.uuid, 3, 3,
                                out.ctypes.data if cap else None, cap, 0, nr.ctypes.data, so.ctypes.data,
                                sl.ctypes.data, res.ctypes.data, None, 0)
        assert rc == 0, name
        assert [int(v) for v in res[:3]] == head, (name, res)
        if head[0] == lc.OVERFLOW:
            assert [int(v) for v in res[3:]] == [len(base.want), base.n_commits, 0, 0, 0], (name, res)
        else:
            assert [int(v) for v in res[3:]] == [0] * 5, (name, res)
        assert bool((out == CANARY).all() and (nr == 0x5A5A).all() and (so == 0x5A5A).all() and (sl == 0x5A5A).all()), name


def test_edges_that_are_legal():
    """A key that ends exactly at src_size, an empty key at src_size, a delete whose val_len is garbage."""
    base, _ = lc.bad_inputs()
    size = len(base.src)
    recs = base.recs.copy()
    recs[0] = (size - 3, 3, size, 0)
    recs[1] = (size, 0, lc.U64_MAX, 12345)
    case = lc.Case("edges", base.src, recs, tx_end=base.tx_end)
    d, out = run_host(case)
    check_against_image(case, d, out.tobytes())


# ---------------------------------------------- parity with the reference's writer
def _rewrite(img: bytes, upto=None):
    """The list, the table and the header fields of a file the reference wrote;
    upto: only the commits before that index, then the finalise commit."""
    recs, rc = ri.host_records(img, zsfile.ACTIVE)
    off, ln, wrc, end = zsfile.walk(img)
    assert rc == zsfile.END and wrc == zsfile.END and end == len(img)
    commit_at = (off + ln).astype(np.uint64)
    if upto is not None:
        commit_at = commit_at[:upto]
        recs = recs[recs[:, 0] < commit_at[-1]]
    tx_end = [int((recs[:, 0] < c).sum()) for c in commit_at]
    uuid, sidx, eidx = img[12:28], int.from_bytes(img[28:32], "big"), int.from_bytes(img[32:36], "big")
    return recs, tx_end, uuid, sidx, eidx, ln


def test_reference_active_clean_is_rewritten_identically():
    with open(os.path.join(GOLDEN, "active_clean.zs"), "rb") as fh:
        img = fh.read()
    recs, tx_end, uuid, sidx, eidx, ln = _rewrite(img)
    assert len(tx_end) == 60 and len(recs) > 60 and int((recs[:, 2] == lc.U64_MAX).sum()) > 0
    d = zsfile.log(img, recs, tx_end, uuid, sidx, eidx)
    assert d["code"] == 0 and d["image"].tobytes() == img


def test_reference_active_stale_prefix_is_rewritten_identically():
    """active_stale.zs holds zero-length commits the reference hashed from a
    stale register in mid-file (zs_active_file_finalise between transactions:
    offsets 28512 and 28776).  The interface writes such a commit only behind
    the last transaction of a call, so the file is rewritten in the three calls
    the reference's own history consists of: up to and with the first stale
    commit (FINALISE), the part up to the second appended with FINALISE, and
    the rest appended -- each call from the records and commits listed in the
    reference's bytes, and the whole must be the identical file."""
    with open(os.path.join(GOLDEN, "active_stale.zs"), "rb") as fh:
        img = fh.read()
    recs, rc = ri.host_records(img, zsfile.ACTIVE)
    off, ln, wrc, end = zsfile.walk(img)
    assert rc == zsfile.END and wrc == zsfile.END and end == len(img)
    commit_at = [int(o + l) for o, l in zip(off, ln)]
    # a zero-length commit right behind another commit: the stale finalise commit
    stale = [c for c, (o, l) in enumerate(zip(off, ln)) if l == 0 and c and commit_at[c - 1] + 8 == commit_at[c]]
    assert [commit_at[c] for c in stale] == [28512, 28776]
    uuid, sidx, eidx = img[12:28], int.from_bytes(img[28:32], "big"), int.from_bytes(img[32:36], "big")
    out = np.zeros(len(img), np.uint8)
    at, first_commit, prev = 0, 0, 0
    for stop in stale + [len(commit_at)]:
        cs = commit_at[first_commit:stop]
        lo = at if at else 40
        part = recs[(recs[:, 0] >= lo) & (recs[:, 0] < (cs[-1] if cs else lo))]
        tx_end = [int((part[:, 0] < c).sum()) for c in cs]
        fin = stop != len(commit_at)
        d = zsfile.log(img, part, tx_end, uuid, sidx, eidx, out=out[:], at=at, finalise=fin, prev_crc=prev)
        assert d["code"] == 0
        at, first_commit, prev = d["end"], stop + 1, d["last_crc"]
        assert out[:at].tobytes() == img[:at], stop
    assert at == len(img) and out.tobytes() == img
