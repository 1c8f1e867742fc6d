"""zscrc_zs_gather, the value gather in host memory, against the model of
tests/gather_cases.py on every case, on the hits zsfile.find produces over the
cases of tests/find_cases.py, and on the record list of the reference-written
packed file tests/golden/ref_format/packed.zs.  No GPU."""
import os

import numpy as np
import pytest

from oracle import oracle
from oracle import zs_format as zf
from tests import find_cases as fc
from tests import gather_cases as gc
from tests.images import REF
from zeroskip_amd import repack, zsfile
from zeroskip_amd._lib import lib

CANARY = 0xA5


def _raw(src: bytes, items, cap, crcs=True, out_null=False):
    """zscrc_zs_gather into canary-filled arrays: (out, offs, crcs, res) as they are afterwards."""
    items = gc.items_of(items)
    nq = len(items)
    s = np.frombuffer(src, np.uint8)
    out = np.full(cap + 32, CANARY, np.uint8)
    offs = np.full(nq + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    crc = np.full(nq, 0xA5A5A5A5, np.uint32)
    res = np.zeros(8, np.uint64)
    rc = lib().zscrc_zs_gather(s.ctypes.data if len(s) else None, len(s), items.ctypes.data if nq else None, nq,
                               None if out_null else out.ctypes.data, cap, offs.ctypes.data,
                               crc.ctypes.data if crcs else None, res.ctypes.data)
    assert rc == 0
    return out, offs, crc, [int(v) for v in res]


def _same(case):
    values, offs, crcs, res = case.model()
    total = res[3]
    for cap in (total, total + 7):
        out, o, c, r = _raw(case.src, case.items, cap)
        assert r == res, (case.name, r, res)
        assert o.tolist() == offs.tolist(), case.name
        assert out[:total].tobytes() == values.tobytes(), case.name
        assert bool((out[total:] == CANARY).all()), case.name             # nothing at or past the total
        assert c.tolist() == crcs.tolist(), case.name
    assert res[2] + res[4] + res[5] + res[6] == res[1] == case.nq
    # the wrapper: a sizing call, then the gather
    v, o, c, r = zsfile.gather(case.src, case.items, crcs=True)
    assert v.tobytes() == values.tobytes() and o.view(np.uint64).tolist() == offs.tolist()
    assert c.tolist() == crcs.tolist() and [int(x) for x in r.view(np.uint64)] == res
    v2, o2, c2, _ = zsfile.gather(case.src, case.items)
    assert c2 is None and v2.tobytes() == v.tobytes() and o2.tolist() == o.tolist()


@pytest.fixture(scope="module")
def cases():
    return gc.small_cases()


def test_the_model_is_the_plain_slices(cases):
    """What the other tests rest on: the vectorised model against src[off:off + len] joined."""
    for case in cases + [gc.random_case(0)]:
        values, offs, crcs, res = case.model()
        parts = gc.slices(case.src, case.items)
        assert values.tobytes() == b"".join(p or b"" for p in parts), case.name
        assert offs.tolist() == np.cumsum([0] + [len(p or b"") for p in parts]).tolist()
        assert crcs.tolist() == [oracle.crc32c_hw(0, p) if p else 0 for p in parts]


def test_every_small_case(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) >= 35
    for case in cases:
        _same(case)


def test_tiles_one_byte_values_and_a_long_value():
    for case in (gc.residue_case(1024, 3), gc.residue_case(16384, 11), gc.one_byte_case(70_001), gc.long_value_case()):
        _same(case)


def test_random_cases():
    for seed in range(5):
        _same(gc.random_case(seed))


def test_items_without_a_value(cases):
    by = {c.name: c for c in cases}
    for name, word in (("only_misses", 5), ("only_deletes", 4), ("only_badq", 6)):
        out, offs, crc, res = _raw(by[name].src, by[name].items, 64)
        assert res == [0, 300, 0, 0] + [300 if w == word else 0 for w in (4, 5, 6)] + [0]
        assert offs.tolist() == [0] * 301 and crc.tolist() == [0] * 300 and bool((out == CANARY).all())
    c = by["misses_between"]
    assert c.items[0, 0] == gc.NONE and c.items[-1, 0] == gc.NONE and c.nq == 30_003
    values, offs, _, res = c.model()
    assert res[2:6] == [3, 88, 0, 30_000] and offs[10_000] == 0 and offs[10_001] == 50 and offs[-1] == 88


def test_overflow_and_the_sizing_call(cases):
    for case in (next(c for c in cases if c.name == "n257"), gc.random_case(1)):
        values, offs, crcs, res = case.model()
        total = res[3]
        for cap in (total - 1, 16, 0):
            out, o, c, r = _raw(case.src, case.items, cap)
            assert r == [gc.OVERFLOW] + res[1:], (case.name, cap)
            assert o.tolist() == offs.tolist()                     # complete
            assert bool((out == CANARY).all())                     # no byte of the output
            assert c.tolist() == [0] * case.nq                     # every CRC 0
            assert case.model(cap=cap)[3] == r
        out, o, c, r = _raw(case.src, case.items, 0, out_null=True)   # the sizing call leaves the CRCs alone
        assert r == [gc.OVERFLOW] + res[1:] and o.tolist() == offs.tolist()
        assert bool((c == 0xA5A5A5A5).all())


def test_values_outside_the_source(cases):
    case = next(c for c in cases if c.name == "n4097")
    size = len(case.src)
    val = np.flatnonzero(gc.kinds(case.items)[0])

    def bad(changes, first):
        items = case.items.copy()
        for i, off, ln in changes:
            items[i, 2:] = (off, ln)
        out, offs, crc, res = _raw(case.src, items, 1 << 16)
        assert res == [gc.EINVAL64, first, 0, 0, 0, 0, 0, 0] == gc.model(case.src, items)[3], (changes, res)
        assert bool((out == CANARY).all()) and bool((offs == 0xA5A5A5A5A5A5A5A5).all())
        assert crc.tolist() == [0] * case.nq

    a, b, c = int(val[3]), int(val[len(val) // 2]), int(val[-1])
    assert a < 1024 <= c
    bad([(a, size - 4, 5)], a)                       # one byte past the source
    bad([(b, size, 1)], b)
    bad([(b, size + 1, 0)], b)                       # val_off beyond the source, no byte asked for
    bad([(c, 0, 1 << 63)], c)
    bad([(c, gc.U64_MAX - 1, 3)], c)                 # an add that would wrap
    bad([(c, 1, size), (b, 9, size), (a, size, 0)], b)   # the smaller index; a value that ends with the source is fine


def test_hits_of_the_find_cases():
    """find, then gather: the values the levels hold for the queries, and the two stages' counts."""
    n = 0
    for case in fc.small_cases() + [fc.random_find_case(2)]:
        hits, fres = zsfile.find(case.src, case.levels, case.qsrc, case.queries)
        want, wres = case.model()
        assert hits.view(np.uint64).tolist() == want.tolist()
        v, o, c, r = zsfile.gather(case.src, hits, crcs=True)
        mv, mo, mc, mr = gc.model(case.src, want)
        assert v.tobytes() == mv.tobytes() and o.view(np.uint64).tolist() == mo.tolist() and c.tolist() == mc.tolist()
        r = [int(x) for x in r.view(np.uint64)]
        assert r == mr
        assert [r[2], r[3], r[4], r[5], r[6]] == [wres[2], wres[6], wres[3], wres[4], wres[5]], case.name
        n += r[2]
    assert n > 1000


def test_reference_packed_file():
    img = open(os.path.join(REF, "packed.zs"), "rb").read()
    pairs = zf.packed_records(img)
    (ko, kl, vo, vl), rc = repack.records(img, zsfile.PACKED)
    recs = np.stack([ko, kl, vo, vl], axis=1)
    assert len(recs) == len(pairs) > 100
    v, o, c, r = zsfile.gather(img, recs, crcs=True)         # a record list is a gather list as it stands
    o = o.tolist()
    got = [v[o[i]:o[i + 1]].tobytes() for i in range(len(pairs))]
    dele = [val is None for _, val in pairs]
    assert got == [val or b"" for _, val in pairs]
    assert [int(x) for x in r] == [0, len(pairs), len(pairs) - sum(dele), len(v), sum(dele), 0, 0,
                                   max(len(g) for g in got)]
    assert c.tolist() == [oracle.crc32c_hw(0, g) if g else 0 for g in got]
    mv, mo, mc, mr = gc.model(img, recs)
    assert v.tobytes() == mv.tobytes() and o == mo.tolist() and [int(x) for x in r] == mr
