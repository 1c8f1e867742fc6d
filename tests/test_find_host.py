"""zscrc_zs_find, the lookup for lists and keys in host memory, against the
model of tests/find_cases.py on every case, and over the reference-written
packed file tests/golden/ref_format/packed.zs.  No GPU."""
import os

import numpy as np
import pytest

from oracle import zs_format as zf
from tests import find_cases as fc
from tests import merge_cases as mc
from tests.images import REF, U64_MAX
from zeroskip_amd import repack, zsfile


def _same(case, check_order=False):
    want, wres = case.model()
    hits, res = zsfile.find(case.src, case.levels, case.qsrc, case.queries, check_order=check_order)
    assert [int(v) for v in res.view(np.uint64)] == wres, case.name
    assert hits.view(np.uint64).tolist() == want.tolist(), case.name
    assert sum(wres[2:6]) == wres[1] == len(case.queries)


@pytest.fixture(scope="module")
def cases():
    return fc.small_cases()


def test_every_small_case(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) >= 25
    for case in cases:
        for check_order in (False, True):
            _same(case, check_order)


def test_random_cases():
    for seed in range(6):
        _same(fc.random_find_case(seed), bool(seed & 1))


def test_deletes_and_levels(cases):
    c = next(c for c in cases if c.name == "deletes")
    hits, res = zsfile.find(c.src, c.levels, c.qsrc, c.queries)
    h = hits.view(np.uint64).tolist()
    a, b, cc, d = h[0], h[1], h[2], h[3]
    assert a[0] == 0 and a[2] == U64_MAX                    # a delete in level 0 over a value in level 2
    assert b[0] == 0 and c.src[b[2]:b[2] + b[3]] == b"new"  # a value in level 0 over a delete in level 2
    assert cc[0] == 2 and c.src[cc[2]:cc[2] + cc[3]] == b"last"
    assert d == [fc.NONE, 3, 0, 0]                          # level 2 holds a, b, c below d
    assert [int(v) for v in res] == [0, 8, 4, 1, 3, 0, 3 + 1 + 4 + 1, 0]


def test_bad_queries_among_good_ones(cases):
    c = next(c for c in cases if c.name == "n65")
    q = c.queries.copy()
    size = len(c.qsrc)
    q[3, 1] = size - int(q[3, 0]) + 1       # ends one byte past the query bytes
    q[10, 0] = U64_MAX - 3                  # an offset near 2^64
    q[20, 1] = U64_MAX                      # key_len = 2^64 - 1
    bad = fc.FindCase("badq", c.src, c.levels, c.qsrc, q)
    want, wres = bad.model()
    assert wres[5] == 3 and [int(want[i, 0]) for i in (3, 10, 20)] == [fc.BAD_QUERY] * 3
    _same(bad)


def test_records_outside_the_source(cases):
    c = next(c for c in cases if c.name == "n194")
    size, recs = len(c.src), c.levels[0][0]

    def bad(changes, first, base=0):
        r = recs.copy()
        for i, col, v in changes:
            r[i, col] = v
        hits = np.full((len(c.queries), 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
        res = np.zeros(8, np.uint64)
        arr, k = zsfile._find_levels([(r[:100], base), (r[100:], base)], lambda a: a.ctypes.data)
        from zeroskip_amd._lib import lib
        src = np.frombuffer(c.src, np.uint8)
        qs = np.frombuffer(c.qsrc, np.uint8)
        assert lib().zscrc_zs_find(src.ctypes.data, size, arr, k, qs.ctypes.data, len(qs), c.queries.ctypes.data,
                                   len(c.queries), hits.ctypes.data, res.ctypes.data, 0) == 0
        assert [int(v) for v in res] == [fc.EINVAL64, first, 0, 0, 0, 0, 0, 0], (changes, res)
        assert bool((hits == 0xA5A5A5A5A5A5A5A5).all())

    bad([(9, 0, size - 11)], 9)
    bad([(150, 2, size - 1), (150, 3, 2)], 150)
    bad([(193, 0, U64_MAX - 3)], 193)
    bad([(0, 1, U64_MAX)], 0)
    bad([(150, 2, U64_MAX - 1)], 150)
    bad([(190, 1, U64_MAX), (150, 0, size + 1), (101, 3, size + 1), (160, 0, U64_MAX - 3)], 101)
    bad([], 0, base=size)
    bad([], 0, base=U64_MAX - 5)


def test_check_order(cases):
    c = next(c for c in cases if c.name == "n65")
    recs = c.levels[0][0]
    swapped = recs.copy()
    swapped[[30, 31]] = swapped[[31, 30]]
    equal = recs.copy()
    equal[41] = equal[40]
    for r, first in ((swapped, 31), (equal, 41)):
        # after a level of 7 records: the seq counts them
        levels = [(recs[:7], 0), (r, 0)]
        hits, res = zsfile.find(c.src, levels, c.qsrc, c.queries, check_order=True)
        assert [int(v) for v in res.view(np.uint64)] == [fc.EINVAL64, 7 + first, 0, 0, 0, 0, 0, 1]
        _, res = zsfile.find(c.src, levels, c.qsrc, c.queries)
        assert int(res[0]) == 0 and int(res[1]) == len(c.queries)
    # a bounds offence takes precedence, also a later one
    r = swapped.copy()
    r[50, 1] = U64_MAX
    _, res = zsfile.find(c.src, [(r, 0)], c.qsrc, c.queries, check_order=True)
    assert [int(v) for v in res.view(np.uint64)][:2] + [int(res[7])] == [fc.EINVAL64, 50, 0]
    # a descending step across a level boundary is no offence
    _same(fc.FindCase("boundary", c.src, [(recs[30:], 0), (recs[:30], 0)], c.qsrc, c.queries), True)


def test_reference_packed_file():
    img = open(os.path.join(REF, "packed.zs"), "rb").read()
    pairs = zf.packed_records(img)
    (ko, kl, vo, vl), rc = repack.records(img, zsfile.PACKED)
    level = np.stack([ko, kl, vo, vl], axis=1)
    assert len(level) == len(pairs) > 100
    keys = [k for k, _ in pairs]
    assert keys == sorted(set(keys)) and keys == fc.level_keys(img, level, 0)
    # every key is found at its own index, with its value
    hits, res = zsfile.find(img, [(level, 0)], img, level)
    h = hits.view(np.uint64)
    assert h[:, 0].tolist() == [0] * len(keys) and h[:, 1].tolist() == list(range(len(keys)))
    assert h[:, 2:].tolist() == level[:, 2:].tolist()
    assert int(res[2]) + int(res[3]) == len(keys) and int(res[4]) == 0
    # a byte appended, the last byte dropped: the model's lower bound
    near = [k + b"\x00" for k in keys] + [k[:-1] for k in keys if k]
    qsrc, queries = fc.lay_queries(near, residue=5)
    case = fc.FindCase("packed.zs", img, [(level, 0)], qsrc, queries)
    want, wres = case.model()
    assert wres[4] > len(keys)
    _same(case, True)


def test_levels_of_merge_cases_are_sorted():
    """What the cases rest on: a merge case's winners ascend strictly."""
    for c in mc.small_cases():
        keys = fc.level_keys(c.src, fc.sorted_level(c), 0)
        assert all(a < b for a, b in zip(keys, keys[1:])), c.name
