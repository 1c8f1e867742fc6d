"""zscrc_device_records' argument checks and scratch size (no GPU: both return
before any device call)."""
import ctypes

from zeroskip_amd import zsfile
from zeroskip_amd._lib import lib

EINVAL = -1
PTR = 0x10000  # never dereferenced: the calls below fail their argument checks
A, F, P = zsfile.ACTIVE, zsfile.FINALISED, zsfile.PACKED


def _records(size, kind=A, opts=None, flags=0, image=PTR, res=PTR, scratch=None, cap=0, recs=None):
    return lib().zscrc_device_records(image, size, kind, recs, cap, res, scratch,
                                      None if opts is None else ctypes.byref(zsfile.WalkOpts(*opts)), flags, None)


def test_bad_arguments_are_einval():
    assert _records(39) == EINVAL                       # shorter than a header, as zscrc_zs_records
    assert _records(39, F) == EINVAL
    assert _records(55, P) == EINVAL                    # shorter than a header and two short commits
    for kind in (A, F, P):
        assert _records(4096, kind, image=None) == EINVAL
        assert _records(4096, kind, res=None) == EINVAL
        assert _records(4096, kind, cap=4) == EINVAL           # cap > 0 needs the record array
        assert _records(4096, kind, flags=2) == EINVAL         # unknown flag
        assert _records(4096, kind, flags=3) == EINVAL
        assert _records(4096, kind, scratch=PTR + 8) == EINVAL  # scratch not 16-byte aligned
    for kind in (3, -1, 100):
        assert _records(4096, kind) == EINVAL           # unknown kind
        assert zsfile.records_scratch_bytes(4096, kind) == 0


def test_bad_option_pairs():
    # the pairs of tests/test_walk_args.py: the options and their limits are zscrc_device_walk's
    for opts in ((96, 64), (64, 128), (1 << 20, 32), (1 << 20, 1 << 15), (1 << 31, 64), (32, 0)):
        for kind in (A, F, P):
            assert _records(4096, kind, opts) == EINVAL, (opts, kind)
            assert zsfile.records_scratch_bytes(4096, kind, *opts) == 0, (opts, kind)


def test_scratch_bytes_monotone_and_bounded():
    # ACTIVE / FINALISED: the walk's, 8 bytes per 8-byte slot and 16 per block: <= image_size + 24 * blocks
    for block, tile in ((0, 0), (64, 64), (512, 64), (4096, 512), (1 << 30, 16384)):
        bb = block or (1 << 20)
        last = 0
        for size in list(range(40, 300)) + [4095, 4096, 4097, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 5 << 30,
                                            (32 << 30) + 3]:
            need = zsfile.records_scratch_bytes(size, A, block, tile)
            blocks = (size + bb - 1) // bb
            if blocks >= 1 << 24:  # more blocks than one launch has workgroups for: a bad option
                assert need == 0 and _records(size, A, (block, tile)) == EINVAL, (size, block, tile)
                continue
            assert 0 < need <= size + 24 * blocks and need >= last, (size, block, tile)
            assert need == zsfile.records_scratch_bytes(size, F, block, tile) == \
                zsfile.walk_scratch_bytes(size, block, tile)
            last = need


def test_packed_scratch_is_a_few_words():
    last = 0
    for size in (56, 57, 4096, 1 << 20, 5 << 30):
        need = zsfile.records_scratch_bytes(size, P)
        assert 0 < need <= 256 and need % 16 == 0 and need >= last
        last = need
