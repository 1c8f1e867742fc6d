"""zscrc_zs_records (host) against the format oracle's file_records /
packed_records, on the images of test_record_lister_matches_oracle and on the
three byte patterns where the lister and the walk disagree: the lister's
parser lives in a header it shares with the device lister
(zeroskip_amd/csrc/zscrc_records.h), and this pins what it lists.  CPU only."""
import pytest

from oracle import zs_format as zf
from tests import records_images as ri
from zeroskip_amd import zsfile


def test_finalised_file_matches_oracle():
    img = ri.finalised_300()
    recs, rc = ri.host_records(img, zsfile.FINALISED)
    assert rc == zsfile.END and ri.as_pairs(img, recs) == zf.file_records(img)
    assert any(v is None for _, v in ri.as_pairs(img, recs))


def test_wellformed_active_matches_oracle():
    img = ri.wellformed()
    recs, rc = ri.host_records(img, zsfile.ACTIVE)
    assert rc == zsfile.END and ri.as_pairs(img, recs) == zf.file_records(img)


def test_packed_file_matches_oracle():
    img, want = ri.packed_400()
    recs, rc = ri.host_records(img, zsfile.PACKED)
    assert rc == 0 and ri.as_pairs(img, recs) == zf.packed_records(img) == want
    img, want = ri.packed_long_value_70k()
    recs, rc = ri.host_records(img, zsfile.PACKED)
    assert rc == 0 and ri.as_pairs(img, recs) == zf.packed_records(img) == want
    img, want = ri.packed_small(0)
    recs, rc = ri.host_records(img, zsfile.PACKED)
    assert rc == 0 and len(recs) == 0 and zf.packed_records(img) == []


@pytest.mark.parametrize("which", range(3), ids=["commit_span", "voff_16", "klen_room"])
def test_disagreement_images(which):
    """The lister lists the oracle's records up to the crafted record and ends
    as the builders say (they assert the host walk's differing result)."""
    name, img, at, want_rc = ri.disagreement_images()[which]
    recs, rc = ri.host_records(img, zsfile.ACTIVE)
    oracle = zf.file_records(img)
    assert rc == want_rc, name
    if rc == zsfile.END:
        assert ri.as_pairs(img, recs) == oracle and len(recs) == 4, name
    else:
        # every listed record lies before the crafted one; the oracle, which checks no room, reads on
        assert ri.as_pairs(img, recs) == oracle[:len(recs)] and len(oracle) > len(recs), name
        assert all(int(r[0]) < at for r in recs), name
        # cut before the crafted record the image lists the same records and ends
        cut, rc2 = ri.host_records(img[:at], zsfile.ACTIVE)
        assert rc2 == zsfile.END and cut.tolist() == recs.tolist(), name


def test_capped_listing_reports_every_record():
    img = ri.wellformed()
    recs, _ = ri.host_records(img, zsfile.ACTIVE)
    for cap in (0, 1, len(recs) - 1, len(recs), len(recs) + 1):
        got, rc, n = ri.host_records_capped(img, zsfile.ACTIVE, cap)
        assert n == len(recs) and rc == (zsfile.OVERFLOW if cap < n else zsfile.END)
        assert got.tolist() == recs[:cap].tolist()
