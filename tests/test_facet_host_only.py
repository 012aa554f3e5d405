"""A facet is resolved on the snapshot's device: a host-only snapshot answers PS_ENODEVICE (no GPU needed)."""
import pytest

import probly_search_amd as psa


def test_facet_needs_a_device_snapshot():
    idx = psa.Index(1)
    idx.add_field_values(0, ["a b c"])
    with pytest.raises(psa.PsError) as e:
        idx.snapshot(device=-1).facet([0], [2])
    assert e.value.status == psa._lib.PS_ENODEVICE
