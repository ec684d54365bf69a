"""CPU: the condition tests/test_miwae_small_gpu.py relies on for its edge shapes, on the float64 oracle alone (as
tests/test_miwae_oracle.py::test_trainer_case_seeds_keep_the_kink_band_small for the trainer cases)."""
import pytest
import torch

import miwae_cases as C
import miwae_oracle as O
import miwae_small_cases as SC


@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("shape", SC.EDGE_SHAPES)
def test_edge_case_seeds_keep_the_kink_band_small(shape, kind):
    """At most 1e-4 of the hidden units (rounded up) have a float64 pre-activation within KINK_BAND of their layer's max,
    the cases with zeroed mask rows included."""
    p, x, m, mp, eps = C.oracle_inputs(SC.edge_case(shape, kind))
    stats = O.new_gate_stats()
    with torch.no_grad():
        O.run(p, x, m, mp, eps, C.ALPHA, stats=stats)
    B, S = shape[:2]
    assert stats["units"] == (2 if kind == "reg" else 1) * (B + B * S) * 2 * C.HID
    assert stats["in_band"] <= C.band_limit(stats["units"]), stats


def test_empty_rows_case_has_empty_rows():
    c = SC.edge_case(SC.EMPTY_ROWS_SHAPE, "reg")
    assert not c["mask"][3].any() and not c["mask_p"][3].any() and not c["mask_p"][7].any()
    assert c["mask"][7].any() and C.model_case(*SC.EMPTY_ROWS_SHAPE, True, SC.SEED)["mask"][3].any()


def test_row_limit_variable(monkeypatch):
    import vpc_amd
    from vpc_amd import miwae
    monkeypatch.delenv("VPC_MIW_SMALL", raising=False)
    assert miwae.small_max_rows() == 0
    monkeypatch.setenv("VPC_MIW_SMALL", "2560")
    assert miwae.small_max_rows() == 2560
    monkeypatch.setenv("VPC_MIW_SMALL", "many")
    with pytest.raises(vpc_amd.VpcError, match="VPC_MIW_SMALL"):
        miwae.small_max_rows()
