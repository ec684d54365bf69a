"""CPU: the decoder-generic AIS restatement (tests/ais_family_oracle.py) in float64 against the goldens recorded from the
reference's own ais_trajectory on its own MNAR, flow, wide and latent-20 models (tests/golden/make_golden_ais_families.py),
its identity with tests/ais_oracle.py on the dense chain, and the figures recorded next to the cases."""
import numpy as np
import pytest
import torch

import ais_cases as AC
import ais_family_cases as FC
import ais_family_oracle as FO
import ais_oracle as AO
from conftest import load_golden


@pytest.mark.parametrize("name", FC.GOLDENS)
def test_oracle_f64_reproduces_golden(name):
    g = load_golden(name)
    i = FC.golden_chain_inputs(g)
    o = FC.golden_oracle(g, torch.float64)
    ref_logw = FC.golden_chain_logw(g).double()
    assert (o["logw"] - ref_logw).abs().max() <= 2e-5 * ref_logw.abs().max()
    nb, L = g["x"].shape[0], int(g["L"])
    ref_z = torch.from_numpy(g["saved_latents"]).reshape(-1, L).double()  # AIS.py:225: a plain reshape of the chain-major z
    assert (o["z"] - ref_z).abs().max() <= 2e-4 * ref_z.abs().max()
    np.testing.assert_allclose(o["epsilon"].numpy(), g["epsilon"], rtol=1e-6)
    np.testing.assert_array_equal(o["accept_hist"].numpy(), g["accept_hist"])
    mean = AO.batch_mean(o["logw"], i["n_sample"], i["mode"]).item()
    assert abs(mean - g["means"][0]) <= 2e-5 * abs(g["means"][0])
    assert abs(float(g["saved_ais"]) - g["means"][0]) <= 1e-6 * abs(g["means"][0])
    assert g["saved_latents"].shape == (nb, i["n_sample"], L)


def test_goldens_fit_the_size_limit():
    import os
    from conftest import GOLDEN
    for name in FC.GOLDENS:
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= 956 * 1024


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("name", ["a", "d"])
def test_dense_description_equals_ais_oracle_bitwise(name, sign, dtype):
    i = AC.inputs(name)
    ref = AO.run(i["params"], i["x"], i["schedule"], i["n_sample"], i["z0"], i["v"], i["u"], sign=sign, dtype=dtype,
                 init_step_size=i["step"])
    got = FO.run(FO.dense(i["params"], AO.X_LOGVAR), i["x"], i["schedule"], i["n_sample"], i["z0"], i["v"], i["u"],
                 sign=sign, dtype=dtype, init_step_size=i["step"])
    for k in ("logw", "z", "epsilon", "accept_hist", "accept", "prob", "margin"):
        assert torch.equal(ref[k], got[k]), k
    assert ref["clamped"] == got["clamped"]


def test_all_ones_mask_is_no_mask():
    i = FC.inputs("mnar14")
    o = FC.oracle("mnar14")
    m = FO.run(i["desc"], i["x"], i["schedule"], i["n_sample"], i["z0"], i["v"], i["u"], sign=i["sign"],
               init_step_size=i["step"], mask=torch.ones_like(i["x"]))
    for k in ("logw", "z", "epsilon", "accept_hist"):
        assert torch.equal(o[k], m[k])
    assert not torch.equal(o["logw"], FC.oracle("mnar14_mask")["logw"])


@pytest.mark.parametrize("name", list(FC.CASES))
def test_case_figures_are_the_recorded_ones(name):
    """The margin of a case is 4 x the measured fp32-vs-fp64 probability difference of this restatement, its seed leaves the
    float64 oracle no excluded decision, the fp32 restatement flips none, and both branches of accept / reject run."""
    c = FC.CASES[name]
    dp, e_logw, e_z, flips, rate, min_margin = FC.fp32_vs_fp64(name)
    m_dp, m_logw, m_z, m_rate = FC.MEASURED[name]
    print(f"{name}: dp {dp:.3e} logw {e_logw:.2e} z {e_z:.2e} flips {flips} rate {rate:.3f} min margin {min_margin:.2e}")
    assert dp <= 1.02 * m_dp and c["margin"] >= 4 * dp and c["margin"] <= 4.1 * m_dp
    assert min_margin >= c["margin"] and flips == 0
    assert 0.0 < rate < 1.0 and abs(rate - m_rate) <= 0.01
    b_logw, b_z = c.get("bounds", (2e-5, 2e-4))
    assert e_logw <= b_logw and e_z <= b_z
    if "bounds" in c:  # 4 x the measured error of the fp32 restatement, which misses at least one project bound here
        assert e_logw > 2e-5 or e_z > 2e-4
        assert b_logw <= 4.1 * m_logw and b_z <= 4.1 * m_z and e_logw <= 1.02 * m_logw and e_z <= 1.02 * m_z
    if "grad_clip" in c:
        assert FC.oracle(name)["clamped"] >= 1
