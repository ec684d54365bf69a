"""CPU: the plain-torch AIS restatement (tests/ais_oracle.py) in float32 against the goldens recorded from the reference's
own ais_trajectory (tests/golden/make_golden_ais.py), and the package's schedules against the reference's values."""
import numpy as np
import pytest
import torch

import ais_oracle as AO
from ais_cases import GOLDENS, golden_chain_inputs, golden_chain_logw
from conftest import load_golden

@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_f32_reproduces_golden(name):
    g = load_golden(name)
    i = golden_chain_inputs(g)
    o = AO.run(i["params"], i["x"], g["schedule"], i["n_sample"], i["z0"], i["v"], i["u"], sign=i["sign"],
               dtype=torch.float32)
    ref_logw = golden_chain_logw(g)
    assert (o["logw"] - ref_logw).abs().max() <= 2e-5 * ref_logw.abs().max()
    nb, L = g["x"].shape[0], int(g["L"])
    ref_z = torch.from_numpy(g["saved_latents"]).reshape(-1, L)  # AIS.py:225 is a plain reshape of the chain-major z
    assert (o["z"] - ref_z).abs().max() <= 2e-4 * ref_z.abs().max()
    np.testing.assert_allclose(o["epsilon"].numpy(), g["epsilon"], rtol=1e-6)
    np.testing.assert_array_equal(o["accept_hist"].numpy(), g["accept_hist"])
    mean = AO.batch_mean(o["logw"], i["n_sample"], i["mode"]).item()
    assert abs(mean - g["means"][0]) <= 2e-5 * abs(g["means"][0])
    assert abs(float(g["saved_ais"]) - g["means"][0]) <= 1e-6 * abs(g["means"][0])
    assert g["saved_latents"].shape == (nb, i["n_sample"], L)


@pytest.mark.parametrize("name", GOLDENS)
def test_schedules_equal_reference(name):
    g = load_golden(name)
    T = len(g["schedule"])
    np.testing.assert_array_equal(AO.linear_schedule(T), g["ref_linear_schedule"])
    np.testing.assert_allclose(np.array(AO.sigmoidial_schedule(T)), g["ref_sigmoidial_schedule"], rtol=0, atol=1e-15)
    import vpc_amd as vpc
    np.testing.assert_array_equal(vpc.ais.linear_schedule(T), g["ref_linear_schedule"])
    np.testing.assert_array_equal(np.array(vpc.ais.sigmoidial_schedule(T)), g["ref_sigmoidial_schedule"])


def test_package_log_mean_exp():
    import vpc_amd as vpc
    t = torch.randn(5, 7, generator=torch.Generator().manual_seed(0)) * 30
    ref = torch.log(torch.mean(torch.exp(t.double()), 1))
    assert torch.allclose(vpc.ais.log_mean_exp(t).double(), ref, rtol=1e-6)
