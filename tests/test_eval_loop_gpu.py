"""eval_vae (evaluate.py:136-297) and eval_vae_mnar (evaluate.py:13-69) against the same quantities computed by a loop written
out here with the reference's positional order (tests/family_cases.py): equal seeds, M = 2, one batch of 16 rows, exact."""
import pytest
import torch

import family_cases as F
import vpc_amd as vpc
from vpc_amd import harness

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
M, P_MISS, EPOCHS = 2, 30, 100
HYPER = dict(alpha=0.5, beta=0.7, beta_annealing=True, alpha_annealing=True, stage="evaluate")


def _seed():
    torch.manual_seed(7)
    harness._seed_counter[0] = 0


@pytest.mark.parametrize("vae_type,cls", [("reg_vae1", "Reg_VAE"), ("vanilla_vae1", "vanilla_VAE")])
def test_eval_vae_is_the_reference_loop(vae_type, cls):
    make, reference_call, d, B = F.FAMILIES[cls]
    torch.manual_seed(0)
    model = make(d).to(DEV)
    loader = F.batches(1, B, d, seed=4)
    _seed()
    got = vpc.eval_vae([(loader, "test")], 30, d, 500, 10, M, F.L, "toy", F.TP, "exp", vae_type, EPOCHS, 1, 1, device=DEV,
                       p_missingness=P_MISS, reg_type="kl_reg", model=model, save=False, **HYPER)["test"]
    _seed()
    recon, res, res_negll, res_negll_imp = [], [], [], []
    with torch.no_grad():
        for _ in range(M):
            for x, mask in loader:  # (one batch: the means over the batches are means of one value)
                mask_p = vpc.create_missing_uci(x.shape, P_MISS, device=DEV) * mask if cls == "Reg_VAE" else None
                o, (_, train_loss, negl, negl_imp) = reference_call(model, x, mask, mask_p, epoch=EPOCHS, llh_eval=True, **HYPER)
                x_mean = o[6] if cls == "Reg_VAE" else o[2]  # evaluate.py:210, :219: the q pass's reconstruction mean
                inv = ~mask
                recon.append(torch.stack([torch.sqrt(torch.sum(torch.square(torch.squeeze(x_mean) * inv - x * inv))
                                                     / torch.sum(inv))]).mean())
                res.append(torch.mean(torch.stack([train_loss])))
                res_negll.append(torch.mean(torch.stack([torch.as_tensor(negl, device=DEV, dtype=torch.float32)])))
                res_negll_imp.append(torch.mean(torch.stack([torch.as_tensor(negl_imp, device=DEV, dtype=torch.float32)])))
    want = dict(rmse=torch.stack(recon).mean(), elbo=torch.stack(res).mean(), negll=torch.stack(res_negll).mean(),
                negll_imp=torch.stack(res_negll_imp).mean())
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.isfinite(v) and torch.equal(got[k], v.cpu()), (k, got[k], v)


def test_eval_vae_mnar_is_the_reference_loop():
    make, reference_call, d, B = F.FAMILIES["REG_notMIWAE_v2"]
    torch.manual_seed(0)
    model = make(d).to(DEV)
    (x, mask), = F.batches(1, B, d, seed=4, float_mask=True)
    _seed()
    got = vpc.eval_vae_mnar(x, mask, 50, d, 500, 10, M, F.L, "toy", F.TP, "exp", "reg_notMIWAE1", EPOCHS, 5, 1, device=DEV,
                            p_missingness=P_MISS, reg_type="kl_reg", model=model, save=False, **HYPER)
    _seed()
    recon = []
    with torch.no_grad():
        for _ in range(M):
            mask_p = vpc.create_missing_uci(x.shape, P_MISS, device=DEV).float() * mask
            _, (xm, _, _) = reference_call(model, x, mask, mask_p, epoch=EPOCHS, llh_eval=True, **HYPER)
            inv = 1 - mask
            recon.append(torch.sqrt(torch.sum(torch.square(xm * inv - x * inv)) / torch.sum(inv)))
    want = torch.stack(recon).mean().cpu()
    assert torch.isfinite(want) and torch.equal(got, want), (got, want)
