"""model.forward_loss against the reference's forward -> loss call written out by hand (tests/family_cases.py), one case per
model class: equal seeds, every tensor of forward's tuple and of loss's return exactly equal.  Once with the training
keywords (train.py) and once as the evaluation loops call it (llh_eval=True, stage='evaluate'; evaluate.py).
Shapes: 16 rows, d = 14, L = 10; the image-width EDDI classes 4 rows of d = 784; the flows d = 12."""
import pytest
import torch

import family_cases as F

pytestmark = pytest.mark.gpu

TRAIN = dict(epoch=3, alpha=0.5, beta=0.7, beta_annealing=True, alpha_annealing=True, stage="train")
EVAL = dict(epoch=100, alpha=0.5, beta=0.7, beta_annealing=True, alpha_annealing=True, stage="evaluate")


@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_forward_loss_is_the_reference_sequence(name):
    make, reference_call, d, B = F.FAMILIES[name]
    torch.manual_seed(0)
    m = make(d).cuda()
    mnar = "notMIWAE" in name
    (x, mask), = F.batches(1, B, d, seed=1, float_mask=mnar)
    keep = torch.rand(B, d, generator=torch.Generator().manual_seed(2)).cuda() < 0.7
    mask_p = mask * keep  # (float for the MNAR classes, as the harness hands it to them)
    for kw, extra in ((TRAIN, {}), (EVAL, {"llh_eval": True})):
        torch.manual_seed(11)
        o_ref, out_ref = reference_call(m, x, mask, mask_p, **kw, **extra)
        torch.manual_seed(11)
        o, out = m.forward_loss(x, mask, mask_p if m.regularised else None, **kw, **extra)
        F.same(o_ref, o, (name, "forward", kw["stage"]))
        F.same(out_ref, out, (name, "loss", kw["stage"]))
        assert len(out) == (2 if not extra else 3 if ("MIWAE" in name) else 4)
        assert torch.isfinite(out[1]).all()
