"""The preparation EnsembleTrainer, EnsembleEvaluator and EnsembleAcquirer share (ensemble._MemberSet and the helpers beside it)
on the MI355X, at the smallest shapes where it can go wrong: obs_dim 5 (rows padded to 8 columns), 17 rows (a second tile with
one valid row), three members.  Everything is compared with torch.equal: the same kernels on the same buffers, so a difference is
a preparation defect (a stride, a padding slot, a stale image), not rounding."""
import pytest
import torch

import vpc_amd as vpc
from vpc_amd import ensemble as E
from vpc_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TP = {"batch_size": 16, "patience": 100}
G, D, L, N, M = 3, 5, 3, 17, 2


def build(params=None):
    m = vpc.Reg_VAE(D, 500, 10, L, TP, "exp", "kl_reg")
    if params is not None:
        m.load_state_dict(params)
    return m.to(DEV)


def test_trainer_evaluator_and_acquirer_share_one_preparation(monkeypatch):
    assert ops.step_small_max_rows() >= N  # the small-batch step is on
    installs = []
    install = E.install_image_stack
    monkeypatch.setattr(E, "install_image_stack", lambda models, *a: installs.append(list(models)) or install(models, *a))
    torch.manual_seed(0)
    ms = [build() for _ in range(G)]
    seeds = [3, 5, 2 ** 40 + 7]
    g = torch.Generator().manual_seed(1)
    x, mask = torch.rand(G, N, D, generator=g).to(DEV), (torch.rand(G, N, D, generator=g) < 0.7).to(DEV)
    mask[:, [0, 16], 0] = False  # every batch (16 rows, 1 row) has an unobserved entry: its rmse is no 0 / 0

    tr = E.EnsembleTrainer(ms, seeds=seeds)
    for _ in range(2):
        tr.step(x, mask, epoch=1)
    ev, acq = tr.evaluator(), E.EnsembleAcquirer(ms, seeds=seeds)
    kw = dict(epoch=1, beta=1.0)
    after = ev.evaluate(x, mask, 16, M, **kw)
    R = M * N
    eps = torch.randn(R, L, generator=g).to(DEV)
    shared = ev.evaluate(x, mask, 16, M, eps=eps, **kw)
    run_eps = torch.randn(5, R, L, generator=g).to(DEV)  # max_steps = 2: 1 + 2 x 2 forward calls
    run_shared = acq.run(x, M, max_steps=2, eps=run_eps)

    # one image stack, the trainer's, read by all three: nobody installed a second one
    assert len(installs) == 1 and all(a is b for a, b in zip(installs[0], ms))
    stack = E.image_stack_of(ms, tr.n_img, tr.dev)
    assert stack is not None and stack[0].data_ptr() == tr.img.data_ptr() and stack[1] == tr.img.stride(0)
    assert ev.img is None and acq.img is None
    assert ev._images()[0].data_ptr() == acq._images()[0].data_ptr() == tr.img.data_ptr()

    # after the two steps the evaluator reads the stepped weights: a fresh evaluator on copies of the members agrees
    copies = [build({k: v.detach().cpu() for k, v in m.state_dict().items()}) for m in ms]
    fresh = E.EnsembleEvaluator(copies, seeds=seeds)
    assert torch.isfinite(after).all() and torch.equal(fresh.evaluate(x, mask, 16, M, **kw), after)
    assert torch.equal(fresh.evaluate(x, mask, 16, M, eps=eps, **kw), shared) and not torch.equal(shared, after)

    # injected eps shared by the members (member stride 0) == the same eps given per member, as an expanded view of the
    # shared one (a member axis whose own stride is 0) and as a dense copy of it
    for per in (lambda t, *shape: t.expand(*shape), lambda t, *shape: t.expand(*shape).contiguous()):
        assert torch.equal(ev.evaluate(x, mask, 16, M, eps=per(eps, G, R, L), **kw), shared)
        for a, b in zip(run_shared, acq.run(x, M, max_steps=2, eps=per(run_eps, G, 5, R, L))):
            assert torch.equal(a, b)
    # the same for the data: one x shared by the members == its expanded view
    assert torch.equal(ev.evaluate(x[0].expand(G, N, D), mask, 16, M, eps=eps, **kw), ev.evaluate(x[0], mask, 16, M, eps=eps, **kw))
    assert torch.isfinite(run_shared[0][:, :, :3]).all() and bool((run_shared[1][:, :, :, :2] >= 0).all())
