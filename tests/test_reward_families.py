"""Active-variable-selection reward (BASELINE config 5) for the encoder families beyond the plain Reg_VAE / vanilla_VAE
with <= 128 columns: EDDI (point-net encoder), mask-augmented encoders ([x*mask | mask]) and wide encoders (obs_dim > 128).

CPU: the oracle's reward_matrix (evaluate.py:424-433, 514-634 restated) with EDDIPort, TorchPort(mask_augm=True) and
TorchPort at d = 129 against the reference's own R_lindley_chain (tests/golden/make_golden_reward_families.py).
GPU: vpc.reward_matrix (vpc_reward_matrix_ex) against the same vectors, against the oracle on larger shapes with briefly
trained weights, inside active_learning_func, after parameter writes, and the guards of the plain path.  The rewards are
differences of O(1) KL terms that cancel to ~1e-4, so the tolerances are absolute (tests/test_reward.py).
"""
import os

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from conftest import golden_params, load_golden
from oracle import eddi_oracle as EO
from oracle import vae_oracle as O

L = 10
TP = {"batch_size": 64, "patience": 100}
FIXTURES = {"eddi": "reward_eddi_d14.npz", "vaemask": "reward_vaemask_d14.npz", "d129": "reward_d129.npz"}


def _t(a, dev="cpu"):
    return torch.from_numpy(np.array(a)).to(dev)


def _port(family, params, Ld=L):
    if family == "eddi":
        return EO.EDDIPort(params, Ld)
    return O.TorchPort(params, Ld, mask_augm=family == "vaemask")


def _new_model(family, d, reg=True, K=10, Ld=L):
    if family == "eddi":
        return vpc.Reg_EDDI(d, 500, K, Ld, TP, "exp", "kl_reg") if reg else vpc.vanilla_EDDI(d, 500, K, Ld, TP, "exp")
    if family == "vaemask":
        return vpc.Reg_VAE_mask(d, 500, 10, Ld, TP, "exp", "kl_reg") if reg else vpc.vanilla_VAE_mask(d, 500, 10, Ld, TP, "exp")
    return vpc.Reg_VAE(d, 500, 10, Ld, TP, "exp", "kl_reg") if reg else vpc.vanilla_VAE(d, 500, 10, Ld, TP, "exp")


def _golden_model(family, g):
    d = g["x"].shape[1]
    m = _new_model(family, d)
    sd = m.state_dict()
    sd.update({k: v.clone() for k, v in golden_params(g).items()})
    m.load_state_dict(sd)
    return m.cuda()


def _data(rows, d, seed):
    """Rows whose columns share a few factors: revealing a feature tells something about the target (last column)."""
    g = torch.Generator().manual_seed(seed)
    base, mix = torch.rand(rows, 4, generator=g), torch.rand(4, d, generator=g)
    data = torch.sigmoid(3.0 * (base @ mix / mix.sum(0) - 0.5)) + 0.05 * torch.rand(rows, d, generator=g)
    return (data - data.min(0).values) / (data.max(0).values - data.min(0).values)


def _train(m, data, steps, seed=0):
    """A brief training run on the API path (model.forward / model.loss / backward / Adam): the rewards of a freshly
    initialised encoder are fp32 round-off."""
    g = torch.Generator().manual_seed(seed)
    x = data.cuda()
    B, d = x.shape
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=3e-3)
    reg = hasattr(m, "reg_type")
    for s in range(steps):
        mt = (torch.rand(B, d, generator=g) < 0.7).cuda()
        if reg:
            mp = mt & (torch.rand(B, d, generator=g) < 0.7).cuda()
            o = m.forward(x, mt, mp, "train")
            _, tl = m.loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mt, mp, s + 1, alpha=1.0)
        else:
            mf = mt.float()
            o = m.forward(x, mf)
            _, tl = m.loss(x, o[2], o[3], o[0], o[1], s + 1, mf)
        opt.zero_grad()
        tl.backward()
        opt.step()
    return m


def _params(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if "prior" not in k}


def _inputs(n, d, M, seed):
    g = torch.Generator().manual_seed(seed)
    x = _data(n, d, seed + 1)
    mask = (torch.rand(n, d, generator=g) < 0.5).float()
    mask[:, -1] = (torch.rand(n, generator=g) < 0.4).float()
    im = torch.rand(M, n, d, generator=g)
    return x, mask, im


def _check(R, want, atol=2e-6, min_scale=1e-4):
    assert np.array_equal(R == -1e4, want == -1e4)
    live = want != -1e4
    scale = np.max(np.abs(want[live]))
    assert scale > min_scale  # a trained encoder: rewards well above round-off
    err = np.max(np.abs(R[live] - want[live]))
    assert err <= atol + 1e-3 * scale, (err, scale)


# ------------------------------------------------------------------------------------------------ CPU: oracle vs reference
@pytest.mark.parametrize("family", list(FIXTURES))
@pytest.mark.parametrize("tag", ["t0", "t1"])
def test_oracle_reward_family_matches_reference(family, tag):
    g = load_golden(FIXTURES[family])
    port = _port(family, golden_params(g))
    x, mask, im = _t(g["x"]), _t(g[f"mask_{tag}"]), _t(g["im"])
    with torch.no_grad():
        R = O.reward_matrix(port, x, mask, im.shape[0], im)
        k1, k2 = O.chaini_I(port, x, mask, 3), O.chaini_II(port, x, mask, 3)
    want = g[f"R_{tag}"]
    assert np.array_equal(R.numpy() == -1e4, want == -1e4)
    assert np.max(np.abs(want[want != -1e4])) > 1e-3
    assert np.max(np.abs(R.numpy() - want)) <= 2e-7
    assert np.max(np.abs(k1.numpy() - g[f"kl1_{tag}"])) <= 2e-7 and np.max(np.abs(k2.numpy() - g[f"kl2_{tag}"])) <= 2e-7


# ------------------------------------------------------------------------------------------------ GPU: against the reference
@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FIXTURES))
@pytest.mark.parametrize("tag", ["t0", "t1"])
def test_gpu_reward_family_matches_reference(family, tag):
    g = load_golden(FIXTURES[family])
    m = _golden_model(family, g)
    x, mask, im = _t(g["x"], "cuda"), _t(g[f"mask_{tag}"], "cuda"), _t(g["im"], "cuda")
    R = vpc.reward_matrix(m, x, mask, im).cpu().numpy()
    want = g[f"R_{tag}"]
    assert np.array_equal(R == -1e4, want == -1e4)
    live = want != -1e4
    tol = 5e-7 + 1e-3 * np.max(np.abs(want[live]))
    assert np.max(np.abs(R[live] - want[live])) <= tol
    # drop-in single-candidate call with the reference's signature
    for u in (3, x.shape[1] - 2):
        loc = np.where(g[f"mask_{tag}"][:, u] == 0)[0]
        r1 = vpc.R_lindley_chain(u, x, mask, im.shape[0], m, im, loc).cpu().numpy()
        assert np.max(np.abs(r1 - want[loc, u])) <= tol


# ------------------------------------------------------------------------------------------------ GPU: against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("reg,d,K,n,M", [(True, 128, 10, 6, 7), (False, 128, 10, 5, 50), (True, 128, 32, 7, 17),
                                         (False, 128, 32, 3, 7), (True, 40, 32, 13, 50)])
def test_gpu_reward_eddi_vs_oracle(reg, d, K, n, M):
    torch.manual_seed(d + K)
    m = _train(_new_model("eddi", d, reg, K).cuda(), _data(256, d, 7), 60)
    x, mask, im = _inputs(n, d, M, d + K + n)
    with torch.no_grad():
        want = O.reward_matrix(EO.EDDIPort(_params(m), L), x, mask, M, im).numpy()
    R = vpc.reward_matrix(m, x.cuda(), mask.cuda(), im.cuda()).cpu().numpy()
    _check(R, want)


@pytest.mark.gpu
@pytest.mark.parametrize("reg,d,n,M", [(True, 64, 9, 17), (False, 64, 6, 50), (True, 100, 6, 7), (False, 100, 5, 17)])
def test_gpu_reward_mask_augm_vs_oracle(reg, d, n, M):
    torch.manual_seed(d + n)
    m = _train(_new_model("vaemask", d, reg).cuda(), _data(256, d, 8), 60)
    assert m._wide == (2 * d > 128)
    x, mask, im = _inputs(n, d, M, d + n)
    with torch.no_grad():
        want = O.reward_matrix(O.TorchPort(_params(m), L, mask_augm=True), x, mask, M, im).numpy()
    R = vpc.reward_matrix(m, x.cuda(), mask.cuda(), im.cuda()).cpu().numpy()
    _check(R, want)


@pytest.mark.gpu
@pytest.mark.parametrize("reg,d,n,M", [(True, 129, 10, 50), (False, 200, 7, 17), (True, 1000, 5, 7)])
def test_gpu_reward_wide_vs_oracle(reg, d, n, M):
    torch.manual_seed(d + n)
    m = _train(_new_model("d129", d, reg).cuda(), _data(256, d, 9), 60)
    assert m._wide
    x, mask, im = _inputs(n, d, M, d + n)
    with torch.no_grad():
        want = O.reward_matrix(O.TorchPort(_params(m), L), x, mask, M, im).numpy()
    R = vpc.reward_matrix(m, x.cuda(), mask.cuda(), im.cuda()).cpu().numpy()
    if d < 1000:
        _check(R, want)
    else:  # one feature of a thousand moves the posterior little: rewards ~5e-5, so a tighter absolute bound
        _check(R, want, atol=5e-7, min_scale=2e-5)


# ------------------------------------------------------------------------------------------------ GPU: the loop
@pytest.mark.gpu
@pytest.mark.parametrize("family,d,n,M", [("d129", 129, 17, 8), ("eddi", 40, 19, 8)])
def test_gpu_loop_families_vs_oracle(family, d, n, M, tmp_path, monkeypatch):
    """The first 3 acquisition steps of active_learning_func, the forward passes REPLAYED into both loops (one seeded stream
    of the oracle's decoder outputs), against the oracle's restatement of the loop: identical acquisitions."""
    monkeypatch.chdir(tmp_path)
    steps = 3
    torch.manual_seed(5)
    data = _data(n + 512, d, 21)
    m = _train(_new_model(family, d).cuda(), data[n:], 100)
    port = _port(family, _params(m))
    x = data[:n].clone()
    tmask = torch.rand(n, d, generator=torch.Generator().manual_seed(2)) < 0.7

    def replay(seed):  # one model.forward: x_mean_q of the oracle's port under a seeded eps stream
        gg = torch.Generator().manual_seed(seed)

        def fwd(mask):
            eps = torch.randn(n, L, generator=gg)
            with torch.no_grad():
                z, _, _ = port.encoder(x, (mask.cpu() > 0.5).float(), eps=eps)
                return port.decoder(z)[0]
        return fwd

    with torch.no_grad():
        ref = O.active_learning_loop(x, M, replay(5), lambda xx, mm, im: O.reward_matrix(port, xx, mm, M, im), max_steps=steps)
    vae_type = "reg_EDDI1" if family == "eddi" else "reg_vae1"
    out = vpc.active_learning_func(None, x, tmask, 30, d, 500, 10, M, L, "toy", TP, "exp", vae_type, 100, 1, 1, alpha=1.0,
                                   p_missingness=30, reg_type="kl_reg", Repeat=1, model=m, _forward=replay(5),
                                   max_steps=steps, save=False)
    R, want = out["R_hist_CHAI"][0, :steps].numpy(), ref["R_hist"].numpy()
    live = want != -1e4
    scale = np.max(np.abs(want[live]))
    assert scale > 1e-3
    assert np.array_equal(R == -1e4, ~live)
    assert np.max(np.abs(R[live] - want[live])) <= 1e-4 * scale + 5e-7, (np.max(np.abs(R[live] - want[live])), scale)
    assert np.array_equal(out["action_CHAI"][0, :, :steps].numpy(), ref["action"].numpy())
    assert np.array_equal(out["im_CHAI"][0, :steps].numpy(), ref["im"].numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("vae_type", ["reg_EDDI1", "reg_vae_mask_augm1"])
def test_gpu_loop_families_end_to_end(vae_type, tmp_path, monkeypatch):
    """The product path through model_loader('test'): a briefly trained checkpoint in the reference's naming, model.forward
    on the GPU.  RNG-dependent, so properties only: every row acquires d - 1 distinct features and the information curve
    ends well below its start."""
    monkeypatch.chdir(tmp_path)
    d, n, M = 14, 24, 10
    torch.manual_seed(9)
    data = _data(n + 256, d, 31)
    m = _train(_new_model("eddi" if "EDDI" in vae_type else "vaemask", d).cuda(), data[n:], 300)
    ck = vpc.checkpoint_path("exp", "toy", vae_type, 30, alpha=1.0, p_missingness=30, reg_type="kl_reg")
    os.makedirs(os.path.dirname(ck), exist_ok=True)
    torch.save({k: v.cpu() for k, v in m.state_dict().items()}, ck)
    x, tmask = data[:n].clone(), torch.rand(n, d, generator=torch.Generator().manual_seed(4)) < 0.7
    out = vpc.active_learning_func(None, x, tmask, 30, d, 500, 10, M, L, "toy", TP, "exp", vae_type, 100, 1, 1, alpha=1.0,
                                   p_missingness=30, reg_type="kl_reg", Repeat=2)
    act = out["action_CHAI"].numpy()
    assert act.shape == (2, n, d - 1)
    for r in range(2):
        for row in act[r]:
            assert sorted(row.astype(int)) == list(range(d - 1))
    curve = out["information_curve_CHAI"][:, 0].numpy()
    assert np.all(curve[:, -1] < 0.5 * curve[:, 0])
    for f in vpc.active_result_paths("exp", "toy", vae_type, 30, 1.0, 30, "kl_reg").values():
        assert os.path.exists(f)


# ------------------------------------------------------------------------------------------------ GPU: freshness and guards
@pytest.mark.gpu
def test_gpu_reward_wide_follows_parameter_writes():
    d, n, M = 129, 6, 7
    torch.manual_seed(1)
    m = _train(_new_model("d129", d).cuda(), _data(256, d, 3), 40)
    x, mask, im = _inputs(n, d, M, 77)
    R0 = vpc.reward_matrix(m, x.cuda(), mask.cuda(), im.cuda()).cpu().numpy()
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.5)
        want = O.reward_matrix(O.TorchPort(_params(m), L), x, mask, M, im).numpy()
    R1 = vpc.reward_matrix(m, x.cuda(), mask.cuda(), im.cuda()).cpu().numpy()
    assert not np.allclose(R0, R1)
    live = want != -1e4
    assert np.array_equal(R1 == -1e4, ~live)
    assert np.max(np.abs(R1[live] - want[live])) <= 2e-6 + 1e-3 * np.max(np.abs(want[live]))


@pytest.mark.gpu
def test_gpu_plain_reward_unchanged():
    """The plain Reg_VAE at d = 128 still runs the original entry point: bitwise the result of a direct call."""
    import ctypes as C

    from vpc_amd._lib import check, lib, ptr, stream_ptr
    d, n, M = 128, 37, 19
    torch.manual_seed(2)
    m = _train(_new_model("d129", d).cuda(), _data(256, d, 4), 20)
    x, mask, im = [t.cuda() for t in _inputs(n, d, M, 5)]
    R = vpc.reward_matrix(m, x, mask, im)
    sizes = [C.c_long() for _ in range(3)]
    check(lib().vpc_reward_scratch(n, d, M, *[C.byref(s) for s in sizes]), "vpc_reward_scratch")
    pre, stat, w1t = (torch.empty(s.value, device="cuda") for s in sizes)
    R_old = torch.empty(n, d - 1, device="cuda")
    w1, b1 = m.trainable()[0], m.trainable()[1]
    check(lib().vpc_reward_matrix(ptr(x), ptr(mask.to(torch.uint8)), ptr(im), ptr(w1.data), ptr(b1.data), ptr(m._enc_img()),
                                  ptr(pre), ptr(stat), ptr(w1t), ptr(R_old), n, d, L, M, stream_ptr()), "vpc_reward_matrix")
    assert torch.equal(R, R_old)


@pytest.mark.gpu
def test_gpu_reward_wide_latent16_refused():
    m = vpc.Reg_VAE(129, 500, 10, 16, TP, "exp", "kl_reg").cuda()
    x, mask, im = [t.cuda() for t in _inputs(4, 129, 3, 6)]
    with pytest.raises(vpc.VpcError):
        vpc.reward_matrix(m, x, mask, im)
