"""The ensemble step of the mask-augmented and point-net members on the host (ensemble.MaskEnsembleTrainer / EDDIEnsembleTrainer;
vpc_step_small_multi_aug_f32, vpc_step_small_multi_eddi_f32, vpc_reduce_step_adam_eddi_multi).  No GPU: the exported symbols, the
refusals of the three C entries (dummy pointers, nothing launched), the validation of the two classes and the routing of
harness.train_sweep with stub trainers."""
import ctypes

import pytest
import torch

import vpc_amd as vpc
from vpc_amd import ensemble as E
from vpc_amd import harness as H
from vpc_amd import ops

ERR_ARG, ERR_SHAPE = 1, 2
TP = {"batch_size": 16, "patience": 1}
L = 10


def mask_reg(d=12, rt="kl_reg", Ld=L):
    return vpc.Reg_VAE_mask(d, 500, 10, Ld, TP, "e", rt)


def mask_van(d=12):
    return vpc.vanilla_VAE_mask(d, 500, 10, L, TP, "e")


def eddi_reg(d=12, K=10, rt="kl_reg", Ld=L):
    return vpc.Reg_EDDI(d, 500, K, Ld, TP, "e", rt)


def eddi_van(d=12, K=10):
    return vpc.vanilla_EDDI(d, 500, K, L, TP, "e")


# ------------------------------------------------------------------ the library
def test_new_symbols_are_exported():
    h = ctypes.CDLL(vpc.LIB_PATH)
    for name in ("vpc_step_small_multi_aug_f32", "vpc_step_small_multi_eddi_f32", "vpc_reduce_step_adam_eddi_multi"):
        assert hasattr(h, name), name
        assert name in vpc._lib.exported_symbols()
    assert (ops.MS_PARTF, ops.MS_SNAP, ops.MS_COUNT_FAMILIES) == (ops.MS_COUNT, ops.MS_COUNT + 1, ops.MS_COUNT + 2)
    assert ops.MS_COUNT == 9  # the existing entries keep their nine strides


def _strides(over=()):
    """Member strides that hold every slice of B <= 32, pitch 64, K = 32, three planes, ONE tile's blocks."""
    lay = vpc._lib.pointnet_layout(12, 10, L)
    v = {ops.MS_X: 32 * 64, ops.MS_MASK: 32 * 64, ops.MS_MASK_P: 32 * 64, ops.MS_EPS: 3 * 32 * 16, ops.MS_IMG: 65536,
         ops.MS_PARTE: lay.enc_part, ops.MS_PARTD: lay.dec_part, ops.MS_LOSS: 8, ops.MS_PARAM: 65536,
         ops.MS_PARTF: 2 * 32 * 64, ops.MS_SNAP: 4096}
    v.update(dict(over))
    return (ctypes.c_long * ops.MS_COUNT_FAMILIES)(*ops.stride_vector(ops.MS_COUNT_FAMILIES, v))


def test_c_entries_refuse_before_any_launch():
    """Host buffers and no device: every refusal is returned by the argument checks.  (Every call below is one the entries
    refuse: a call that passed the checks would launch on these dummy pointers.)"""
    l = vpc._lib.lib()
    host = (ctypes.c_float * 96)()
    p = ctypes.c_void_p((ctypes.addressof(host) + 63) // 64 * 64)  # (the entries check 16-byte alignment before the strides)

    def aug(d, d_real, Ld=L, G=2, B=16, draw=0, strides=None):
        return l.vpc_step_small_multi_aug_f32(p, p, p, p, p, p, p, G, 2, 2, draw, 0, 0, 1.0, 0.0, p, p, p, strides or _strides(), B,
                                              d, d_real, Ld, 0, None)

    def pn(d, d_real, K=10, Ld=L, G=2, B=16, draw=0, strides=None, front=p):
        return l.vpc_step_small_multi_eddi_f32(p, p, p, p, p, p, p, G, 2, 2, draw, 0, 0, 1.0, 0.0, p, p, p, strides or _strides(), B,
                                               d, d_real, Ld, K, front, p, p, 0, None)

    # ---- VPC_ERR_SHAPE
    assert aug(68, 65) == ERR_SHAPE and aug(68, 68) == ERR_SHAPE      # 2 d_real > 128 (and pitch 68)
    assert pn(12, 12, K=33) == ERR_SHAPE                               # K = 33
    assert pn(68, 68) == ERR_SHAPE and pn(68, 65) == ERR_SHAPE         # pitch 68
    assert aug(16, 12) == ERR_SHAPE and pn(16, 12) == ERR_SHAPE        # pitch - d_real = 4
    assert aug(12, 12, Ld=16) == ERR_SHAPE and pn(12, 12, Ld=16) == ERR_SHAPE
    many = vpc.ensemble.MAX_BLOCKS // 2 + 1                            # G x tiles > VPC_MULTI_MAX_BLOCKS (B = 32: two tiles)
    big = dict(G=many, B=32, strides=_strides({ops.MS_PARTE: 1 << 20, ops.MS_PARTD: 1 << 20, ops.MS_LOSS: 16,
                                                 ops.MS_PARTF: 1 << 20}))
    assert aug(12, 12, **big) == ERR_SHAPE and pn(12, 12, **big) == ERR_SHAPE
    # ---- VPC_ERR_ARG
    assert pn(12, 12, front=None) == ERR_ARG
    lay = vpc._lib.pointnet_layout(12, 10, L)
    short = _strides({ops.MS_PARTE: 2 * lay.enc_part - 4, ops.MS_PARTD: 2 * lay.dec_part, ops.MS_LOSS: 16,
                        ops.MS_PARTF: 1 << 20})                         # two tiles, the encoder blocks' stride one block short
    assert aug(12, 12, B=32, strides=short) == ERR_ARG and pn(12, 12, B=32, strides=short) == ERR_ARG
    assert pn(12, 12, strides=_strides({ops.MS_PARTF: 0})) == ERR_ARG                      # shared front_partials
    assert pn(12, 12, strides=_strides({ops.MS_PARTF: 2 * 10 * 12 - 4})) == ERR_ARG        # ... or one short of a block
    assert aug(12, 12, draw=1, strides=_strides({ops.MS_MASK_P: 0})) == ERR_ARG            # a written mask_p shared by two
    assert pn(12, 12, draw=1, strides=_strides({ops.MS_MASK_P: 0})) == ERR_ARG

    def tail(K=10, dp=12, d=12, strides=None, blocks=1, partF=p):
        return l.vpc_reduce_step_adam_eddi_multi(p, p, p, blocks, lay.enc_part, lay.dec_part, strides or _strides(), p, p, 2, p,
                                                 lay.n_params, 16, d, p, p, p, p, p, 0.9, 0.999, 1e-8, 1, p, p, partF, p, K, dp,
                                                 None)

    assert tail(K=33) == ERR_SHAPE and tail(dp=8) == ERR_SHAPE and tail(dp=68) == ERR_SHAPE
    assert tail(partF=None) == ERR_ARG
    assert tail(blocks=2, strides=short) == ERR_ARG
    assert tail(strides=_strides({ops.MS_PARTF: 0})) == ERR_ARG and tail(strides=_strides({ops.MS_SNAP: 0})) == ERR_ARG
    assert tail(strides=_strides({ops.MS_PARAM: lay.n_params})) == ERR_ARG  # a row must hold the front-end too


def test_wrappers_refuse_a_nine_slot_stride_vector():
    t = torch.zeros(4)
    with pytest.raises(vpc.VpcError, match="member strides"):
        ops.step_small_multi_eddi_f32(t, t, t, t, t, t, t, 2, 2, 2, 0, 0, 0, 1.0, 0.0, t, t, t, [0] * ops.MS_COUNT, 16, 12, 12, L, 10,
                                      t, t, t)


# ------------------------------------------------------------------ validation of the two classes
CASES = [
    ("mask", lambda: [], vpc.VpcError),
    ("mask", lambda: [mask_reg(), mask_van()], TypeError),                                 # mixed classes
    ("mask", lambda: [mask_reg(12), mask_reg(14)], vpc.VpcError),                          # shapes
    ("mask", lambda: [mask_reg(), mask_reg(Ld=8)], vpc.VpcError),
    ("mask", lambda: [mask_reg(), mask_reg(rt="ml_reg")], vpc.VpcError),                   # reg_type
    ("mask", lambda: [vpc.Reg_VAE(12, 500, 10, L, TP, "e", "kl_reg")] * 2, TypeError),     # a plain member
    ("mask", lambda: [mask_reg(), eddi_reg()], TypeError),                                 # a foreign family
    ("mask", lambda: [mask_reg(65), mask_reg(65)], vpc.VpcError),                          # 2 d > 128: no instantiation
    ("eddi", lambda: [], vpc.VpcError),
    ("eddi", lambda: [eddi_reg(), eddi_van()], TypeError),
    ("eddi", lambda: [eddi_reg(12), eddi_reg(16)], vpc.VpcError),
    ("eddi", lambda: [eddi_reg(K=10), eddi_reg(K=20)], vpc.VpcError),                      # emb_dim
    ("eddi", lambda: [eddi_reg(), eddi_reg(Ld=8)], vpc.VpcError),
    ("eddi", lambda: [eddi_reg(), eddi_reg(rt="ml_reg")], vpc.VpcError),
    ("eddi", lambda: [vpc.vanilla_VAE(12, 500, 10, L, TP, "e")] * 2, TypeError),
    ("eddi", lambda: [eddi_reg(), mask_reg()], TypeError),
    ("eddi", lambda: [eddi_reg(68), eddi_reg(68)], vpc.VpcError),                          # obs_dim > 64: no instantiation
]


@pytest.mark.parametrize("family,models,exc", CASES)
def test_members_are_validated_before_any_device_call(family, models, exc):
    cls = vpc.MaskEnsembleTrainer if family == "mask" else vpc.EDDIEnsembleTrainer
    ms = models()
    with pytest.raises(exc) as info:
        cls(ms)
    assert "CPU tensor" not in str(info.value)
    assert all("_stack" not in m.__dict__ for m in ms)  # nothing was stacked


@pytest.mark.parametrize("cls,make", [(vpc.MaskEnsembleTrainer, mask_reg), (vpc.EDDIEnsembleTrainer, eddi_reg)])
def test_world_size_per_member_lengths_and_the_ml_term(cls, make):
    ms = [make(), make()]
    with pytest.raises(vpc.VpcError, match="single-process") as info:
        cls(ms, world_size=2)
    assert "CPU tensor" not in str(info.value)
    with pytest.raises(vpc.VpcError, match="3 values for 2 members"):
        cls(ms, lr=[1e-3] * 3)
    with pytest.raises(vpc.VpcError, match="1 values for 2 members"):
        cls(ms, seeds=[1])
    assert all("_stack" not in m.__dict__ for m in ms)
    # members that disagree on the ml_reg term are refused by the member table, before any launch (as under EnsembleTrainer)
    t = E.MemberTable([make(rt="ml_reg"), make(rt="ml_reg")])
    with pytest.raises(vpc.VpcError, match="ml_reg term"):
        t.update(epoch=3, alpha=[0.0, 0.5])
    assert t.update(epoch=3, alpha=[0.3, 0.5]) and t.need_ml


def test_valid_members_reach_the_device_check():
    """A valid member list passes validation and stacking; only then the CPU tensors are refused."""
    for cls, ms in ((vpc.MaskEnsembleTrainer, [mask_reg(14), mask_reg(14)]), (vpc.EDDIEnsembleTrainer, [eddi_van(14), eddi_van(14)])):
        with pytest.raises(vpc.VpcError, match="CPU tensor"):
            cls(ms)
    with pytest.raises((TypeError, vpc.VpcError)):  # the plain trainer's rule is what it was
        vpc.EnsembleTrainer([mask_reg(), mask_reg()])


def test_family_pitch_and_layout():
    assert E.MASK.pitch(14) == 16 and E.EDDI.pitch(14) == 16 and E.PLAIN.pitch(14) == 16 and E.MASK.pitch(12) == 12
    lay = E.EDDI.layout(eddi_reg(14, 20))
    assert lay is vpc._lib.pointnet_layout(14, 20, L) and lay.K == 20 and lay.n_front == 14 * 20 + 14 + 20 * 22 + 20
    assert E.MASK.layout(mask_reg(14)).mask_augm == 1


# ------------------------------------------------------------------ routing of train_sweep
def _loader(sizes, d=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, d, generator=g), torch.rand(n, d, generator=g) < 0.7) for n in sizes]


def test_train_sweep_routes_the_families(monkeypatch):
    made, trained = [], []

    def stub(name):
        class Stub:
            def __init__(self, models, lr=None, seeds=None):
                made.append((name, [type(m).__name__ for m in models], list(seeds), lr))
                self.G, self.steps = len(models), 0

            def step(self, x, mask, **kw):
                self.steps += 1

            def epoch_total(self):
                return [0.0] * self.G
        return Stub

    for name in ("EnsembleTrainer", "MaskEnsembleTrainer", "EDDIEnsembleTrainer"):
        monkeypatch.setattr(H, name, stub(name))
    monkeypatch.setattr(H, "train", lambda *a, **kw: trained.append((a[10], kw["seed"], type(kw["model"]).__name__)))
    cfgs = [dict(vae_type="reg_vae1_mask_augm", alpha=0.5, seed=1), dict(vae_type="vanilla_EDDI1", seed=2),
            dict(vae_type="reg_EDDI1", seed=3), dict(vae_type="reg_vae2_mask_augm", alpha=0.8, seed=4),
            dict(vae_type="vanilla_vae1_with_drop_mask_augm", seed=5), dict(vae_type="reg_vae1", seed=6),
            dict(vae_type="vanilla_EDDI2", seed=7), dict(vae_type="reg_vae2", seed=8)]
    torch.manual_seed(5)
    out = vpc.train_sweep((_loader([16, 16]), None), cfgs, 30, 12, 500, 10, 1, L, "synth", TP, "e", 20, 10, max_epochs=1,
                          device=torch.device("cpu"), reg_type="kl_reg", verbose=False, save=False)
    assert [type(m).__name__ for m in out] == ["Reg_VAE_mask", "vanilla_EDDI", "Reg_EDDI", "Reg_VAE_mask", "vanilla_VAE_mask",
                                               "Reg_VAE", "vanilla_EDDI", "Reg_VAE"]
    assert sorted(made) == sorted([("MaskEnsembleTrainer", ["Reg_VAE_mask"] * 2, [1, 4], 0.001),
                                   ("EDDIEnsembleTrainer", ["vanilla_EDDI"] * 2, [2, 7], 0.001),
                                   ("EnsembleTrainer", ["Reg_VAE"] * 2, [6, 8], 0.001)])
    assert trained == [("reg_EDDI1", 3, "Reg_EDDI"), ("vanilla_vae1_with_drop_mask_augm", 5, "vanilla_VAE_mask")]
    # the probe that decides the groups leaves torch's generator alone: the members start from what they start from without it
    torch.manual_seed(5)
    ref = [vpc.model_loader("train", 12, 500, 10, L, 30, "synth", TP, 1, 20, 10, "e", "kl_reg", c["vae_type"]) for c in cfgs]
    for a, b in zip(out, ref):
        for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka


def test_train_sweep_keeps_singles_and_unroutable_members_alone(monkeypatch):
    made, trained = [], []

    class Stub:
        def __init__(self, models, lr=None, seeds=None):
            made.append(len(models))

    for name in ("MaskEnsembleTrainer", "EDDIEnsembleTrainer"):
        monkeypatch.setattr(H, name, Stub)
    monkeypatch.setattr(H, "train", lambda *a, **kw: trained.append(a[10]))
    run = lambda cfgs, d, sizes: vpc.train_sweep((_loader(sizes, d), None), cfgs, 30, d, 500, 10, 1, L, "synth", TP, "e", 20, 10,
                                                 max_epochs=1, device=torch.device("cpu"), reg_type="kl_reg", verbose=False,
                                                 save=False)
    # point-net members of a width that is no multiple of 4: no device draws in the ensemble launch
    run([dict(vae_type="vanilla_EDDI1"), dict(vae_type="vanilla_EDDI2")], 14, [16])
    # groups of one; members that differ in the ml_reg term or the class
    run([dict(vae_type="reg_vae1_mask_augm"), dict(vae_type="vanilla_vae1_mask_augm"), dict(vae_type="reg_EDDI1")], 12, [16])
    # a first batch beyond the small-batch step
    run([dict(vae_type="reg_vae1_mask_augm"), dict(vae_type="reg_vae2_mask_augm")], 12, [ops.step_small_max_rows() + 1])
    assert made == [] and len(trained) == 7
