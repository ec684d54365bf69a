"""Row-tiled fp32 step: mask_p and eps drawn by the kernels that read them (csrc/vpc_rng.h mask_lane_* / eps_lane_counter,
enc_fwd_draw_kernel, dec8_draw_kernel, FusedTrainer._draw_fused).

CPU: a stand-alone host program checks the lane-to-counter mapping exhaustively against the index arithmetic of
draw_mask_body / eps_counter.  GPU: the same trainer from one seed with VPC_DRAW_FUSED=1 (draws inside encoder_fwd /
decoder_fused) and VPC_DRAW_FUSED=0 (the separate vpc_draw_step launch) must agree bit for bit in everything a step leaves
behind, on the smallest shapes at which the kernels can go wrong; steps that are not eligible keep the separate launch.
"""
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae-posterior-consistency_amd", "csrc")
L = 10
DEV = "cuda"
TP = {"batch_size": 64, "patience": 100}

LANE_CHECK = r"""
#include <cstdio>
#include <initializer_list>
#include "vpc_rng.h"
using namespace vpc;
int main() {
    long bad = 0, checked = 0;
    const long B = 300;  // local rows of the shard (three 128-row workgroup tiles, the last one ragged)
    for (int dk : {72, 96, 128})
        for (long row_lo : {0L, 300L}) {
            const long elem_lo = row_lo * dk, rows_global = 600;
            const EpsShard sh{B, rows_global, row_lo, 16};
            for (int wg = 0; wg < 3; ++wg)
                for (int w = 0; w < 8; ++w)
                    for (int c = 0; c < 16; ++c)
                        for (int q = 0; q < 4; ++q) {
                            const long row = 128L * wg + 16 * w + c;  // local row of lane (q, c) of wave w
                            // ---- mask_p: draw_mask_body gives local element i the global group (elem_lo + i) / 8, half (elem_lo + i) % 8
                            for (int t = 0; t < 8; ++t) {
                                if (16 * t + 4 * q + 3 >= dk) continue;  // column group out of range: never drawn, never stored
                                const long G = mask_lane_group(elem_lo, row, dk, t, q);
                                for (int k = 0; k < 4; ++k) {
                                    const long e = elem_lo + row * dk + 16 * t + 4 * q + k;
                                    if (G != e / 8 || mask_lane_half0(q) + k != e % 8) {
                                        if (bad < 20) std::printf("mask dk=%d lo=%ld row=%ld t=%d q=%d k=%d: group %ld half %d, want %ld %ld\n",
                                                                  dk, row_lo, row, t, q, k, G, mask_lane_half0(q) + k, e / 8, e % 8);
                                        ++bad;
                                    }
                                    ++checked;
                                }
                                // the call of this group is made by this lane or by lane q ^ 1 (same row), once per tile pair
                                const int u = t >> 1, maker = (mask_lane_call_tile(u, q) == t) ? q : (q ^ 1);
                                // (the partner holds the other four halves: the two words it hands over are the ones it does not use)
                                if (mask_lane_call_tile(u, maker) != t || mask_lane_group(elem_lo, row, dk, t, maker) != G ||
                                    (maker >> 1) != (q >> 1) || (maker != q && mask_lane_half0(maker) == mask_lane_half0(q))) {
                                    if (bad < 20) std::printf("share dk=%d row=%ld t=%d q=%d maker=%d\n", dk, row, t, q, maker);
                                    ++bad;
                                }
                                // the kernel walks the pairs with a stride of 4 groups from the group of pair 0
                                if (mask_lane_group(elem_lo, row, dk, mask_lane_call_tile(u, q), q) !=
                                    mask_lane_group(elem_lo, row, dk, mask_lane_call_tile(0, q), q) + 4 * u) {
                                    if (bad < 20) std::printf("stride dk=%d row=%ld t=%d q=%d\n", dk, row, t, q);
                                    ++bad;
                                }
                                ++checked;
                            }
                            // ---- eps: eps_counter of the group's index in the local [planes][B][16] array
                            if (row < B)
                                for (int plane = 0; plane < 2; ++plane) {
                                    const long g = (plane * B + row) * 4 + q;
                                    if (eps_lane_counter(sh, plane, row, q) != eps_counter(sh, g)) {
                                        if (bad < 20) std::printf("eps lo=%ld row=%ld q=%d plane=%d\n", row_lo, row, q, plane);
                                        ++bad;
                                    }
                                    ++checked;
                                }
                        }
        }
    std::printf("checked %ld counters, %ld bad\n", checked, bad);
    return bad ? 1 : 0;
}
"""
# per (dk, row_lo): 3 x 8 x 16 rows x [dk / 4 column groups x (4 halves + 1 sharing check)]; eps: 300 rows x 4 x 2 planes
N_CHECKED = sum(2 * (384 * (dk // 4) * 5 + 300 * 4 * 2) for dk in (72, 96, 128))


def _host_cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return c
    raise RuntimeError("no host C++ compiler")


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_lane_counters_host_program(tmp_path, san):
    """Group and halves of every mask byte a lane holds, the lane that makes the group's Philox call, and the eps counter of
    every (row, q, plane): dk in {72, 96, 128}, row_lo in {0, 300}, three workgroups, tiles 0..7."""
    src = tmp_path / "lane_check.cpp"
    src.write_text(LANE_CHECK)
    exe = tmp_path / ("lane_check_san" if san else "lane_check")
    flags = ["-std=c++17", "-O1", "-Wall", "-I", CSRC]
    if san:
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([_host_cxx()] + flags + [str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"checked {N_CHECKED} counters, 0 bad" in r.stdout


# ------------------------------------------------------------------------------------------------------------ GPU
def _data(B, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, d, generator=g).to(DEV), (torch.rand(B, d, generator=g) < 0.7).to(DEV)


def _trainer(vpc, d, rt="kl_reg", seed=5):
    torch.manual_seed(0)
    m = vpc.Reg_VAE(d, 500, 10, L, TP, "exp", rt) if rt else vpc.vanilla_VAE(d, 500, 10, L, TP, "exp")
    return vpc.FusedTrainer(m.to(DEV), seed=seed)


class _Recorder:
    """Stands in for the loaded library: records every vpc_* symbol fetched, hands out the real one."""

    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        if name.startswith("vpc_"):
            self.names.append(name)
        return getattr(self.real, name)


def _record(monkeypatch, fn):
    from vpc_amd import _lib
    rec = _Recorder(_lib.lib())
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "_lib", rec)
        fn()
    return rec.names


def _state(tr, planes):
    return {"mask_p": tr.mask_p_buf.clone(), "eps": tr.eps_buf[:planes].clone(), "out9": tr.out9.clone(),
            "grad": tr.grad.clone(), "flat": tr.model._flat.clone(), "exp_avg": tr.exp_avg.clone(),
            "exp_avg_sq": tr.exp_avg_sq.clone(), "rng_offset": tr.rng_offset}


def _same(a, b, skip=()):
    for k in a:
        if k in skip:
            continue
        u, v = a[k], b[k]
        ok = (u == v) if k == "rng_offset" else torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u,
                                                            v.view(torch.int32) if v.dtype == torch.float32 else v)
        assert ok, k


def _two_steps(vpc, monkeypatch, fused, d, B, rt="kl_reg", graph=False, expect=None, **kw):
    """Two consecutive steps of a fresh trainer (seed 5) with the switch forcing the in-kernel draws (fused) or the
    separate launch; returns the state after each step.  The throughput shape is forced in both (VPC_TILE=128), so the
    partial blocks - and with them the gradient's summation order - are those of the row-tiled kernels either way."""
    monkeypatch.setenv("VPC_TILE", "128")
    monkeypatch.setenv("VPC_DRAW_FUSED", "1" if fused else "0")
    tr = _trainer(vpc, d, rt)
    x, mask = _data(B, d, seed=B + d)
    planes = 1 if rt is None else 2
    out = []
    for i in range(2):
        step = (lambda: tr.step_graph(x, mask, **kw)) if graph else (lambda: tr.step(x, mask, **kw))
        names = _record(monkeypatch, step)
        if expect is not None and not graph:
            assert (("vpc_draw_step" if rt else "vpc_fill_normal") in names) == (not expect), names
            assert ("vpc_decoder_fused_draw_f32" in names) == expect, names
            assert ("vpc_encoder_fwd_draw_f32" in names) == (expect and rt is not None), names
        out.append(_state(tr, planes))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("d,B,rt", [(128, 300, "kl_reg"), (128, 257, "kl_reg"), (72, 300, "kl_reg"), (128, 300, None)],
                         ids=["d128_b300", "d128_b257", "d72_b300", "vanilla_d128_b300"])
def test_inkernel_draws_equal_draw_step(d, B, rt, monkeypatch):
    """(128, 300): two full tiles and a 44-row remainder; (128, 257): a one-row tile; d = 72: column tiles that can hold
    out-of-range columns; vanilla_VAE: one pass, no mask_p, one eps plane."""
    import vpc_amd as vpc
    new = _two_steps(vpc, monkeypatch, True, d, B, rt, expect=True, alpha=0.8, beta=0.9)
    old = _two_steps(vpc, monkeypatch, False, d, B, rt, expect=False, alpha=0.8, beta=0.9)
    skip = ("mask_p",) if rt is None else ()
    for a, b in zip(new, old):
        _same(a, b, skip=skip)


@pytest.mark.gpu
def test_inkernel_draws_sharded(monkeypatch):
    """Rows 300..599 of a global batch of 600: the draws are those of rows 300..599 of the unsharded in-kernel step and of
    the sharded step through vpc_draw_step."""
    import vpc_amd as vpc
    d, B, Bg = 128, 300, 600
    monkeypatch.setenv("VPC_TILE", "128")
    x, mask = _data(Bg, d, seed=3)
    res = {}
    for name, fused, sl, kw in (("whole", True, slice(0, Bg), {}),
                                ("shard", True, slice(B, Bg), dict(global_batch=Bg, row_lo=B)),
                                ("shard_old", False, slice(B, Bg), dict(global_batch=Bg, row_lo=B))):
        monkeypatch.setenv("VPC_DRAW_FUSED", "1" if fused else "0")
        tr = _trainer(vpc, d)
        st = []
        for i in range(2):
            names = _record(monkeypatch, lambda: tr.step(x[sl], mask[sl], alpha=0.8, beta=0.9, update=False, **kw))
            assert ("vpc_encoder_fwd_draw_f32" in names) == fused and ("vpc_decoder_fused_draw_f32" in names) == fused, names
            st.append(_state(tr, 2))
        res[name] = st
    for i in range(2):
        _same(res["shard"][i], res["shard_old"][i])
        assert torch.equal(res["shard"][i]["mask_p"], res["whole"][i]["mask_p"][B:Bg])
        assert torch.equal(res["shard"][i]["eps"].view(torch.int32), res["whole"][i]["eps"][:, B:Bg].view(torch.int32))
        assert res["shard"][i]["rng_offset"] == res["whole"][i]["rng_offset"]


@pytest.mark.gpu
def test_inkernel_draws_graph_replay(monkeypatch):
    """step_graph (one eager step that captures, then a replay: the Philox offset lives on the device) against two eager
    steps, both with the in-kernel draws."""
    import vpc_amd as vpc
    g = _two_steps(vpc, monkeypatch, True, 128, 300, graph=True, alpha=0.8, beta=0.9)
    e = _two_steps(vpc, monkeypatch, True, 128, 300, expect=True, alpha=0.8, beta=0.9)
    h = _two_steps(vpc, monkeypatch, False, 128, 300, graph=True, alpha=0.8, beta=0.9)
    for a, b, c in zip(g, e, h):
        _same(a, b)
        _same(a, c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["d100", "mask_p_injected", "eps_injected", "ml_reg", "bf16x3", "below_bound"])
def test_ineligible_steps_keep_draw_step(case, monkeypatch):
    """dk % 8 != 0, an injected draw, the ml_reg sample (a third eps plane), another precision: the separate draw launch
    stays even with the switch on, and the step gives what it gives with the switch off.  below_bound: without the switch
    a batch that does not give every CU a 128-row tile keeps it too."""
    import vpc_amd as vpc
    monkeypatch.setenv("VPC_TILE", "128")
    d = 100 if case == "d100" else 128
    B = 300
    x, mask = _data(B, d, seed=9)
    gen = torch.Generator().manual_seed(1)
    inj = {}
    if case == "mask_p_injected":
        inj = dict(mask_p=mask & (torch.rand(B, d, generator=gen) < 0.7).to(DEV))
    if case == "eps_injected":
        inj = dict(eps_q=torch.randn(B, L, generator=gen).to(DEV), eps_p=torch.randn(B, L, generator=gen).to(DEV))
    kw = dict(alpha=0.8, beta=0.9, epoch=1400 if case == "ml_reg" else 1)
    res = []
    for env in ((None,) if case == "below_bound" else ("1", "0")):
        if env is None:
            monkeypatch.delenv("VPC_DRAW_FUSED", raising=False)
        else:
            monkeypatch.setenv("VPC_DRAW_FUSED", env)
        torch.manual_seed(0)
        m = vpc.Reg_VAE(d, 500, 10, L, TP, "exp", "ml_reg" if case == "ml_reg" else "kl_reg").to(DEV)
        tr = vpc.FusedTrainer(m, seed=5, precision="bf16x3" if case == "bf16x3" else "f32")
        for i in range(2):
            names = _record(monkeypatch, lambda: tr.step(x, mask, **inj, **kw))
            assert "vpc_encoder_fwd_draw_f32" not in names and "vpc_decoder_fused_draw_f32" not in names, names
            if not inj:
                assert "vpc_draw_step" in names, names
        if case == "ml_reg":
            assert tr.coefficients(1400, 0.8, 0.9, False).ml_on
        res.append(_state(tr, 3 if case == "ml_reg" else 2))
    if len(res) == 2:
        if case == "eps_injected":  # injected eps fills the L columns it has: the pad columns of eps_buf are not written
            for r in res:
                r["eps"] = r["eps"][:, :, :L].contiguous()
        _same(res[0], res[1], skip=("mask_p",) if case == "mask_p_injected" else ())  # (injected: mask_p_buf is not written)
