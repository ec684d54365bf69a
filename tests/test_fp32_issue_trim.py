"""fp32 step, lane bases and balanced dW2 ownership (csrc/vpc_layout.h frag_* / fragT_*, csrc/vpc_device.h frag_bases /
fragT_bases, dec8_kernel, enc_bwd_kernel).

CPU: a stand-alone host program checks the address split exhaustively.  GPU: the 8-wave kernels against the oracle on the
shapes where the new code can go wrong (ragged last tile, out-of-range columns, a second tile per workgroup), against the
4-wave kernels, which keep the earlier addressing and ownership, and against themselves run to run.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae-posterior-consistency_amd", "csrc")
L = 10
DEV = "cuda"

SPLIT_CHECK = r"""
#include <cstdio>
#include <set>
#include <vector>
#include "vpc_layout.h"
using namespace vpc;
int main() {
    int bad = 0;
    long checked = 0;
    for (int S : {16, 64, 128}) {
        const int mask = (S / 4 - 1) & 15;
        std::set<std::vector<int>> fwd, tr[4];
        // forward / staging fragment: lane (m, q) reads 16 bytes of row 16 mt + m at slot (4 kt + q) ^ (m & mask)
        for (int mt = 0; mt < 8; ++mt)
            for (int kt = 0; kt < 8 && kt < S / 16; ++kt) {
                std::vector<int> lanes;
                const int imm = frag_imm(S, mt, kt);
                if (imm < 0 || imm >= 65536) { std::printf("fwd imm S=%d mt=%d kt=%d: %d\n", S, mt, kt, imm); ++bad; }
                for (int m = 0; m < 16; ++m)
                    for (int q = 0; q < 4; ++q) {
                        const int orig = 4 * ((16 * mt + m) * S + 4 * ((4 * kt + q) ^ (m & mask)));  // tile_fwd*, stage_frag
                        const int got = frag_base(S, frag_var(S, kt), m, q) + imm;
                        if (frag_addr(S, mt, kt, m, q) != orig || got != orig) {
                            if (bad < 20) std::printf("fwd S=%d mt=%d kt=%d m=%d q=%d: %d != %d\n", S, mt, kt, m, q, got, orig);
                            ++bad;
                        }
                        lanes.push_back(orig - imm);
                        ++checked;
                    }
                fwd.insert(lanes);
            }
        if ((int)fwd.size() != frag_nvar(S)) { std::printf("fwd S=%d: %zu bases, %d held\n", S, fwd.size(), frag_nvar(S)); ++bad; }
        // transposed fragment: register j of lane (m, q) reads row 16 kt + 4 q + j, column 16 mt + m
        for (int mt = 0; mt < 8 && mt < S / 16; ++mt)
            for (int kt = 0; kt < 8; ++kt) {
                const int imm = fragT_imm(S, mt, kt);
                if (imm < 0 || imm >= 65536) { std::printf("T imm S=%d mt=%d kt=%d: %d\n", S, mt, kt, imm); ++bad; }
                for (int j = 0; j < 4; ++j) {
                    std::vector<int> lanes;
                    for (int m = 0; m < 16; ++m)
                        for (int q = 0; q < 4; ++q) {
                            const int col = 16 * mt + m, cs = col >> 2, cl = col & 3, r = 4 * q + j;
                            const int orig = 4 * ((16 * kt + r) * S + (((cs ^ (r & mask)) << 2) | cl));  // tile_T*
                            const int got = fragT_base_j(S, j, m, q) + fragT_base_v(S, fragT_var(S, mt), q) + imm;
                            if (fragT_addr(S, mt, kt, j, m, q) != orig || got != orig) {
                                if (bad < 20) std::printf("T S=%d mt=%d kt=%d j=%d m=%d q=%d: %d != %d\n", S, mt, kt, j, m, q, got, orig);
                                ++bad;
                            }
                            lanes.push_back(orig - imm);
                            ++checked;
                        }
                    tr[j].insert(lanes);
                }
            }
        // per register j: one base per held second part
        for (int j = 0; j < 4; ++j)
            if ((int)tr[j].size() != fragT_nvar(S)) { std::printf("T S=%d j=%d: %zu bases, %d held\n", S, j, tr[j].size(), fragT_nvar(S)); ++bad; }
    }
    std::printf("checked %ld addresses, %d bad\n", checked, bad);
    return bad ? 1 : 0;
}
"""


def _host_cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return c
    raise RuntimeError("no host C++ compiler")


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_address_split_host_program(tmp_path, san):
    """base + immediate == the swizzled address of the readers, every immediate fits the 16-bit offset field, and the number
    of distinct bases is the number the kernels hold - for S in {16, 64, 128}, every lane, kt < 8, mt < 8, j < 4."""
    src = tmp_path / "split_check.cpp"
    src.write_text(SPLIT_CHECK)
    exe = tmp_path / ("split_check_san" if san else "split_check")
    flags = ["-std=c++17", "-O1", "-Wall", "-I", CSRC]
    if san:
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([_host_cxx()] + flags + [str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checked 33280 addresses, 0 bad" in r.stdout


# ------------------------------------------------------------------------------------------------------------ GPU
def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def _synth(B, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, d, generator=g)
    mask = torch.rand(B, d, generator=g) < 0.7
    mask_p = mask & (torch.rand(B, d, generator=g) < 0.7)
    return x, mask, mask_p, torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)


def _model(vpc, d, params):
    m = vpc.Reg_VAE(d, 500, 10, L, {"batch_size": 64, "patience": 100}, "exp", "kl_reg")
    sd = m.state_dict()
    for k, v in params.items():
        sd[k] = v.clone()
    m.load_state_dict(sd)
    return m.to(DEV)


def _fused_step(vpc, d, params, data, **kw):
    m = _model(vpc, d, params)
    tr = vpc.FusedTrainer(m)
    tr.step(*[t.to(DEV) for t in data], update=False, **kw)
    return m, tr


def _slices(m, O):
    """{parameter key: slice of the flat gradient}"""
    out, off = {}, 0
    for k, p in zip(O.PARAM_KEYS, m.trainable()):
        out[k] = (slice(off, off + p.numel()), tuple(p.shape))
        off += p.numel()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("d,B", [(128, 1), (128, 129), (72, 130), (128, 32768 + 129)])
def test_fused_step_8wave_vs_oracle(d, B, monkeypatch):
    """Throughput shape forced (128-row tiles, 8 waves): the tolerances of test_fused_step_ragged_shapes_vs_oracle.  (128, 1)
    and (128, 129): ragged last tile, wave 7 holds real rows in the first tile only; (72, 130): DT = 8 with out-of-range
    columns; (128, 32 897): 258 tiles on 256 workgroups - the bases and the accumulators live through a tile loop."""
    import vpc_amd as vpc
    from oracle import vae_oracle as O
    monkeypatch.setenv("VPC_TILE", "128")
    params = O.init_params(d, L, seed=7)
    data = _synth(B, d, seed=B + d)
    loss_ref, grads_ref, _ = O.torch_reg_step(params, L, *data, alpha=0.8, beta=0.9)
    m, tr = _fused_step(vpc, d, params, data, alpha=0.8, beta=0.9)
    print("loss", tr.loss_value(), loss_ref.item())
    flat = tr.grad.cpu().numpy()
    errs = {k: rel(flat[s].reshape(shp), grads_ref[k].numpy()) for k, (s, shp) in _slices(m, O).items()}
    print(errs)
    assert abs(tr.loss_value() - loss_ref.item()) <= 2e-5 * abs(loss_ref.item())
    for k, e in errs.items():
        assert e < 2e-4, k


@pytest.mark.gpu
@pytest.mark.parametrize("B", [129, 300])
def test_decoder_8wave_vs_4wave_dW5(B, monkeypatch):
    """The 4-wave dec_kernel (VPC_DEC8=0) keeps the addressing at the read: dW5 / db5 of the 8-wave kernel against it, with
    the tolerance of test_decoder_kernel_variants_agree."""
    import vpc_amd as vpc
    from oracle import vae_oracle as O
    d = 128
    monkeypatch.setenv("VPC_TILE", "128")
    params = O.init_params(d, L, seed=11)
    data = _synth(B, d, seed=B * 3 + d)
    res = []
    for v in ("1", "0"):
        monkeypatch.setenv("VPC_DEC8", v)
        m, tr = _fused_step(vpc, d, params, data, alpha=0.6, beta=0.9)
        res.append((tr.loss_value(), tr.grad.cpu().numpy().copy()))
    sl = _slices(m, O)
    assert abs(res[0][0] - res[1][0]) <= 2e-6 * abs(res[1][0])
    for k in (O.PARAM_KEYS[8], O.PARAM_KEYS[9]):  # decoder layer 5: weight, bias
        e = rel(res[0][1][sl[k][0]], res[1][1][sl[k][0]])
        print(k, e)
        assert e < 2e-5, k
    assert rel(res[0][1], res[1][1]) < 2e-5


@pytest.mark.gpu
def test_encoder_8wave_vs_4wave_dW2(monkeypatch):
    """The small-batch shape (VPC_TILE=64: 4 waves, every wave owns two in tiles of dW2) keeps its ownership: dW2 / db2 of
    the 8-wave shape, where wave 7 computes three of the 28 tile products, against it - the tolerance of
    test_workgroup_shapes_agree."""
    import vpc_amd as vpc
    from oracle import vae_oracle as O
    d, B = 128, 200
    params = O.init_params(d, L, seed=3)
    data = _synth(B, d, seed=B)
    res = {}
    for tile in ("128", "64"):
        monkeypatch.setenv("VPC_TILE", tile)
        m, tr = _fused_step(vpc, d, params, data, alpha=0.8, beta=0.9)
        res[tile] = (tr.loss_value(), tr.grad.cpu().numpy().copy())
    sl = _slices(m, O)
    assert abs(res["64"][0] - res["128"][0]) <= 2e-6 * abs(res["128"][0])
    for k in (O.PARAM_KEYS[2], O.PARAM_KEYS[3]):  # encoder layer 2: weight, bias
        e = rel(res["128"][1][sl[k][0]], res["64"][1][sl[k][0]])
        print(k, e)
        assert e < 2e-5, k
    assert rel(res["128"][1], res["64"][1]) < 2e-5


@pytest.mark.gpu
def test_8wave_step_is_bit_reproducible(monkeypatch):
    import vpc_amd as vpc
    from oracle import vae_oracle as O
    d, B = 128, 300
    monkeypatch.setenv("VPC_TILE", "128")
    params = O.init_params(d, L, seed=5)
    data = _synth(B, d, seed=B)
    _, a = _fused_step(vpc, d, params, data, alpha=0.8, beta=0.9)
    _, b = _fused_step(vpc, d, params, data, alpha=0.8, beta=0.9)
    assert a.loss_value() == b.loss_value() and torch.equal(a.grad, b.grad)
