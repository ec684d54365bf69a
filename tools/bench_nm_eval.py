"""eval_vae_mnar with engine="stream" (csrc/vpc_nm_impute.hip) against engine="chain" (the launch chain of forward_loss with
llh_eval, max_decoder_rows at its default), in one process:

  * REG_notMIWAE_v2 and notMIWAE_myversion at the reference's own shape (d = 12, L = 10, valid_k = 10 000; N = 1 600 rows and
    N = 64) and at the bench width (d = 128, L = 10, valid_k = 10 000, N = 256),
  * five rounds; a round times one block of each engine in turn (alternating), a block is harness.eval_vae_mnar with M = `reps`
    repetitions between two device synchronisations (the mask_p draw of the chain, the RMSE and the final copy to the host
    included), after a warm-up of the engine; one JSON line per (kind, shape, engine): the block times in ms per repetition,
    their median, min and max, then a summary line with the worst stream block against the best chain block and the
    GEMM-equivalent rate of the stream engine (50.4 k MAC per decoder row at d = 128),
  * the s_chunk sweep behind notmiwae.impute_chunk: notmiwae.impute_stream alone at each chunk length, the same alternation,
    one line per (kind, shape, s_chunk) and one with the default rule's choice.

    python tools/bench_nm_eval.py [--out profiles/nm_eval.jsonl] [--shapes 12:1600,12:64,128:256] [--kinds reg,van] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vpc_amd  # noqa: E402
from vpc_amd import notmiwae  # noqa: E402

TP = {"batch_size": 128, "patience": 1}
LAT, VALID_K = 10, 10000
REPS = {(12, 1600): 4, (12, 64): 40, (128, 256): 10}  # a block of either engine is a few tenths of a second
SWEEP = {(12, 1600): (512, 1008, 2000, 2512, 3344, 5008, 10000), (12, 64): (256, 512, 1008, 1264, 2000, 2512, 3344, 5008, 10000),
         (128, 256): (1008, 2512, 3344, 5008, 10000)}


def make(kind, d, N):
    g = torch.Generator().manual_seed(3)
    x, m = torch.rand(N, d, generator=g), (torch.rand(N, d, generator=g) < 0.5).float()
    torch.manual_seed(0)
    model = (vpc_amd.REG_notMIWAE_v2 if kind == "reg" else vpc_amd.notMIWAE_myversion)(d, 500, 10, LAT, TP, VALID_K, 1).cuda()
    return model, x.cuda(), m.cuda()


def eval_block(model, kind, x, m, engine, reps):
    vae_type = "reg_notMIWAE1" if kind == "reg" else "vanilla_notMIWAE1"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = vpc_amd.eval_vae_mnar(x, m, 50, x.shape[1], 500, 10, reps, LAT, "wine", TP, "exp", vae_type, 10, VALID_K, 1, model=model,
                              save=False, engine=engine, seed=7 if engine == "stream" else None)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, float(r)


def stream_block(model, x, m, s_chunk, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        notmiwae.impute_stream(model, x, m, num_samples=VALID_K, seed=7, offset=i * x.shape[0], s_chunk=s_chunk)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def stats(t):
    return dict(ms_blocks=[round(v, 3) for v in t], ms_median=round(statistics.median(t), 3), ms_min=round(min(t), 3),
                ms_max=round(max(t), 3))


def bench(kind, d, N, rounds, emit):
    model, x, m = make(kind, d, N)
    reps = REPS.get((d, N), 4)
    n_cu = vpc_amd._lib.max_blocks() // 2
    times, rmse = {"chain": [], "stream": []}, {}
    for engine in times:  # code objects, workspaces, first launches
        eval_block(model, kind, x, m, engine, 1)
    for _ in range(rounds):
        for engine in times:
            eval_block(model, kind, x, m, engine, 1)
            t, rmse[engine] = eval_block(model, kind, x, m, engine, reps)
            times[engine].append(t)
    base = dict(kind=kind, N=N, d=d, L=LAT, valid_k=VALID_K, decoder_rows=N * VALID_K, reps_per_block=reps)
    for engine, t in times.items():
        emit(dict(name=f"eval_vae_mnar_{engine}_{kind}_d{d}_n{N}", engine=engine, **base, **stats(t), rmse=rmse[engine]))
    mac = LAT * 128 + 128 * 128 + 128 * 2 * d  # decoder MACs per sample (the encoder runs once per workgroup)
    med = statistics.median(times["stream"])
    emit(dict(name=f"summary_{kind}_d{d}_n{N}", **base, s_chunk_default=notmiwae.impute_chunk(N, VALID_K, n_cu), n_cu=n_cu,
              stream_worst_ms=round(max(times["stream"]), 3), chain_best_ms=round(min(times["chain"]), 3),
              stream_worst_beats_chain_best=max(times["stream"]) < min(times["chain"]),
              chain_median_over_stream_median=round(statistics.median(times["chain"]) / med, 2),
              mac_per_sample=mac, stream_gemm_tflops=round(2.0 * mac * N * VALID_K / (med * 1e-3) / 1e12, 2)))
    sweep = {c: [] for c in SWEEP.get((d, N), (1008, 10000))}
    for c in sweep:
        stream_block(model, x, m, c, 1)
    for _ in range(rounds):
        for c in sweep:
            sweep[c].append(stream_block(model, x, m, c, reps))
    for c, t in sweep.items():
        emit(dict(name=f"impute_stream_{kind}_d{d}_n{N}_c{c}", **base, s_chunk=c, chunks_per_row=-(-VALID_K // c),
                  workgroups=N * -(-VALID_K // c), **stats(t)))
    best = min(sweep, key=lambda c: statistics.median(sweep[c]))
    emit(dict(name=f"sweep_{kind}_d{d}_n{N}", **base, best_s_chunk=best, best_ms_median=round(statistics.median(sweep[best]), 3),
              s_chunk_default=notmiwae.impute_chunk(N, VALID_K, n_cu)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="12:1600,12:64,128:256", help="d:N pairs")
    ap.add_argument("--kinds", default="reg,van")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nm_eval.py measures on the GPU: no device found")
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    for kind in a.kinds.split(","):
        for d, N in (tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")):
            bench(kind, d, N, a.rounds, emit)


if __name__ == "__main__":
    main()
