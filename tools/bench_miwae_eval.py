"""eval_miwae with engine="stream" (csrc/vpc_miw_impute.hip) against engine="chain" (the launch chain of model.impute), in
one process:

  * Reg_MIWAE and MIWAE, d = 12, L = 10, valid_k = 5 000; one loader of ONE batch of N = 1 600 rows and one of ONE batch of 64,
  * five rounds; a round times one block of each engine in turn (alternating), a block is harness.eval_miwae with M = `reps`
    repetitions between two device synchronisations (the mask_p draw of the chain, the RMSE and the final copy to the host
    included), after a warm-up of the engine; one JSON line per (kind, N, engine): the block times in ms per repetition,
    their median, min and max, then a summary line with the worst stream block against the best chain block,
  * the s_chunk sweep that fixes miwae.impute_chunk: miwae.impute_stream alone at each chunk length, the same alternation,
    one line per (kind, N, s_chunk) and one with the default rule's choice.

    python tools/bench_miwae_eval.py [--out profiles/miwae_eval.jsonl] [--rows 1600,64] [--kinds reg,van] [--rounds 5]
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
from vpc_amd import miwae  # noqa: E402

TP = {"batch_size": 64, "patience": 1}
D, LAT, VALID_K = 12, 10, 5000
SWEEP = {1600: (256, 512, 1008, 1664, 2512, 5008), 64: (64, 128, 256, 512, 1008, 1264, 1664, 2512, 5008)}


def make(kind, N):
    g = torch.Generator().manual_seed(3)
    x, m = torch.rand(N, D, generator=g), torch.rand(N, D, generator=g) < 0.5
    torch.manual_seed(0)
    model = (vpc_amd.Reg_MIWAE if kind == "reg" else vpc_amd.MIWAE)(D, 500, 10, LAT, TP, VALID_K, 1).cuda()
    return model, x.cuda(), m.cuda()


def eval_block(model, kind, x, m, engine, reps):
    vae_type = "reg_MIWAE1" if kind == "reg" else "vanilla_MIWAE1"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = vpc_amd.eval_miwae([([(x, m)], "test")], 50, D, 500, 10, reps, LAT, "wine", TP, "exp", vae_type, 10, VALID_K, 1,
                           model=model, save=False, engine=engine, seed=7 if engine == "stream" else None)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, float(r["test"])


def stream_block(model, x, m, s_chunk, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        miwae.impute_stream(model, x, m, num_samples=VALID_K, seed=7, offset=i * x.shape[0], s_chunk=s_chunk)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def stats(t):
    return dict(ms_blocks=[round(v, 3) for v in t], ms_median=round(statistics.median(t), 3), ms_min=round(min(t), 3),
                ms_max=round(max(t), 3))


def bench(kind, N, rounds, emit):
    model, x, m = make(kind, N)
    reps = 20 if N >= 1000 else 200  # a block of either engine is a few tenths of a second
    n_cu = vpc_amd._lib.max_blocks() // 2
    times, rmse = {"chain": [], "stream": []}, {}
    for engine in times:  # code objects, workspaces, first launches
        eval_block(model, kind, x, m, engine, 1)
    for _ in range(rounds):
        for engine in times:
            eval_block(model, kind, x, m, engine, 1)
            t, rmse[engine] = eval_block(model, kind, x, m, engine, reps)
            times[engine].append(t)
    base = dict(kind=kind, N=N, d=D, L=LAT, valid_k=VALID_K, decoder_rows=N * VALID_K, reps_per_block=reps)
    for engine, t in times.items():
        emit(dict(name=f"eval_miwae_{engine}_{kind}_n{N}", engine=engine, **base, **stats(t), rmse=rmse[engine]))
    emit(dict(name=f"summary_{kind}_n{N}", **base, s_chunk_default=miwae.impute_chunk(N, VALID_K, n_cu), n_cu=n_cu,
              stream_worst_ms=round(max(times["stream"]), 3), chain_best_ms=round(min(times["chain"]), 3),
              stream_worst_beats_chain_best=max(times["stream"]) < min(times["chain"]),
              chain_median_over_stream_median=round(statistics.median(times["chain"]) / statistics.median(times["stream"]), 2)))
    sweep = {c: [] for c in SWEEP.get(N, (16, 5008))}
    for c in sweep:
        stream_block(model, x, m, c, 1)
    for _ in range(rounds):
        for c in sweep:
            sweep[c].append(stream_block(model, x, m, c, reps))
    for c, t in sweep.items():
        emit(dict(name=f"impute_stream_{kind}_n{N}_c{c}", **base, s_chunk=c, chunks_per_row=-(-VALID_K // c),
                  workgroups=N * -(-VALID_K // c), **stats(t)))
    best = min(sweep, key=lambda c: statistics.median(sweep[c]))
    emit(dict(name=f"sweep_{kind}_n{N}", **base, best_s_chunk=best, best_ms_median=round(statistics.median(sweep[best]), 3),
              s_chunk_default=miwae.impute_chunk(N, VALID_K, n_cu)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1600,64")
    ap.add_argument("--kinds", default="reg,van")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_miwae_eval.py measures on the GPU: no device found")
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    for kind in a.kinds.split(","):
        for N in (int(n) for n in a.rows.split(",")):
            bench(kind, N, a.rounds, emit)


if __name__ == "__main__":
    main()
