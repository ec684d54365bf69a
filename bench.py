"""bench.py - training samples/sec of the VAE posterior-consistency step (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--scaling weak|strong] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = the build's counterpart of src/experiment_main/train.py:53-117 for Reg_VAE(kl_reg, alpha=1,
beta=1): on-device mask_p draw + eps draw -> 2 x encoder + 2 x decoder forward -> ELBO + consistency loss ->
backward -> (one flat all-reduce) -> Adam, on synthetic batches x ~ U(0,1) [B=65 536, d=128], mask ~
Bern(0.7), already resident in HBM.  The timed loop ROTATES over 8 distinct resident batches (336 MB of x + mask,
more than the 256 MiB Infinity Cache), as an epoch streams different rows every step.
Scaling: "weak" (default) - every rank steps its own B rows (global batch N*B); "strong" (--scaling strong) - the
global batch stays B = 65 536 and every rank steps B/N rows of it (north_star's "partition minibatches").  Either
way the per-step gradient all-reduce (RCCL) is inside the timed region, ranks share ONE Philox seed and the draws
are keyed by the global row.
Warm-up: the W requested steps, then "settle" steps in groups of 8 until the dominant kernel's HIP-event time of two
consecutive groups agrees within 1.5 % (clock ramp after idle; at most 40 groups, all untimed; reported as
`settle_steps`), then EXACTLY K timed steps.  The settle steps only warm the clocks: the trainer state (parameters, Adam
moments, step count, Philox offset, batch rotation) is put back to where the W warm-up steps left it before the timed
steps, so that the timed steps compute the same thing whatever number of settle steps a run needed.

Prints ONE JSON line (rank 0) with the contract's fields plus
  roofline     - dominant kernel (vpc_decoder_fused: reparam + decoder fwd + loss + decoder bwd): algorithmic
                 FLOP per launch / HIP-event duration measured live on the launch stream, vs the f32 MFMA peak
--full adds what takes runs of its own:
  kernels_ms of the other launches (16 steps after the timed region), per_step_sync_ms (the step with the reference's
  per-step `.item()`), with N > 1 the other scaling mode, and with N = 1
  extra_configs - BASELINE configs 2, 3 and 5 and the headline shape in bf16 (--no-extra-configs skips them)
  cpu_baseline  - the oracle's op-for-op torch port of the reference CPU path (oracle/vae_oracle.py), timed on
                  the host cores on a bounded sample (--no-cpu-baseline skips it).
--dump-outputs DIR writes what the last timed step left for its caller (rank 0), as float32 .npy files: loss_terms (the
step's loss and its 8 terms), grad (the flat gradient), params (the flat parameters after the Adam update), exp_avg and
exp_avg_sq (the Adam moments).  Inputs, initial weights and draws are seeded: the same arguments give the same inputs.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense
BF16_MFMA_PEAK_TFLOPS = 2516.6  # same guide: bf16 MFMA = 16 x the fp32 MFMA rate (~2.5 PF dense)
# MFMA peak the algorithmic FLOPs are priced against: a bf16x3 product issues three bf16 MFMAs per fp32 product
PEAK = {"f32": F32_MFMA_PEAK_TFLOPS, "bf16x3": BF16_MFMA_PEAK_TFLOPS / 3.0, "bf16": BF16_MFMA_PEAK_TFLOPS}
HBM_PEAK_TBS = 8.0


def flops_per_sample(d, L, passes=2):
    """Algorithmic FLOP per sample: fwd F, bwd 2F - d*H1 (no dgrad to x)."""
    enc_f = d * 100 + 100 * 50 + 50 * 2 * L
    dec_f = L * 50 + 50 * 100 + 100 * d
    enc = enc_f + (2 * enc_f - d * 100)
    dec = 3 * dec_f
    return dict(total=2 * passes * (enc + dec), decoder_fused=2 * passes * dec, encoder_fwd=2 * passes * enc_f,
                encoder_bwd=2 * passes * (2 * enc_f - d * 100), step_fused=2 * passes * (enc + dec),
                step_small=2 * passes * (enc + dec))


def _traffic_table():
    """Committed rocprofv3 PMC passes (FETCH_SIZE x2 per the gfx950 correction + WRITE_SIZE, mean per dispatch): the newest
    round's file that exists.  PMC counters cannot be read from inside this process, so these are the numbers measured with
    `rocprofv3 --pmc` on this same command (tools/pmc_r03.sh)."""
    for name in ("r03_traffic.json", "r02_traffic.json"):
        try:
            return json.load(open(os.path.join(ROOT, "profiles", name)))
        except Exception:
            continue
    return None


def measured_traffic(B, d, L, precision="f32", dom="decoder_fused"):
    """HBM bytes per launch of the dominant kernel; None for shapes / precisions without a PMC pass."""
    t = _traffic_table()
    try:
        if t is None or (B, d, L) != (65536, 128, 10):
            return None
        ks = t["precisions"][precision]
        key = "step_bf16" if dom == "step_fused" else "dec8"
        return next(v["hbm_bytes_corrected"] for k, v in ks.items() if key in k)
    except Exception:
        return None


def measured_step_traffic(B, d, L, precision="f32", dom="decoder_fused"):
    """HBM bytes per STEP: every kernel of the step that has a PMC pass; launches without one are priced at their
    algorithmic traffic (reduce_step reads the partial blocks = 49 MB and writes < 1 MB; draw_step reads the mask and
    writes mask_p + eps = 22 MB).  None for shapes / precisions without a PMC pass."""
    t = _traffic_table()
    try:
        if t is None or (B, d, L) != (65536, 128, 10):
            return None
        ks = t["precisions"][precision]
        if dom == "step_fused" and not any("step_bf16" in k for k in ks):
            return None
        tot = sum(v["hbm_bytes_corrected"] for v in ks.values())
        if not any("reduce_step" in k for k in ks):
            tot += 49_000_000
        if not any("draw_step" in k for k in ks):
            tot += 22_000_000
        return tot
    except Exception:
        return None


def cpu_baseline(B, d, L, seconds=20.0, threads=None):
    """Reference CPU path (port), fp32: 2 warm-up steps + timed steps, median; then the same with autograd anomaly
    detection ON (the reference's drivers enable it, src/experiment_main/imputation.py:19) as a second row.
    `threads` defaults to the cores this job may use (the GPU box gives a 1-GPU job a 16-core share of a 128-core
    host; torch's default of 128 threads oversubscribes that share 8x and runs the step 6x slower: capped at 16)."""
    from oracle import vae_oracle as O
    if threads is None:
        threads = min(16, len(os.sched_getaffinity(0)))
    torch.set_num_threads(threads)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, d, generator=g)
    mask = torch.rand(B, d, generator=g) < 0.7

    def run(budget, anomaly):
        torch.manual_seed(0)
        tr = O.TorchTrainer(O.init_params(d, L, seed=0), L, reg_type="kl_reg")
        times = []
        t_end = time.perf_counter() + budget
        with torch.autograd.set_detect_anomaly(anomaly):
            for i in range(2 + 30):
                t0 = time.perf_counter()
                tr.step(x, mask, p_missingness=30, alpha=1.0, beta=1.0, epoch=1)
                dt = time.perf_counter() - t0
                if i >= 2:
                    times.append(dt)
                if i >= 4 and time.perf_counter() > t_end:
                    break
        return statistics.median(times), len(times)

    med, n = run(seconds * 0.6, False)
    med_on, n_on = run(seconds * 0.4, True)
    what = (f"steps (median) after 2 warm-up of the same B={B} d={d} Reg_VAE kl_reg step (numpy mask_p draw + forward + "
            f"loss + backward + Adam + .item())")
    return dict(value=B / med, unit="samples/s", cores=torch.get_num_threads(), kind="port",
                sample=f"{n} {what}, anomaly-detect off", ms_per_step=med * 1e3,
                anomaly_on=dict(value=B / med_on, unit="samples/s", ms_per_step=med_on * 1e3,
                                sample=f"{n_on} {what}, torch.autograd.set_detect_anomaly(True) as imputation.py:19"))


def mnar_flops_per_sample(d, L, K, H=128, passes=2):
    """Algorithmic FLOP per data row of the MNAR step (REG_notMIWAE_v2, src/models/VAE.py:2327-2505): encoder
    d->H->H->(L|L) once per pass, decoder L->H->H->(d|d) on K samples per row; backward 2x forward minus the dgrad to x."""
    enc = d * H + H * H + H * 2 * L
    dec = K * (L * H + H * H + H * 2 * d)
    return 2 * passes * (3 * (enc + dec) - d * H)


def self_launch(args):
    """`python bench.py --gpus N` (N > 1) without a launcher: start N rank processes as a `python -m torch.distributed.run`
    CHILD - this parent has not touched the GPU (torch.cuda.device_count() does not initialise it) - and exit with its code.
    Fails non-zero instead of measuring fewer GPUs than asked for."""
    import socket
    import subprocess
    rehearsal = os.environ.get("VPC_DIST_BACKEND") == "gloo"  # N ranks sharing the visible device(s) / the CPU
    ndev = torch.cuda.device_count()
    if ndev < args.gpus and not rehearsal:
        print(f"bench.py: --gpus {args.gpus} but {ndev} GPU(s) are visible; refusing to measure fewer GPUs than asked for "
              f"(VPC_DIST_BACKEND=gloo rehearses the multi-rank path on what is there)", file=sys.stderr)
        return 2
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this driver
    # the ranks' stdout is relayed line by line, JSON lines only: the contract is ONE JSON line on stdout, and some
    # process-group back ends (gloo) print their own chatter there
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in proc.stdout:
        if line.lstrip().startswith("{"):
            sys.stdout.write(line)
            sys.stdout.flush()
        else:
            sys.stderr.write(line)
    return proc.wait()


def ranks_seen(vpc, tr, world, dev):
    """Ranks the step's OWN collective carrier sums over (1 per rank through tr's carrier): what `n_gpus` reports."""
    if world == 1:
        return 1
    one = torch.ones(1, device=dev)
    vpc.dp.allreduce_bucket(one, None, tr._collective())
    torch.cuda.synchronize()
    return int(round(float(one.item())))


def dump_outputs(tr, model, out_dir):
    """What the last step left for its caller (module docstring), as float32 .npy files in out_dir."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss_terms": tr.out9, "grad": tr.grad, "params": model._flat, "exp_avg": tr.exp_avg,
              "exp_avg_sq": tr.exp_avg_sq}
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().float().cpu().numpy())


def measure(vpc, args, rank, world, dev, scaling, dump_dir=None):
    """Warm-up, settle, EXACTLY args.steps timed steps (barrier + synchronize on both sides, MAX over ranks) of the
    headline step in one scaling mode; returns the raw numbers (every rank) - rank 0 formats them.  dump_dir: where rank 0
    writes the last timed step's outputs."""
    d, Ld = args.dim, args.latent
    if scaling == "strong":
        Bg = args.batch
        lo, hi = vpc.dp.shard_rows(Bg, rank, world)
        B = hi - lo
    else:
        B, Bg, lo = args.batch, args.batch * world, rank * args.batch
    torch.manual_seed(0)
    model = vpc.Reg_VAE(d, 500, 10, Ld, {"batch_size": B, "patience": 100}, "bench", "kl_reg").to(dev)
    flat = model.flatten_parameters()
    vpc.dp.broadcast_parameters(flat, model=model)
    # this rank's rows of `--batches` distinct global batches, resident in HBM (8 x 42 MB > the 256 MiB Infinity Cache)
    g = torch.Generator().manual_seed(1234 + rank)
    xs = [torch.rand(B, d, generator=g).to(dev) for _ in range(args.batches)]
    masks = [(torch.rand(B, d, generator=g) < 0.7).to(dev) for _ in range(args.batches)]
    # one shared seed: Philox counters are keyed by the global row, so ranks draw disjoint parts of one stream
    tr = vpc.FusedTrainer(model, lr=1e-3, seed=0, world_size=world, rank=rank, precision=args.precision)
    kw = dict(alpha=1.0, beta=1.0, p_missingness=30, epoch=1, global_batch=Bg, row_lo=lo)
    it = [0]

    def step():
        i = it[0] % args.batches
        it[0] += 1
        tr.step(xs[i], masks[i], **kw)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()

    for _ in range(args.warmup):
        step()
    sync()
    # the state the timed steps start from, put back after the settle steps (module docstring)
    warm = (flat.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.step_count, tr.rng_offset, it[0])
    dom = tr.dominant_launch()  # "decoder_fused", or "step_fused" when the three MFMA kernels are one launch
    # CPython's generation-2 garbage collection fires once around step 70 of the timed loop (the ctypes argument arrays of
    # ~350 launches) and, with torch's millions of live objects, pauses the host for 20-40 ms - longer than the work
    # queued on the GPU at that point (rocprofv3 trace: one 38 ms gap, nothing else).  Collect here, BEFORE the settle
    # steps: a collection right in front of the timed region leaves the GPU idle for tens of ms and the first timed steps
    # then run on ramped-down clocks (a 20-step region read 0.369 instead of 0.340 ms / step).
    gc.collect()
    gc.disable()
    # settle: until the dominant kernel's event time is stable (all ranks run the same number of groups)
    settle = 0
    if not args.no_settle:
        tr.timers, tr.timer_names, tr.timer_every = {}, {dom}, 1
        prev = None
        for _ in range(40):
            tr.timers.clear()
            for _ in range(8):
                step()
            settle += 8
            torch.cuda.synchronize()
            cur = statistics.mean(a.elapsed_time(b) for a, b in tr.timers[dom])
            done = prev is not None and abs(cur - prev) <= 0.015 * prev
            if world > 1:
                flag = torch.tensor([1.0 if done else 0.0], device=dev)
                torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
                done = bool(flag.item() > 0.5)
            if done:
                break
            prev = cur
        tr.timers, tr.timer_every = None, 8
        for dst, src in zip((flat, tr.exp_avg, tr.exp_avg_sq), warm[:3]):
            dst.copy_(src)
        tr.step_count, tr.rng_offset, it[0] = warm[3:]
        # the weight images follow the flat parameters: re-packed from the restored ones by the next step
        model.invalidate_images()
        if tr.prec:
            tr._stale = {"pair": True, "step": True}
        sync()
    del warm
    tr.epoch_total()  # reset the device-side loss accumulator: loss_mean below covers the timed steps only
    # Inside the timed region only the dominant kernel is bracketed by HIP events (every 8th step; every K-th when K < 8, so
    # that a short region holds a sample too); with --full the other launches are sampled right after the region.
    tr.timers, tr.timer_names, tr.timer_every = {}, {dom}, max(1, min(8, args.steps))
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    sync()
    elapsed = time.perf_counter() - t0
    gc.enable()
    total = tr.epoch_total()  # one host read per "epoch", as train.py:118 (the timed steps only)
    if dump_dir is not None and rank == 0:
        dump_outputs(tr, model, dump_dir)
    timers, tr.timers = tr.timers, None
    per_step_sync_ms = None
    if args.full:
        tr.timers = {}
        tr.timer_names, tr.timer_every = {"encoder_fwd", "encoder_bwd", "draw_step", "reduce_step"}, 2
        for _ in range(16):
            step()
        sync()
        timers.update(tr.timers)
        tr.timers = None
        # the reference reads the loss on the host every step (train.py:117 `.item()`): the same steps with that sync
        n_sync = min(args.steps, 50)
        sync()
        t1 = time.perf_counter()
        for _ in range(n_sync):
            step()
            tr.loss_value()
        sync()
        per_step_sync_ms = (time.perf_counter() - t1) / n_sync * 1e3
    seen = ranks_seen(vpc, tr, world, dev)
    if world > 1:
        t = torch.tensor([elapsed, per_step_sync_ms or 0.0], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t[0].item())
        if args.full:
            per_step_sync_ms = float(t[1].item())
        torch.distributed.barrier()
    kern_ms = {k: statistics.mean(a.elapsed_time(b) for a, b in v) for k, v in timers.items()}
    return dict(B=B, Bg=Bg, elapsed=elapsed, per_step_sync_ms=per_step_sync_ms, total=total, settle=settle, kern_ms=kern_ms,
                dom=dom, small=tr.last_blocks[1] > (B + 127) // 128, seen=seen, value=Bg * args.steps / elapsed,
                ms_step=elapsed / args.steps * 1e3)


def timed_steps(fn, warm, n):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def extra_configs(vpc, dev):
    """BASELINE configs 2, 3 and 5 at the reference's own sizes, in this process, after the headline region (each variant
    gets >= 120 warm-up steps: the first launches of a kernel variant carry one-time costs, profiles/r02_notes.md).
    Synthetic stand-ins of the right shape ("UCI gas" = 13 910 x 128, MCAR 30 %): no datasets ship with the reference."""
    out = []
    TP = {"batch_size": 64, "patience": 100}
    N, d, Ld = 13910, 128, 10
    # the headline shape in the precision BASELINE configs 2 / 3 name (plain bf16 inputs, fp32 accumulation and loss math):
    # ONE whole-step kernel (csrc/vpc_step.hip) + draws + gradient reduction / Adam
    try:
        Bh = 65536
        gh = torch.Generator().manual_seed(7)
        xh = torch.rand(Bh, d, generator=gh).to(dev)
        mh = (torch.rand(Bh, d, generator=gh) < 0.7).to(dev)
        torch.manual_seed(0)
        model = vpc.Reg_VAE(d, 500, 10, Ld, {"batch_size": Bh, "patience": 100}, "bench", "kl_reg").to(dev)
        tr = vpc.FusedTrainer(model, precision="bf16")
        dt = timed_steps(lambda: tr.step(xh, mh, alpha=1.0, p_missingness=30), 60, 100)
        fh = flops_per_sample(d, Ld)["total"]
        tb = measured_step_traffic(Bh, d, Ld, "bf16", tr.dominant_launch())
        out.append(dict(config="headline shape, bf16", workload="Reg_VAE kl_reg step, B=65536 d=128, plain bf16 MFMA inputs (whole-step kernel)",
                        dtype="bf16", ms_per_step=dt * 1e3, samples_per_s=Bh / dt,
                        roofline=dict(bound="mfma", achieved=fh * Bh / dt / 1e12, peak=PEAK["bf16"], unit="TFLOP/s",
                                      frac=fh * Bh / dt / 1e12 / PEAK["bf16"], note="whole step incl. draws and Adam"),
                        step_hbm=None if tb is None else dict(bytes_per_step=tb, achieved_TBps=tb / dt / 1e12,
                                                              frac=tb / dt / 1e12 / HBM_PEAK_TBS)))
        del tr, model, xh, mh
    except Exception as e:
        out.append(dict(config="headline shape, bf16", error=repr(e)[:200]))
    g = torch.Generator().manual_seed(1)
    x = torch.rand(N, d, generator=g).to(dev)
    m = (torch.rand(N, d, generator=g) < 0.7).to(dev)
    fl = flops_per_sample(d, Ld)["total"]
    # config 2: Reg_VAE kl_reg, batch 64 (Data/imputation_args.json), fused step incl. draws and Adam
    for prec in ("f32", "bf16"):
        try:
            torch.manual_seed(0)
            model = vpc.Reg_VAE(d, 500, 10, Ld, TP, "bench", "kl_reg").to(dev)
            tr = vpc.FusedTrainer(model, precision=prec)
            bs = [(x[i:i + 64], m[i:i + 64]) for i in range(0, N - 63, 64)]
            k = [0]

            def st():
                xb, mb = bs[k[0] % len(bs)]
                k[0] += 1
                tr.step(xb, mb, alpha=1.0, p_missingness=30)
            dt = timed_steps(st, 160, 2 * len(bs))
            ar = "f32" if tr.dominant_launch() == "step_small" else prec  # small batches run the fp32 N-split kernel in every precision
            out.append(dict(config=2, workload="UCI gas stand-in 13910x128 MCAR, Reg_VAE kl_reg, batch 64, fused step",
                            dtype=prec, us_per_step=dt * 1e6, samples_per_s=64 / dt, kernel=tr.dominant_launch(), arithmetic=ar,
                            roofline=dict(bound="mfma", achieved=fl * 64 / dt / 1e12, peak=PEAK[ar], unit="TFLOP/s",
                                          frac=fl * 64 / dt / 1e12 / PEAK[ar],
                                          note="whole step incl. draws and Adam; latency-bound at this batch")))
            del tr, model
        except Exception as e:  # an extra line must never take the headline down
            out.append(dict(config=2, dtype=prec, error=repr(e)[:200]))
    # config 3: REG_notMIWAE_v2, batch 128, K = 20, p_missingness 50 (Data/imputation_args_mnar.json:1-2)
    for prec in ("f32", "bf16"):
        try:
            from vpc_amd import notmiwae as nm
            K = 20
            mf = m.float()
            torch.manual_seed(0)
            model = nm.REG_notMIWAE_v2(d, 128, 10, Ld, {"batch_size": 128, "patience": 1}, K, 1).to(dev)
            tr = nm.NMTrainer(model, precision=prec)
            bs = [(x[i:i + 128], mf[i:i + 128]) for i in range(0, N - 127, 128)]
            k = [0]

            def st3():
                xb, mb = bs[k[0] % len(bs)]
                k[0] += 1
                tr.step(xb, mb, alpha=0.5, p_missingness=50)
            dt = timed_steps(st3, 160, 2 * len(bs))
            f3 = mnar_flops_per_sample(d, Ld, K)
            out.append(dict(config=3, workload="UCI gas stand-in (MNAR), REG_notMIWAE_v2 K=20, batch 128, p_missingness 50",
                            dtype=prec, us_per_step=dt * 1e6, samples_per_s=128 / dt,
                            decoder="layer-fused kernel (csrc/vpc_nmdec.hip)" if tr.use_nmdec else "GEMM chain",
                            roofline=dict(bound="mfma", achieved=f3 * 128 / dt / 1e12, peak=PEAK[prec], unit="TFLOP/s",
                                          frac=f3 * 128 / dt / 1e12 / PEAK[prec], note="whole step")))
            del tr, model
        except Exception as e:
            out.append(dict(config=3, dtype=prec, error=repr(e)[:200]))
    # config 5: ONE acquisition step of active_learning_func (evaluate.py:394-440) on a Reg_VAE, n_test = 256, M = 50: the M
    # Monte-Carlo forwards as one batched pass + the reward of every (row, candidate) + argmax
    try:
        n, M = 256, 50
        torch.manual_seed(0)
        model = vpc.Reg_VAE(d, 500, 10, Ld, TP, "bench", "kl_reg").to(dev)
        xt, tm = x[:n], m[:n]
        cur = (torch.rand(n, d, generator=torch.Generator().manual_seed(5)) < 0.3).float().to(dev)
        cur[:, -1] = 0
        from vpc_amd import active as act
        with torch.no_grad():
            def st5():
                im = act.mc_forward(model, xt, cur, tm, M)
                R = act.reward_matrix(model, xt, cur, im)
                return R.argmax(1)
            dt = timed_steps(st5, 30, 50)
        enc_evals = 4 * (d - 1) * M * n  # encoder calls the reference makes for this step (evaluate.py:424-433, 514-634)
        # algorithmic FLOP of the formulation the kernel uses: per (row, candidate, sample) two encodings that
        # differ from the row's base encoding by a rank-1 update of layer 1 (100 FMA) + layers 2, 3; per (row, sample) two
        # candidate-independent full encodings
        f5 = 2 * n * M * ((d - 1) * 2 * (100 + 100 * 50 + 50 * 2 * Ld) + 2 * (d * 100 + 100 * 50 + 50 * 2 * Ld))
        out.append(dict(config=5, workload="one active_learning_func acquisition step, Reg_VAE d=128, n_test=256, M=50",
                        dtype="f32", ms_per_step=dt * 1e3, encoder_evaluations_replaced=enc_evals,
                        roofline=dict(bound="mfma", achieved=f5 / dt / 1e12, peak=PEAK["f32"], unit="TFLOP/s",
                                      frac=f5 / dt / 1e12 / PEAK["f32"],
                                      note="whole acquisition step (M batched forwards through the API path + reward kernels "
                                           "+ argmax) priced at the FLOP of the rank-1 formulation the kernel computes, not "
                                           "at the reference's 4 (d-1) M n full encoder calls")))
    except Exception as e:
        out.append(dict(config=5, error=repr(e)[:200]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=65536, help="rows per GPU (weak) / global rows (strong)")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--latent", type=int, default=10)
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="which reading `value` reports; with more than one GPU and --full both are measured and printed")
    ap.add_argument("--precision", choices=["f32", "bf16x3", "bf16"], default="f32",
                    help="f32 = the headline (exact fp32 MFMA); bf16x3 / bf16 = extra lines on v_mfma_f32_16x16x32_bf16")
    ap.add_argument("--batches", type=int, default=8, help="distinct resident batches the loop rotates over")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: the other launches' kernels_ms, per_step_sync_ms, the "
                         "other scaling mode (N > 1), extra_configs and cpu_baseline (N = 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs to DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="with --full: skip the configs 2 / 3 / 5 lines (extra_configs)")
    ap.add_argument("--no-settle", action="store_true", help="skip the settle steps after the W warm-up steps")
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--cpu-threads", type=int, default=None)
    ap.add_argument("--launch-check", action="store_true",
                    help="only bring the ranks up, count them through the collective and print {n_gpus}: launcher test")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))  # before anything in this process touches the GPU

    import vpc_amd as vpc
    rank, world, local = vpc.dp.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.launch_check:  # launcher / rendezvous / rank count only (runs without a GPU over gloo: tests/test_bench_launch.py)
        one = torch.ones(1)
        if world > 1:
            one = one.to(torch.device("cuda", local)) if torch.distributed.get_backend() == "nccl" else one
            torch.distributed.all_reduce(one)
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": int(one.item()), "world_size_env": world,
                              "backend": torch.distributed.get_backend() if world > 1 else None}))
        vpc.dp.shutdown()
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    d, Ld = args.dim, args.latent

    modes = [args.scaling] if world == 1 or not args.full else [args.scaling, "strong" if args.scaling == "weak" else "weak"]
    res = {mode: measure(vpc, args, rank, world, dev, mode, args.dump_outputs if mode == args.scaling else None)
           for mode in modes}
    if rank != 0:
        vpc.dp.shutdown()
        return
    r = res[args.scaling]
    if not (r["total"] == r["total"]):
        raise SystemExit("loss is NaN")
    if r["seen"] != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the step's collective summed over {r['seen']} rank(s)")

    B, Bg, ms_step, value, kern_ms, dom = r["B"], r["Bg"], r["ms_step"], r["value"], r["kern_ms"], r["dom"]
    fl = flops_per_sample(d, Ld)
    achieved = fl[dom] * B / (kern_ms[dom] * 1e-3) / 1e12
    rows = f"B={B} per GPU" if args.scaling == "weak" else f"global B={Bg} sharded {B} rows per GPU"
    kname = {"decoder_fused": ("vpc::dec_kernel<8,true,FUSED,1> (small-batch shape)" if r["small"] else "vpc::dec8_kernel<8,true>")
                              + " (vpc_decoder_fused)",
             "step_fused": "vpc::step_bf16_kernel<8> (vpc_step_fused_bf16: encoder fwd + decoder + loss + all backward)",
             "step_small": "vpc::step_small_kernel<8> (vpc_step_small_f32: the whole step, 16-row tiles split over the waves)"}[dom]
    out = {
        "metric": "training samples/sec (ELBO+consistency step), B=65536 d=128",
        "value": value, "unit": "samples/s", "n_gpus": r["seen"], "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_step, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": args.precision,
        "data": "synthetic",
        "config": {"workload": f"Reg_VAE kl_reg alpha=1 beta=1 training step, synthetic tabular {rows}, "
                               f"d={d}, L={Ld}, MCAR mask 0.7, p_missingness=30, Adam lr=1e-3, "
                               f"{args.batches} resident batches rotated",
                   "global_batch": Bg, "parallelism": f"dp{world}"},
        "roofline": {"bound": "mfma", "kernel": kname,
                     "achieved": achieved, "peak": PEAK[args.precision], "unit": "TFLOP/s",
                     "frac": achieved / PEAK[args.precision],
                     "traffic": measured_traffic(B, d, Ld, args.precision, dom),
                     "flop_per_launch": fl[dom] * B, "avg_launch_ms": kern_ms[dom]},
        "kernels_ms": kern_ms,
        "step_hbm": (lambda tb: None if tb is None else {
            "bytes_per_step": tb, "achieved_TBps": tb / (ms_step * 1e-3) / 1e12, "peak_TBps": HBM_PEAK_TBS,
            "frac": tb / (ms_step * 1e-3) / 1e12 / HBM_PEAK_TBS,
            "compulsory_bytes_per_step": 768 * B})(measured_step_traffic(B, d, Ld, args.precision, dom)),
        "step_tflops_algorithmic": fl["total"] * B * world / (ms_step * 1e-3) / 1e12,
        "settle_steps": r["settle"],
        "loss_mean": r["total"] / args.steps,
    }
    if args.full:
        out["per_step_sync_ms"] = r["per_step_sync_ms"]
    for mode in modes[1:]:
        o = res[mode]
        out[mode] = {"value": o["value"], "unit": "samples/s", "ms_per_step": o["ms_step"], "rows_per_gpu": o["B"],
                     "global_batch": o["Bg"], "n_gpus": o["seen"], "kernels_ms": o["kern_ms"],
                     "small_batch_shape": o["small"]}
    if args.full and world == 1 and not args.no_extra_configs:
        out["extra_configs"] = extra_configs(vpc, dev)
    if args.full and world == 1 and not args.no_cpu_baseline:
        cb = cpu_baseline(B, d, Ld, args.cpu_seconds, args.cpu_threads)
        out["cpu_baseline"] = cb
        out["speedup_vs_cpu"] = value / cb["value"]
    print(json.dumps(out))
    vpc.dp.shutdown()


if __name__ == "__main__":
    main()
