#!/usr/bin/env python3
"""Headline benchmark: weight-columns quantized per second on the synthetic 4096x4096 layer
(BASELINE.json metric; definition in SURVEY.md section 8(d)).

    python bench.py --gpus 1 --steps 3 --warmup 1
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = the complete alternating optimisation of one 4096x4096 layer: K_iter = 10 x (S-solve, T-update,
loss) + best-of-K, i.e. the body of GANQ._perform_quantization_loop after codebook init (ganq.py:525-634), with
W, L, Xxt_damped and T0 already resident in HBM.  value = n_gpus * steps * 4096 / wall time of the timed region
(barrier + synchronize on both sides, max over ranks).

Multi-GPU (weak scaling, no data-path collective in the timed region): every rank quantizes its OWN layer of a
group that shares one set of calibration activations (like q/k/v): rank 0 generates the 128 x 2048 x 4096 fp16
activations and broadcasts them over RCCL/xGMI during setup, every rank accumulates the Hessian with the HIP
kernel and quantizes its layer (seed = rank).  The broadcast time is reported in `setup`.

`--mode rows` (strong scaling): ONE layer whose rows are split over the ranks; value = steps * 4096 / wall time -- the same
layer however many GPUs work on it.  It times what a row-sharded module really costs every rank: a complete `quantize()` on the group's reduced
Hessian -- prologue (two factorisations, replicated), k-means and the fused loop on the rank's row slice, the exchange of the
row losses / chosen rows -- and reports the per-phase seconds of rank 0 (`setup.rows_phases`).  Calibration is data-parallel
there: every rank accumulates the Hessian of ITS share of the sequences and the partial sums meet in one all-reduce
(`setup.hessian_s`, `setup.allreduce_s`).  With more than one GPU the default mode adds the same measurement as the
`row_sharded` object, so one line carries both the weak- and the strong-scaling figure (with --full).

A plain run does only what the headline needs: set-up, warm-up, the timed steps, the outputs of the last step when
--dump-outputs DIR is given, and the result line (`metric`, `value`, `unit`, `ms_per_step`, `setup`, ...).

    python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR   # last step's outputs as DIR/<name>.npy
    python bench.py --gpus 1 --steps 3 --warmup 1 --full                # every object below as well

--dump-outputs writes, from rank 0, what the timed step hands its caller: `codebook` [m,V] float32, `dists` [K] float64,
`best_k` [1] float64 and `indices_sample` (float32 rows of the [m,n] index matrix: all of them when they fit in 32 MiB,
otherwise a fixed, seeded sample of rows, ascending).  The inputs are generated from fixed seeds, so two builds run with the
same arguments can be compared output for output.

With --full the JSON line also carries `roofline` (dominant kernel of the timed region, measured live
with HIP events on the launch stream; `achieved` counts the flops of the rows the launches really solved -- converged
rows are skipped from the third iteration on), `cpu_baseline` (oracle/ganq_oracle.c on this host's cores on a bounded
sample of the same workload, the torch restatement of the reference's own op sequence beside it) and `lut_forward`
(BASELINE configs[2]: the LUT decode kernel against torch fp16 F.linear on the same shapes, device time from HIP-graph
replays, weights hot in the Infinity Cache and cold from HBM), `opt125m` (BASELINE.json's target quantity: whole-model columns/s
on the opt-125m architecture -- 72 linears, 128 x 2048 tokens, K = 10, forward passes included -- next to the C oracle's loop on
the same module shapes) and `ppl` (Wiki2 perplexity through tools/eval_ppl.py when --model-path / --wikitext-path [/ --c4-path]
or GANQ_MODEL_PATH / GANQ_WIKITEXT_PATH / GANQ_C4_PATH name local files; "unmeasured: ..." otherwise -- the boxes have no
network); round 4: `llama32_1b` (whole-model run on the Llama-3.2-1B architecture, BASELINE configs[2]), `stress_3bit`
(V = 8, 512 calibration sequences: Hessian seconds + loop ms, BASELINE configs[4]) and `ppl_tiny` (a TRAINED tiny model:
GPTQ-style PPL of this path next to the reference's own GANQ on the same model and calibration batches).
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs on this driver (already exported on the pool)

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_*_f32 dense peak
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E spec peak (6.29 TB/s measured copy)
INT8_MFMA_PEAK_TOPS = 5000.0    # MI355X_MICROARCH.md: i8 MFMA = 2x the bf16 rate per clock, bf16 dense ~2.5 PF
PMC_FILE = "r04_pmc_traffic.json"      # rocprofv3 --pmc summary of the loop's kernels (tools/pmc_collect.sh); carries the sha256
                                       # of the kernel sources it was collected on -- other sources: traffic is reported as null


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def build_workload(args, dist, dev, warm_quantize=True):
    """synthetic layer of SURVEY 8(d): W = 0.02*randn (fp16-rounded), X = randn * (0.1 + rand(n)) in 128 chunks.
    warm_quantize: time a second complete quantize() on the same statistics (`setup.full_quantize_warm_s`)"""
    import torch.distributed as td
    import torch.nn as nn

    from ganq_amd import _lib
    from ganq_amd import distributed as gdist
    from ganq_amd.looper.named_module import NamedModule
    from ganq_amd.quantization import GANQ, QuantizeConfig

    m, n = args.m, args.n
    seed_rank = getattr(dist, "seed_rank", dist.rank)
    g = torch.Generator(device="cpu").manual_seed(0 + seed_rank)
    lin = nn.Linear(n, m, bias=False).half()
    with torch.no_grad():
        lin.weight.copy_((0.02 * torch.randn(m, n, generator=g)).half())
    lin = lin.to(dev)
    qcfg = QuantizeConfig(bits=args.bits, quant_method="ganq", format="ganq_lut", act_sort="asc", l_damp_style="ganq",
                          dead="mean", damp_percent=0.01, desc_act=True, group_size=128, ganq_iterations=args.iters)

    captured = {}

    class CaptureGANQ(GANQ):
        def _perform_quantization_loop(self, W, Hinv, blocksize, perm=None, invperm=None):
            captured.update(W=W.clone(), Hinv_diag=(Hinv if Hinv.dim() == 1 else torch.diagonal(Hinv)).clone(), L=self.L, H=self.Xxt_damped)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T0 = self._initialize_codebook_kmeans(W, Hinv, self.qcfg.bits, W.device)
            torch.cuda.synchronize()
            captured["kmeans_s"] = time.perf_counter() - t0
            captured["T0"] = T0
            self._initialize_codebook_kmeans = lambda *a, **k: T0  # do not run it twice
            out = super()._perform_quantization_loop(W, Hinv, blocksize, perm, invperm)
            return out

    q = CaptureGANQ(NamedModule(lin, "proj", f"model.layers.0.proj{seed_rank}", 0), qcfg)
    q.quantizer.configure(perchannel=True)

    gs = torch.Generator(device="cpu").manual_seed(999)
    scale = (0.1 + torch.rand(n, generator=gs)).to(dev)
    t_bcast = t_hess = t_allreduce = 0.0
    data_parallel = getattr(args, "mode", "layers") == "rows" and dist.world > 1
    for b in range(args.nseq):
        if data_parallel:
            # data-parallel calibration: rank r generates ("forwards") and accumulates only the sequences b = r (mod world)
            if b % dist.world != dist.rank:
                continue
            gx = torch.Generator(device=dev).manual_seed(1000 + b)
            x = (torch.randn(args.seqlen, n, generator=gx, device=dev) * scale).half()
        elif dist.rank == 0:
            gx = torch.Generator(device=dev).manual_seed(1000 + b)
            x = (torch.randn(args.seqlen, n, generator=gx, device=dev) * scale).half()
        else:
            x = torch.empty((args.seqlen, n), dtype=torch.float16, device=dev)
        if dist.world > 1 and not data_parallel:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gdist.broadcast_tensor(x, 0)  # RCCL over xGMI: calibration activations to every owner rank
            torch.cuda.synchronize()
            t_bcast += time.perf_counter() - t0
        t0 = time.perf_counter()
        q.add_batch(x.unsqueeze(0), None)  # one sequence per call, as the looper's forward hook does
        if b >= args.nseq - dist.world:
            torch.cuda.synchronize()
        t_hess += time.perf_counter() - t0
    torch.cuda.synchronize()
    if data_parallel:  # the partial Hessians meet in ONE all-reduce of n^2 floats (RCCL over xGMI)
        q.hessian  # flush the staged batches outside the timer
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gdist.reduce_group_statistics([q], dist)
        torch.cuda.synchronize()
        t_allreduce = time.perf_counter() - t0
    H_copy, n_copy = q.hessian.clone(), q.nsamples
    t0 = time.perf_counter()
    wq, _, _, _, _, avg_loss, damp = q.quantize()  # full quantize(): prologue + k-means + loop + epilogue
    torch.cuda.synchronize()
    t_full = time.perf_counter() - t0
    t_full_warm = None
    if warm_quantize:
        # the same call again on the same statistics: the first one pays one-time costs (workspaces, library handles)
        q2 = GANQ(NamedModule(lin, "proj", f"model.layers.0.proj{seed_rank}", 0), qcfg)
        q2.quantizer.configure(perchannel=True)
        q2.H, q2.nsamples = H_copy, n_copy
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q2.quantize()
        torch.cuda.synchronize()
        t_full_warm = round(time.perf_counter() - t0, 4)
    captured.update(lin=lin, qcfg=qcfg, H_raw=H_copy, nsamples=n_copy)
    setup = {"hessian_s": round(t_hess, 4), "xgmi_broadcast_s": round(t_bcast, 4), "allreduce_s": round(t_allreduce, 4), "kmeans_s": round(captured["kmeans_s"], 4),
             "full_quantize_s": round(t_full, 4), "full_quantize_warm_s": t_full_warm, "avg_loss": avg_loss, "damp_percent": damp,
             "calib_bytes": args.nseq * args.seqlen * n * 2}
    return captured, setup


def host_cores():
    """CPU threads this process may really use: the smallest of os.cpu_count(), the scheduler affinity mask and the cgroup
    CPU quota (a GPU box hands a one-GPU job a share of a many-core host; running one OpenMP thread per core of the WHOLE host
    inside that share only makes the baseline slower) -> (threads, detail dict)"""
    detail = {"os_cpu_count": os.cpu_count()}
    n = os.cpu_count() or 1
    try:
        detail["sched_affinity"] = len(os.sched_getaffinity(0))
        n = min(n, detail["sched_affinity"])
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                quota, period = txt[0], float(txt[1])
            else:
                quota, period = txt[0], float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota not in ("max", "-1"):
                detail["cgroup_cpu_quota"] = round(float(quota) / period, 2)
                n = min(n, max(1, int(float(quota) / period)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n), detail


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cap, args):
    """CPU figures for the same loop on the box's host cores, on a bounded sample (rows are independent, so layer time
    scales by m/rows; one of the K iterations is timed).  Headline: the C restatement with OpenMP (the faster and
    steadier of the two); next to it the reference's own op sequence on torch CPU (per-column gather + gemv,
    lstsq/gelsd, quad loss), which is what a user of the reference runs."""
    from oracle import c_oracle, ganq_ref

    threads, core_detail = host_cores()  # the box's own host cores, count stated
    log(f"[bench] cpu_baseline on {threads} threads ({core_detail})")
    torch.set_num_threads(threads)
    rows = min(args.cpu_rows, args.m)
    W = cap["W"][:rows].cpu()
    H, L, T0 = cap["H"].cpu(), cap["L"].cpu(), cap["T0"][:rows].cpu()
    timings = []
    t0 = time.perf_counter()
    ganq_ref.run_layer(W, H, L, T0, 1, timings=timings)
    t_ref = time.perf_counter() - t0
    per_layer = t_ref * (args.m / rows) * args.iters
    torch_seq = {"value": round(args.n / per_layer, 4), "unit": "columns/s", "cores": threads,
                 "sample": f"torch op-sequence restatement of ganq.py:533-626 (oracle/ganq_ref.py), {rows} of {args.m} rows x "
                           f"1 of {args.iters} iterations of the same {args.m}x{args.n} layer, {t_ref:.2f} s measured "
                           f"(S-solve {timings[0][0]:.2f} s, T-update {timings[0][1]:.2f} s, loss {timings[0][2]:.2f} s), "
                           f"scaled by rows and iterations",
                 "measured_s": round(t_ref, 3)}
    c_oracle.set_num_threads(threads)
    rows_c = min(4 * rows, args.m)
    Wn, Hn, Ln, Tn = cap["W"][:rows_c].cpu().numpy(), H.numpy(), L.numpy(), cap["T0"][:rows_c].cpu().numpy()
    t0 = time.perf_counter()
    c_oracle.run_layer(Wn, Hn, Ln, Tn, 1)
    t_c = time.perf_counter() - t0
    extra = {}
    if threads > 16:  # rounds 1-2 capped the baseline at 16 threads: kept beside the all-core figure for continuity
        c_oracle.set_num_threads(16)
        t0 = time.perf_counter()
        c_oracle.run_layer(Wn, Hn, Ln, Tn, 1)
        t16 = time.perf_counter() - t0
        c_oracle.set_num_threads(threads)
        extra["c_oracle_16_threads"] = {"value": round(args.n / (t16 * (args.m / rows_c) * args.iters), 4), "cores": 16,
                                         "measured_s": round(t16, 3)}
    return {"value": round(args.n / (t_c * (args.m / rows_c) * args.iters), 4), "unit": "columns/s", "cores": threads,
            "cpu_count": os.cpu_count(), "cores_detail": core_detail, "cpu_model": _cpu_model(), "torch": torch.__version__, "ganq_iterations": args.iters,
            **extra, "kind": "port",
            "sample": f"oracle/ganq_oracle.c (OpenMP, {threads} threads), {rows_c} of {args.m} rows x 1 of {args.iters} iterations "
                      f"of the same {args.m}x{args.n} layer, {t_c:.2f} s measured, scaled by rows and iterations",
            "measured_s": round(t_c, 3), "torch_op_sequence": torch_seq}


def make_sharded_quantize(cap, dist):
    """-> step(timing=False): one complete GANQ.quantize() of the layer on the (already reduced) Hessian with the rows split
    over the ranks (GANQ.row_dist): prologue replicated, k-means + fused loop on the rank's slice, exchange of the row
    losses / chosen rows.  Returns the quantizer (its ganq_stats carry the phase seconds when timing is on)."""
    from ganq_amd.looper.named_module import NamedModule
    from ganq_amd.quantization import GANQ

    def step(timing=False):
        q = GANQ(NamedModule(cap["lin"], "proj", "model.layers.0.proj0", 0), cap["qcfg"])
        q.quantizer.configure(perchannel=True)
        q.H, q.nsamples = cap["H_raw"].clone(), cap["nsamples"]
        q.row_dist, q.time_collectives = dist, timing
        q.force_row_path = True  # also at world = 1: the same code path and phase timers for every N
        q.fwd_counter = 1
        q.quantize()
        return q

    return step


def rows_phases(cap, dist):
    """one extra instrumented sharded quantize(): seconds per phase on this rank"""
    step = make_sharded_quantize(cap, dist)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    q = step(timing=True)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    st = {k: round(v, 5) for k, v in q.ganq_stats.items() if isinstance(v, float) and k.endswith("_s") and k != "enqueue_s"}
    st["prologue_epilogue_s"] = round(total - sum(st.values()), 5)
    st["total_s"] = round(total, 5)
    return st


def opt125m_report(args, cap_unused=None):
    """BASELINE.json's target is written on opt-125m: whole-model quantization of that ARCHITECTURE (random weights -- no
    checkpoint is reachable), 72 linears, 128 x 2048 synthetic tokens, K = 10, forward passes included, as columns/s; beside
    it the C oracle's loop on the three module shapes (one of K iterations on all rows, scaled), i.e. what the CPU needs for
    the loops alone -- its Hessians, k-means and forward passes are not even counted."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import quantize_model_bench as qmb

    from oracle import c_oracle, ganq_ref

    qmb.run("opt-125m", nsamples=16, seqlen=512, batch=8, iters=2, layers=1)  # warm-up: workspaces, library handles
    log("[bench] opt125m: warm-up done")
    rep = qmb.run("opt-125m", nsamples=args.nseq, seqlen=args.seqlen, batch=8, bits=args.bits, iters=args.iters)
    threads, _ = host_cores()
    c_oracle.set_num_threads(threads)
    rng = np.random.default_rng(0)
    cpu_loop_s, ref_loop_s, per_shape = 0.0, 0.0, {}
    torch.set_num_threads(threads)
    for shape, count in rep["module_shapes"].items():
        m, n = (int(v) for v in shape.split("x"))
        W = (0.02 * rng.standard_normal((m, n))).astype(np.float32)
        X = (rng.standard_normal((2 * n, n)) * (0.1 + rng.random(n))).astype(np.float32)
        H = (X.T @ X / n).astype(np.float64)
        H += 0.01 * np.mean(np.diag(H)) * np.eye(n)
        L = np.linalg.cholesky(H + np.diag(np.clip(np.abs(H).sum(1) - 2 * np.diag(H), 1e-8, None))).astype(np.float32)
        T0 = np.quantile(W, (np.arange(2 ** args.bits) + 0.5) / 2 ** args.bits, axis=1).T.astype(np.float32).copy()
        t0 = time.perf_counter()
        c_oracle.run_layer(W, H.astype(np.float32), L, T0, 1)
        dt = time.perf_counter() - t0
        # the reference's own op sequence (per-column gather + gemv, lstsq / gelsd, quad loss: oracle/ganq_ref.py) on a sample of rows
        rows = min(m, 256)
        t0 = time.perf_counter()
        ganq_ref.run_layer(torch.from_numpy(W[:rows]), torch.from_numpy(H.astype(np.float32)), torch.from_numpy(L), torch.from_numpy(T0[:rows]), 1)
        dt_ref = (time.perf_counter() - t0) * (m / rows)
        per_shape[shape] = {"modules": count, "cpu_one_iteration_s": round(dt, 4), "reference_op_sequence_one_iteration_s": round(dt_ref, 3)}
        log(f"[bench] opt125m: {shape}: C oracle {dt:.3f} s, reference op sequence {dt_ref:.2f} s per iteration")
        cpu_loop_s += dt * args.iters * count
        ref_loop_s += dt_ref * args.iters * count
    rep["cpu_loops_only"] = {"kind": "port", "cores": threads, "seconds": round(cpu_loop_s, 2),
                             "columns_per_s": round(rep["weight_columns"] / cpu_loop_s, 2), "per_shape": per_shape,
                             "sample": "oracle/ganq_oracle.c (round 4: 4-5 x faster than in rounds 1-3, same bits), one of K iterations on all rows of "
                                       "each module shape, scaled by K and the module count; Hessian, k-means and forward passes NOT included on the CPU side"}
    rep["cpu_reference_op_sequence_loops_only"] = {
        "kind": "torch restatement of the reference's op sequence (ganq.py:533-626)", "cores": threads, "seconds": round(ref_loop_s, 1),
        "columns_per_s": round(rep["weight_columns"] / ref_loop_s, 2),
        "sample": "oracle/ganq_ref.py, 256 rows x one of K iterations per module shape, scaled by rows, K and the module count"}
    rep["speedup_whole_gpu_run_vs_cpu_loops_only"] = round(rep["columns_per_s_whole_run"] / rep["cpu_loops_only"]["columns_per_s"], 1)
    rep["speedup_whole_gpu_run_vs_reference_op_sequence_loops_only"] = round(
        rep["columns_per_s_whole_run"] / rep["cpu_reference_op_sequence_loops_only"]["columns_per_s"], 1)
    rep["target"] = (">= 50x the reference CPU columns/s on opt-125m 4-bit (BASELINE.json): measured against the reference's op sequence "
                     "AND against this repository's much faster C port")
    return rep


def llama32_1b_report(args):
    """BASELINE.json configs[2]: whole-model quantization of the Llama-3.2-1B ARCHITECTURE (random weights -- no checkpoint is
    reachable), 112 linears, 128 x 2048 synthetic tokens, K = 10, forward passes included, as columns/s"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import quantize_model_bench as qmb

    qmb.run("llama-3.2-1b", nsamples=16, seqlen=512, batch=8, iters=2, layers=1)  # warm-up: workspaces, library handles
    rep = qmb.run("llama-3.2-1b", nsamples=args.nseq, seqlen=args.seqlen, batch=8, bits=args.bits, iters=args.iters)
    rep["what"] = "Llama-3.2-1B architecture at its real dimensions, random weights, whole run incl. forward passes, Hessians, k-means"
    return rep


def stress_3bit_report(args, dist, dev):
    """BASELINE.json configs[4]: 3-bit (V = 8), 512 calibration sequences (p = 1 M tokens) on the 4096 x 4096 layer: the
    Hessian accumulation of all 512 x 2048 tokens (seconds) and the K = 10 loop (ms), the same definitions as the headline"""
    import copy

    from ganq_amd import _lib

    a = copy.copy(args)
    a.bits, a.nseq, a.mode = 3, 512, "layers"
    cap, setup = build_workload(a, dist, dev)
    ws = _lib.run_layer_workspace(a.m, a.n, 8, dev)
    for _ in range(2):
        out = _lib.run_layer(cap["W"], cap["H"], cap["L"], cap["T0"], a.iters, alias_q=True, workspace=ws)
    torch.cuda.synchronize()
    steps = 5
    t0 = time.perf_counter()
    for _ in range(steps):
        out = _lib.run_layer(cap["W"], cap["H"], cap["L"], cap["T0"], a.iters, alias_q=True, workspace=ws)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    tokens = a.nseq * a.seqlen
    return {"what": f"synthetic {a.m}x{a.n} layer, 3-bit (V=8), K={a.iters}, {a.nseq}x{a.seqlen} fp16 calibration tokens (BASELINE configs[4])",
            "hessian_s": setup["hessian_s"], "hessian_tokens": tokens,
            "hessian_TFLOPs_by_2pn2": round(2.0 * tokens * a.n * a.n / setup["hessian_s"] / 1e12, 1),
            "kmeans_s": setup["kmeans_s"], "full_quantize_warm_s": setup["full_quantize_warm_s"],
            "loop_ms": round(dt * 1e3, 3), "columns_per_s": round(a.n / dt, 1),
            "dists": [round(float(x), 6) for x in out[2].cpu().tolist()], "best_k": int(out[3])}


def ppl_tiny_report():
    """The PPL half of the metric on TRAINED weights without a download: the committed tiny OPT model (tests/golden/tiny_lm,
    trained on text that ships with the interpreter) quantized by this path on the calibration batches the reference's own
    GANQ was given; GPTQ-style PPL on held-out text next to the fixture's fp / reference-GANQ figures."""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_tiny_lm as tiny

    from ganq_amd.models.quantize import gptq_style_ppl, quantize_model
    from ganq_amd.quantization import QuantizeConfig

    fx = np.load(os.path.join(ROOT, "tests", "golden", "tiny_lm", "fixture.npz"))
    ev = torch.from_numpy(fx["eval_ids"].astype(np.int64))
    out = {"what": "4-layer OPT architecture (hidden 256), trained; 4-bit GANQ K=10 with the reference's recipe, 64 x 512 calibration "
                   "tokens; GPTQ-style PPL (byte-level tokens) on held-out text; reference = the reference's own GANQ object on the CPU "
                   "(tests/golden/make_golden_tiny_lm.py)",
           "ppl_fp_reference_run": round(float(fx["ppl_fp"]), 4), "ppl_ganq_reference": round(float(fx["ppl_ref"]), 4),
           "ppl_ganq_reference_8_runs_1e-6_input_noise": {"mean": round(float(np.mean(fx["ppl_ref_runs"])), 4),
                                                          "std": round(float(np.std(fx["ppl_ref_runs"], ddof=1)), 4),
                                                          "min": round(float(np.min(fx["ppl_ref_runs"])), 4),
                                                          "max": round(float(np.max(fx["ppl_ref_runs"])), 4)}}
    ref_mean, ref_std = float(np.mean(fx["ppl_ref_runs"])), float(np.std(fx["ppl_ref_runs"], ddof=1))
    for tag, dtype, fmt in (("fp32_fake", torch.float32, "fake"), ("fp16_packed", torch.float16, "ganq_lut")):
        model = tiny.load_model(dtype).cuda()
        qcfg = QuantizeConfig(bits=4, quant_method="ganq", format=fmt, act_sort="asc", l_damp_style="ganq", dead="mean",
                              desc_act=True, ganq_iterations=10, group_size=128, damp_percent=0.01)
        batches = [torch.from_numpy(fx["calib"][i:i + 1].astype(np.int64)).cuda() for i in range(fx["calib"].shape[0])]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        quantize_model(model, batches, qcfg)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ppl = gptq_style_ppl(model, ev, seqlen=int(fx["seq"]))
        out[f"ppl_ganq_hip_{tag}"] = round(ppl, 4)
        out[f"delta_vs_reference_mean_{tag}"] = round(ppl - ref_mean, 4)
        out[f"sigmas_from_reference_mean_{tag}"] = round((ppl - ref_mean) / ref_std, 2)
        out[f"quantize_s_{tag}"] = round(dt, 3)
    out["within_3_sigma_of_reference_runs"] = bool(abs(out["delta_vs_reference_mean_fp32_fake"]) <= max(0.05, 3 * ref_std))
    out["note"] = ("the metric's +-0.05 is below this 3.4 M-parameter model's noise floor: the reference's OWN PPL moves by std "
                   f"{ref_std:.3f} under 1e-6 relative noise on the calibration activations (tests/test_tiny_lm.py)")
    return out


def ppl_report(args):
    """Wiki2 PPL of opt-125m fp16 / GANQ 4-bit (README.md:21-27 of the reference) when the files are on this box"""
    model = args.model_path or os.environ.get("GANQ_MODEL_PATH")
    wiki = args.wikitext_path or os.environ.get("GANQ_WIKITEXT_PATH")
    c4 = args.c4_path or os.environ.get("GANQ_C4_PATH")
    if not (model and os.path.exists(model) and wiki and os.path.exists(wiki)):
        return "unmeasured: no checkpoint / dataset on this box (pass --model-path --wikitext-path [--c4-path] or set " \
               "GANQ_MODEL_PATH / GANQ_WIKITEXT_PATH / GANQ_C4_PATH; reference: opt-125m fp16 27.65, GANQ 4-bit 28.45)"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_ppl

    calib = "c4" if (c4 and os.path.exists(c4)) else "wikitext2"
    out = eval_ppl.evaluate(model, wiki, c4, calib=calib, nsamples=32, seqlen=2048, bits=args.bits, iters=args.iters)
    out.pop("modules", None)
    return out


class _SameSeed:
    """a Dist whose `rank` reads 0 where build_workload derives seeds / names from it, so that every rank builds the same
    layer (row-sharded mode); broadcasts still see the real rank"""

    def __init__(self, dist):
        self._d = dist
        self.world = dist.world
        self.device = dist.device
        self.rank = dist.rank
        self.seed_rank = 0


def lut_forward_report():
    """GanqHipQuantLinear decode forward vs torch fp16 F.linear (BASELINE configs[2]) -- tools/bench_lut_decode.py"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_lut_decode as bl

    rows = []
    for (m, n, M, cold) in [(4096, 4096, 1, False), (4096, 4096, 1, True), (14336, 4096, 1, True), (4096, 14336, 1, True),
                            (4096, 4096, 16, True)]:
        rows.append(bl.bench(m, n, 4, M, cold))
    # BASELINE configs[2]: the seven linears of one Llama-3.2-1B decoder layer at decode (M = 1), cold
    layer = {"q_proj": (2048, 2048), "k_proj": (512, 2048), "v_proj": (512, 2048), "o_proj": (2048, 2048),
             "gate_proj": (8192, 2048), "up_proj": (8192, 2048), "down_proj": (2048, 8192)}
    per_shape = {}
    for shape in sorted(set(layer.values())):
        per_shape[shape] = bl.bench(shape[0], shape[1], 4, 1, True)
        rows.append(per_shape[shape])
    lut_us = sum(per_shape[s]["lut_us"] for s in layer.values())
    f16_us = sum(per_shape[s]["torch_fp16_us"] for s in layer.values())
    # prefill (M >= 2048): the LUT forward (round 4: dequantise once + the hand-written dense GEMM of csrc/gemm_h16.hip from
    # ~1024 rows on, the fused LUT-dequant GEMM below) against the library fp16 GEMM on the pre-dequantised weight and against
    # dequant + library
    import bench_lut_gemm as bg

    gemm = []
    for (m, n) in [(4096, 4096), (14336, 4096), (4096, 14336)]:
        for M in (2048, 4096):
            r = bg.bench(m, n, M)
            gemm.append({k: r[k] for k in ("out_x_in", "M", "lut_gemm_us", "lib_fp16_gemm_us", "dequant_plus_lib_us", "lut_gemm_TFLOPs",
                                           "lib_TFLOPs", "vs_lib", "vs_dequant_plus_lib")})
    floor_us = bl.launch_floor()
    for r in rows:  # the share of a call that is the harness's launch floor, and the rate over the rest
        r["GBs_above_launch_floor"] = round(r["m"] * r["n"] * r["bits"] / 8 / max(r["lut_us"] - floor_us, 1e-3) / 1e3, 1)
    return {"gemm": gemm, "what": "y = x @ dequant(qweight, lut)^T, 4-bit, fp16 activations; device us per call from HIP-graph replays of 200 calls; "
                    "cold = a ring of layers larger than the 256 MB Infinity Cache", "peak_GBs": HBM_PEAK_GBS,
            "launch_floor_us": floor_us, "launch_floor_what": "a 1 KB fill kernel, 200 dependent launches in the same HIP graph: what any kernel costs here",
            "shapes": rows,
            "llama32_1b_decoder_layer_M1_cold": {"linears": 7, "lut_us": round(lut_us, 2), "torch_fp16_us": round(f16_us, 2),
                                                 "speedup": round(f16_us / lut_us, 2)}}


def executed_rows(cap, args):
    """rows the S-solve launches of one layer really solve: all of them in iterations 0 and 1, afterwards the rows whose
    indices changed in the previous iteration (run_layer.hip); from one extra untimed run with the indices recorded"""
    from ganq_amd import _lib

    rec = _lib.run_layer_rows(cap["W"], cap["H"], cap["L"], cap["T0"], args.iters, alias_q=True, want_q_all=True)
    Qa = rec["Q_all"]
    m = Qa.shape[1]
    rows = [m, m]
    for k in range(2, args.iters):
        changed = int((Qa[k - 1] != Qa[k - 2]).any(dim=1).sum())
        rows.append((changed + 15) // 16 * 16 if changed else 0)  # whole 16-row workgroup tiles
    return rows[:args.iters]


DUMP_INDEX_BYTES = 32 << 20  # float32 rows of the index matrix written by --dump-outputs (the whole dump stays under 64 MB)


def dump_outputs(out, dirpath):
    """the arrays the timed step returns to its caller, as DIR/<name>.npy in float32 / float64: codebook, dists, best_k and
    the index matrix (a fixed, seeded sample of its rows when all of them would exceed DUMP_INDEX_BYTES)"""
    import numpy as np

    T, Q, dists, best_k = out
    os.makedirs(dirpath, exist_ok=True)
    arrays = {"dists": dists.double().cpu().numpy(), "best_k": np.array([int(best_k)], dtype=np.float64)}
    if T is not None:
        arrays["codebook"] = T.float().cpu().numpy()
    if Q is not None:
        m, n = Q.shape
        keep = max(1, DUMP_INDEX_BYTES // (4 * n))
        rows = torch.arange(m) if keep >= m else torch.from_numpy(np.sort(np.random.default_rng(0).choice(m, keep, replace=False)))
        arrays["indices_sample"] = Q[rows.to(Q.device)].float().cpu().numpy()
    for name, a in arrays.items():
        np.save(os.path.join(dirpath, name + ".npy"), a)
    log(f"[bench] outputs of the last step -> {dirpath}: " + ", ".join(f"{k} {tuple(v.shape)}" for k, v in arrays.items()))


def roofline_report(prof_all, prof, dom_name, exec_rows, exec_frac, elapsed, args, dist):
    """`roofline`, `path_hbm` and `kernels` of the full line: the dominant kernel of the timed region from its HIP events,
    the whole-path algorithmic bytes over the loop time, and the per-kernel table of the instrumented step"""
    m, n, K, V = args.m, args.n, args.iters, 2 ** args.bits
    kern = {k: {"total_ms": round(v[0], 3), "launches": v[1], "avg_ms": round(v[0] / v[1], 4)} for k, v in prof_all.items()}
    dom_ms, dom_cnt = prof[dom_name]  # HIP events over the timed region, on the stream the kernel is launched on
    avg_s = dom_ms / dom_cnt / 1e3
    if dom_name == "solve_s_kernel":
        # residual chain: n(n-1)/2 fused multiply-adds per SOLVED row on the fp32 matrix cores; converged rows are
        # skipped from the third iteration on, so the flops are those of the rows the launches really solved
        m_loc = m if args.mode == "layers" else (m + dist.world - 1) // dist.world
        work_full = float(m_loc) * n * (n - 1)
        work = work_full * exec_frac
        roof = {"kernel": dom_name, "bound": "mfma", "achieved": round(work / avg_s / 1e12, 3),
                "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "peak_dtype": "f32",
                "executed_rows_per_iteration": exec_rows, "executed_fraction_of_reference_flops": round(exec_frac, 4),
                "achieved_if_all_rows_counted": round(work_full / avg_s / 1e12, 3)}
    elif dom_name == "onehot_accum_kernel":
        # bucket sum of H per row on the int8 matrix cores: one-hot [16 codes] x 4 digit planes, pairs u > v only
        work = 2.0 * 16 * 4 * m * n * (n - 1) / 2
        roof = {"kernel": dom_name, "bound": "mfma", "achieved": round(work / avg_s / 1e12, 3),
                "peak": INT8_MFMA_PEAK_TOPS, "unit": "TFLOP/s", "peak_dtype": "i8 (dense, 2x bf16)"}
    elif dom_name == "gemm_f32_kernel":
        work = 2.0 * m * n * n
        roof = {"kernel": dom_name, "bound": "mfma", "achieved": round(work / avg_s / 1e12, 3),
                "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "peak_dtype": "f32"}
    else:
        nbytes = 4.0 * n * n + 1.0 * m * n
        roof = {"kernel": dom_name, "bound": "hbm", "achieved": round(nbytes / avg_s / 1e9, 2), "peak": HBM_PEAK_GBS,
                "unit": "GB/s"}
    roof["frac"] = round(roof["achieved"] / roof["peak"], 5)
    roof["avg_launch_ms"] = round(dom_ms / dom_cnt, 4)
    # HBM bytes per launch from the PMC counters of a separate rocprofv3 --pmc pass over the same kernels
    # (profiles/<PMC_FILE>, tools/pmc_collect.sh; FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950)
    roof["traffic"] = None
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from pmc_parse import csrc_digest

        pmc = json.load(open(os.path.join(ROOT, "profiles", PMC_FILE)))
        if pmc.get("_csrc_sha256") != csrc_digest(ROOT):
            roof["traffic_note"] = f"profiles/{PMC_FILE} was collected on other kernel sources than the ones running: not reported"
        else:
            for k, v in pmc.items():
                if k.split("<")[0] == dom_name and (m, n) == (4096, 4096):
                    roof["traffic"] = int((2.0 * v["FETCH_SIZE_KB_avg"] + v["WRITE_SIZE_KB_avg"]) * 1024)
                    roof["traffic_source"] = f"profiles/{PMC_FILE} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, FETCH_SIZE x2 for gfx950)"
    except (OSError, ValueError, KeyError, AttributeError):
        pass
    # whole-path HBM view: algorithmic bytes of the loop per layer / loop time
    b_loop = K * (15.0 * m * n + 10.0 * n * n + 8.0 * m * V)
    path_gbs = b_loop / (elapsed / args.steps) / 1e9
    path_hbm = {"algorithmic_GB_per_layer": round(b_loop / 1e9, 3), "achieved_GBs": round(path_gbs, 2),
                "frac_of_peak": round(path_gbs / HBM_PEAK_GBS, 5)}
    return roof, path_hbm, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layer-m", dest="m", type=int, default=4096)
    ap.add_argument("--layer-n", dest="n", type=int, default=4096)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10, help="GANQ iterations K (README PPL numbers use 10)")
    ap.add_argument("--nseq", type=int, default=128)
    ap.add_argument("--seqlen", type=int, default=2048)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last step as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: per-kernel table and roofline, row-sharded quantize(), "
                         "CPU baseline, LUT forward, whole-model runs, 3-bit stress, PPL objects")
    ap.add_argument("--cpu-rows", type=int, default=1024)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the cpu_baseline object")
    ap.add_argument("--no-lut", action="store_true", help="with --full: skip the lut_forward object")
    ap.add_argument("--no-opt125m", action="store_true", help="with --full: skip the opt125m object (whole-model run on the opt-125m architecture)")
    ap.add_argument("--no-llama", action="store_true", help="with --full: skip the llama32_1b object (whole-model run on the Llama-3.2-1B architecture)")
    ap.add_argument("--no-stress", action="store_true", help="with --full: skip the stress_3bit object (V = 8, 512 calibration sequences)")
    ap.add_argument("--no-tiny", action="store_true", help="with --full: skip the ppl_tiny object (trained tiny model, PPL vs the reference's GANQ)")
    ap.add_argument("--model-path", default=None, help="with --full: local HF model directory: adds measured Wiki2 PPL (fp16 / GANQ) to the line")
    ap.add_argument("--wikitext-path", default=None)
    ap.add_argument("--c4-path", default=None)
    ap.add_argument("--mode", choices=["layers", "rows"], default="layers",
                    help="layers: one layer per GPU (weak scaling, the default); rows: one layer, rows split over the GPUs (strong)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    from ganq_amd import _lib
    from ganq_amd import distributed as gdist

    dist = gdist.init_from_env()
    if dist.world != args.gpus:
        log(f"warning: --gpus {args.gpus} but WORLD_SIZE={dist.world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    dev = dist.device
    _lib.selftest()
    import torch.distributed as td

    if args.mode == "rows":
        cap, setup = build_workload(args, _SameSeed(dist), dev, warm_quantize=args.full)  # every rank needs the SAME layer
    else:
        cap, setup = build_workload(args, dist, dev, warm_quantize=args.full)
    V = 2 ** args.bits
    ws = _lib.run_layer_workspace(args.m, args.n, V, dev)

    if args.mode == "rows":
        sharded_step = make_sharded_quantize(cap, dist)

        def step():
            q = sharded_step()
            return q.ganq_codebook, q.ganq_indices, q.ganq_stats["dists"], q.ganq_stats["best_k"]
    else:
        def step():
            return _lib.run_layer(cap["W"], cap["H"], cap["L"], cap["T0"], args.iters, alias_q=True, workspace=ws)

    log(f"[bench] workload ready: {setup}")
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    prof_all = dom_name = None
    if args.full:
        # per-kernel breakdown: ONE extra untimed step with every kernel instrumented.  The events of a fully instrumented
        # run sit between dependent launches and cost about 1 ms of idle time per layer, so the timed steps below carry
        # events only around the dominant kernel (the one the roofline object is about).
        _lib.profile_enable(True)
        step()
        prof_all = _lib.profile_report()
        _lib.profile_enable(False)
        dom_name = max(prof_all.items(), key=lambda kv: kv[1][0])[0]
        if args.mode == "rows" and "solve_s_kernel" in prof_all:
            dom_name = "solve_s_kernel"  # the roofline object stays on the loop's dominant kernel (k-means is outside t_loop)
    torch.cuda.synchronize()
    if dist.world > 1:
        td.barrier()
    if args.full:
        _lib.profile_enable(True, only=dom_name)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    if dist.world > 1:
        td.barrier()
    elapsed = time.perf_counter() - t0
    log(f"[bench] timed region: {args.steps} steps in {elapsed:.4f} s")
    prof = None
    if args.full:
        prof = _lib.profile_report()
        _lib.profile_enable(False)
    if dist.world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        if td.get_backend() != "gloo":
            t = t.to(dev)
        td.all_reduce(t, op=td.ReduceOp.MAX)
        elapsed = float(t)
    if args.dump_outputs and dist.rank == 0:
        dump_outputs(out, args.dump_outputs)

    # strong-scaling figure: the SAME layer (rank 0's) quantized by all ranks together -- data-parallel statistics are
    # already reduced in rows mode; in layers mode rank 0's weight and Hessian are broadcast first
    row_sharded = phases = None
    if args.full and args.mode == "rows":
        phases = rows_phases(cap, dist)
    elif args.full:  # every N (also 1): the complete row-sharded quantize() of rank 0's layer, with its phases
        if dist.world > 1:
            gdist.broadcast_tensor(cap["lin"].weight.data, 0)
            gdist.broadcast_tensor(cap["H_raw"], 0)
        sharded_step = make_sharded_quantize(cap, dist)
        sharded_step()
        phases = rows_phases(cap, dist)
        torch.cuda.synchronize()
        if dist.world > 1:
            td.barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            sharded_step()
        torch.cuda.synchronize()
        if dist.world > 1:
            td.barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev if (dist.world > 1 and td.get_backend() != "gloo") else "cpu")
        if dist.world > 1:
            td.all_reduce(t, op=td.ReduceOp.MAX)
        row_sharded = {"what": "ONE 4096x4096 layer, complete quantize() on the reduced Hessian (prologue replicated; k-means + fused "
                               "loop on each rank's row slice; exchange of row losses / chosen rows), rows split over the GPUs: strong scaling",
                       "columns_per_s": round(args.steps * args.n / float(t), 2), "ms_per_layer": round(float(t) / args.steps * 1e3, 3),
                       "single_gpu_full_quantize_warm_ms": round(setup["full_quantize_warm_s"] * 1e3, 3), "phases_rank0_s": phases}

    exec_rows, exec_frac = None, 1.0
    if args.full and dist.rank == 0 and args.mode == "layers":
        exec_rows = executed_rows(cap, args)
        exec_frac = sum(exec_rows) / float(args.m * args.iters)
    if dist.rank == 0:
        m, n, K = args.m, args.n, args.iters
        value = (dist.world if args.mode == "layers" else 1) * args.steps * n / elapsed
        result = {
            "metric": "weight-columns quantized/sec @4096x4096 (GANQ 4-bit, K=10 alternating-optimisation loop)",
            "value": round(value, 2), "unit": "columns/s", "n_gpus": dist.world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak" if args.mode == "layers" else "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"synthetic {m}x{n} layer, {args.bits}-bit (V={V}), K={K}, act_sort=asc, "
                                   f"l_damp_style=ganq, {args.nseq}x{args.seqlen} fp16 calibration tokens; "
                                   + ("one layer per GPU" if args.mode == "layers" else "ONE layer, rows split over the GPUs"),
                       "m": m, "n": n, "bits": args.bits, "ganq_iterations": K, "mode": args.mode,
                       "parallelism": f"layers x{dist.world}" if args.mode == "layers" else f"rows /{dist.world}"},
            "column_steps_per_s": round(value * K, 1),
        }
        if args.full:
            roof, path_hbm, kern = roofline_report(prof_all, prof, dom_name, exec_rows, exec_frac, elapsed, args, dist)
            result.update({
                "roofline": roof, "path_hbm": path_hbm, "kernels": kern,
                "kernels_note": "one extra untimed step with every kernel instrumented; the timed steps carry HIP events around "
                                f"{dom_name} only (events between dependent launches cost idle time)"})
        result.update({
            "setup": setup,
            "dists_last_step": [round(float(x), 6) for x in out[2].cpu().tolist()], "best_k": int(out[3]),
            "parity": "this exact workload, K = 10, is checked against the CPU oracle by tests/test_hip_configs.py::"
                      "test_bench_workload_k10_vs_oracle (indices bit-exact, codebooks <= 1e-5, row losses <= 1e-6)",
        })
        if phases is not None and args.mode == "rows":
            result["setup"]["rows_phases"] = phases
        if row_sharded is not None:
            result["row_sharded"] = row_sharded
        if args.full and dist.world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(cap, args)
            result["speedup_vs_cpu_baseline"] = round(value / result["cpu_baseline"]["value"], 1)
        if args.full and dist.world == 1 and not args.no_lut:
            cap = ws = None  # free the layer before the rings of weights are allocated
            torch.cuda.empty_cache()
            log("[bench] lut_forward ...")
            result["lut_forward"] = lut_forward_report()
        if args.full and dist.world == 1 and not args.no_opt125m:
            log("[bench] opt125m (whole-model run on the architecture + C oracle loops) ...")
            cap = ws = None
            torch.cuda.empty_cache()
            result["opt125m"] = opt125m_report(args)
        if args.full and dist.world == 1 and not args.no_llama:
            log("[bench] llama32_1b (whole-model run on the architecture) ...")
            torch.cuda.empty_cache()
            result["llama32_1b"] = llama32_1b_report(args)
        if args.full and dist.world == 1 and not args.no_stress:
            log("[bench] stress_3bit (V = 8, 512 sequences) ...")
            torch.cuda.empty_cache()
            result["stress_3bit"] = stress_3bit_report(args, dist, dev)
        if args.full and dist.world == 1 and not args.no_tiny:
            log("[bench] ppl_tiny (trained tiny model vs the reference's GANQ) ...")
            torch.cuda.empty_cache()
            result["ppl_tiny"] = ppl_tiny_report()
        if args.full and dist.world == 1:
            result["ppl"] = ppl_report(args)
        print(json.dumps(result), flush=True)
    if dist.world > 1:
        td.barrier()
        td.destroy_process_group()


if __name__ == "__main__":
    main()
