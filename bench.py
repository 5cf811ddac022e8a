#!/usr/bin/env python
"""Benchmark of the GNN-RAG reasoning hot path on MI355X.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A "step" = one pass of the hot path over one batch of synthetic question subgraphs:
T x L consecutive ReasonGNNLayer.forward calls (T = 1 for the C2 / C4 / C5 workloads, 3 for the WebQSP-shaped C1 / C3:
the released checkpoint's num_iter), i.e. per iteration L calls (relation transform + typed-edge aggregation +
gated update + score + masked softmax each) starting from the seed distribution, exactly as
one iteration of ReaRev.forward drives the layer (reference rearev.py:206-211).  Inputs
(CSR structure, features, parameters) are resident in HBM when the timed region starts; the
CSR build is timed separately and reported as ``csr_build_ms``.

Workload (BASELINE.json configs[1], the config the metric is quoted on): synthetic
Freebase-shaped subgraphs, 2000 nodes / 10000 typed edges (+2000 self loops) per question,
batch 64 per GPU, 3 layers, hidden 200, 2 instructions, fp32.

With N > 1 every rank owns its own 64 questions (question-sharded, weak scaling) and ends
each step with ONE all-gather of the scored nodes (pred_dist) over RCCL.

Prints ONE JSON line (rank 0).  value = typed KG edges aggregated per second, whole job:
N * B * E * L * K / t  (t = max over ranks of the barrier-bracketed wall time of K steps).

A plain run only sets up, warms up, times the K steps and prints that line.  --full adds the side measurements
(step-time spread, exact-fp32 loop, structure-build timings, roofline, CPU baseline with parity_in_run, other workloads,
e2e, train_step).  --dump-outputs DIR writes what the last timed step returned as .npy files (see dump_outputs).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time


def _cpu_budget():
    """os.cpu_count() capped by the cgroup-v2 CFS quota (no package import: the parent of a self-launch only sizes pools)."""
    budget = os.cpu_count() or 1
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            budget = min(budget, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return budget


def _limit_thread_pools_early():
    """Before numpy / torch are imported: the default size of every CPU thread pool of this process (OpenMP, OpenBLAS,
    MKL) follows the visible hardware threads (256 on the MI355X box), not the container's CPU quota (16 cores there).
    Pools that size spin the quota away and the kernel then parks every thread of the process for the rest of a 100 ms
    period - including the one that enqueues the timed steps (seen as 24-36 ms of silence inside a 30 ms timed region,
    profiles/r05n_host_stall_in_timed_region.txt).  min(8, quota / 2) threads per pool unless the variable is already
    set; GNNRAG_HOST_THREADS=0 leaves everything as it is.  The CPU-baseline legs size their own teams later."""
    if os.environ.get("GNNRAG_HOST_THREADS") == "0":
        return
    budget = _cpu_budget()
    # the ranks of one node share the quota (same rule as gnnrag_amd.install.host_thread_limit, restated here because
    # nothing of the package may be imported before the pools are sized)
    lw = os.environ.get("LOCAL_WORLD_SIZE") or os.environ.get("WORLD_SIZE") or "1"
    local = int(lw) if lw.isdigit() and int(lw) > 0 else 1
    n = str(max(1, min(8, budget // (2 * local))))
    for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "NUMEXPR_NUM_THREADS"):
        os.environ.setdefault(k, n)


_limit_thread_pools_early()

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBPS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6.3 TB/s achievable
FP32_MFMA_PEAK_TFLOPS = 157.3
BF16_MFMA_PEAK_TFLOPS = 2500.0   # dense bf16 (MI355X_MICROARCH.md); a bf16x3 kernel issues 6 bf16 MFMAs per fp32-equivalent
                                 # product, so its ceiling in fp32-equivalent flops is 2500 / 6 = 417 TFLOP/s


PARITY_BAR = 1e-4           # north_star: answer-node scores within 1e-4 (fp32) of the reference CPU path


def parity_in_run(gpu_results, ref, cfg):
    """GPU results of the timed configuration against the reference's own ReasonGNNLayer (host cores, the cpu_baseline
    leg's last pass) on the IDENTICAL batch: per math mode the largest |dist_gpu - dist_ref| over all L layers' answer
    distributions and all B x N node slots, the final node state relative to its largest entry, and whether every
    question's argmax (= its Hits@1 decision) is the same.  ``ok`` is False - and bench.py exits non-zero - above 1e-4
    or when an argmax differs for a question whose two best reference scores are further apart than the bar."""
    out = {"questions": int(cfg.B), "layers": int(cfg.L), "bar": PARITY_BAR, "ok": True,
           "against": "the reference's own ReasonGNNLayer (oracle/_ref/gnn, torch CPU), same seeded batch, features and "
                      "parameters as the timed steps"}
    ref_dist = [np.asarray(d, dtype=np.float64) for d in ref["dist"]]
    ref_h = np.asarray(ref["h"], dtype=np.float64)
    hmax = float(np.abs(ref_h).max())
    top2 = np.sort(ref_dist[-1], axis=1)[:, -2:]
    gap = top2[:, 1] - top2[:, 0]
    for name, g in gpu_results.items():
        dd = [float(np.abs(np.asarray(a, dtype=np.float64) - b).max()) for a, b in zip(g["dist"], ref_dist)]
        dh = float(np.abs(np.asarray(g["h"], dtype=np.float64) - ref_h).max()) / max(hmax, 1e-30)
        am_g, am_r = np.asarray(g["dist"][-1]).argmax(1), ref_dist[-1].argmax(1)
        diff = np.nonzero(am_g != am_r)[0]
        # (a distribution over ~N candidates has entries of ~1/N: the error relative to the largest probability beside it)
        dr = max(float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(b.max(), 1e-30)) for a, b in zip(g["dist"], ref_dist))
        o = {"max_abs_dist": max(dd), "max_abs_dist_per_layer": dd, "max_dist_err_rel_to_largest_prob": dr, "max_rel_h": dh,
             "argmax_equal": bool(len(diff) == 0), "argmax_equal_questions": int(cfg.B - len(diff))}
        if "timed_loop_last_step_bit_identical" in g:
            o["timed_loop_last_step_bit_identical"] = g["timed_loop_last_step_bit_identical"]
        if len(diff):
            o["argmax_differs_only_at_reference_ties"] = bool((gap[diff] <= PARITY_BAR).all())
        o["ok"] = bool(max(dd) <= PARITY_BAR and dh <= PARITY_BAR and (len(diff) == 0 or o["argmax_differs_only_at_reference_ties"])
                       and g.get("timed_loop_last_step_bit_identical", True))
        out[name] = o
        out["ok"] = out["ok"] and o["ok"]
    first = next(iter(gpu_results), None)
    if first is not None:        # the headline figures: the timed configuration's
        for k in ("max_abs_dist", "max_rel_h", "argmax_equal"):
            out[k] = out[first][k]
        out["math_of_headline"] = first
    return out


def bytes_agg(cfg, F_g: int) -> float:
    """Algorithmic HBM bytes of ONE aggregation layer call (pinned):
    two CSRs (row_ptr + src + rel, int32), dist read, agg write, T tables once, instructions."""
    per_graph = 2 * ((cfg.N + 1) + 2 * F_g) * 4 + cfg.N * 4 + cfg.N * 2 * cfg.I * cfg.D * 4
    total = cfg.B * per_graph + 2 * cfg.R1 * cfg.D * 4 + cfg.B * cfg.I * cfg.D * 4
    if cfg.normalized_gnn:
        total += 2 * F_g * 4 * cfg.B
    return float(total)


def flops_update(cfg) -> float:
    return 2.0 * cfg.B * cfg.N * (2 * cfg.I + 1) * cfg.D * cfg.D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: the chip needs ~20 steps after an idle period before its clocks (and the step time) settle - measured
    # series at C2: 1.13, 0.91, 0.94, 0.98, ... 0.86 after 20 steps, p50 0.845 (tools/probe/spread_probe.py) - so the
    # default warm-up covers that ramp
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: every rank owns its own cfg.B questions; strong: ONE global batch of cfg.B questions is "
                         "split over the ranks by facts (the WebQSP-dev mode of SURVEY.md section 8e)")
    ap.add_argument("--dry-run-cpu", action="store_true",
                    help="CI only: the multi-rank skeleton on CPU (gloo, the oracle as the per-rank step, tiny batch)")
    ap.add_argument("--spread-steps", type=int, default=200,
                    help="extra steps timed one by one after the timed region (step-time spread); 0 = off")
    ap.add_argument("--launch", choices=["eager", "graph"], default="eager",
                    help="eager: one gnnrag_reason_stack call per step; graph: the step captured once as a hipGraph "
                         "(gnnrag_reason_stack_capture) and replayed")
    ap.add_argument("--cpu-sample-b", type=int, default=None,
                    help="questions of the CPU-baseline sample (the reference's own layer on the host cores); default: the "
                         "workload's whole per-GPU batch up to 64 questions of C2 size (C2: all 64), 4 for the larger shapes")
    ap.add_argument("--no-e2e", action="store_true",
                    help="skip the end-to-end block (unmodified main.py --is_eval on the staged dataset, GPU and CPU)")
    ap.add_argument("--other-workloads", default="C3,C4,C5",
                    help="comma-separated workloads timed in short legs of their own after the main run (default bench at "
                         "--workload C2 on one GPU only; '' = none): the other BASELINE shapes in the driver-run line")
    ap.add_argument("--clock-ramp-ms", type=float, default=600.0,
                    help="keep the chip busy with HBM copy kernels for this long before the warm-up steps (clock ramp of an "
                         "idle chip); 0 = off")
    ap.add_argument("--fp32-steps", type=int, default=20,
                    help="steps of the additional exact-fp32 timed loop (ms_per_step_fp32); 0 = off")
    ap.add_argument("--math", choices=["default", "fp32", "bf16x3", "mixed"], default="default",
                    help="math mode of the dense projections (default = the library's default)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline figure: step-time spread, exact-fp32 loop, structure-build "
                         "timings, roofline, CPU baseline and parity_in_run, other workloads, e2e and train_step legs.  "
                         "Without it a run sets up, warms up, times --steps steps and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned to DIR/<name>.npy (rank 0): pred_dist.npy, the answer "
                         "distribution [B, N], and node_state.npy, the final node state (a fixed sample of its rows when large)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` as the driver may call it: launch the N ranks ourselves (one process per GPU,
        # rendezvous on 127.0.0.1); rank 0 prints the one JSON line, the other ranks stay silent, the exit code is theirs
        return self_launch(args.gpus)
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d was launched with WORLD_SIZE=%d" % (args.gpus, world))
    if args.dry_run_cpu:
        return dry_run_cpu(args, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # GNNRAG_FORCE_DIST=1 runs the RCCL path with world size 1 (single-GPU boxes: exercises init + all-gather)
    distributed = world > 1 or os.environ.get("GNNRAG_FORCE_DIST") == "1"
    if distributed:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib, install, ops, shard, stack, synth
    _lib.load()
    # the rank drives one GPU: no OpenMP team (install.limit_host_threads - spinning workers exhaust a container's CPU quota
    # and the kernel then parks the launching thread too); the CPU-baseline legs set their own thread counts later
    install.limit_host_threads()
    if args.math != "default":
        ops.set_dense_math({"fp32": ops.MATH_FP32, "bf16x3": ops.MATH_BF16X3, "mixed": ops.MATH_MIXED}[args.math])
    math_name = ops.MATH_NAMES[ops.get_dense_math()]

    cfg = synth.CONFIGS[args.workload]
    strong = args.scaling == "strong" and world > 1
    ranges = None
    if strong:
        # ONE global batch (same seed on every rank), split by facts: the rank keeps its contiguous question range
        gcfg = cfg
        gbatch = synth.make_batch(gcfg)
        gfeats = synth.make_features(gcfg)
        batch, feats, ranges = strong_shard(gbatch, gfeats, rank, world)
        cfg = batch.cfg
        global_B = gcfg.B
    else:
        # every rank owns its own questions (weak scaling): same shapes, different seed
        batch = synth.make_batch(cfg, seed=cfg.seed + 1000 * rank)
        feats = synth.make_features(cfg, seed=cfg.seed + 1000 * rank)
        global_B = cfg.B * world
    params = synth.make_layer_params(cfg)
    F = batch.F
    F_g = max(F // max(cfg.B, 1), 1)

    devin = stack.DeviceInputs(batch, feats, dev)
    layer = stack.build_layer(cfg, batch, params, dev)
    t0 = time.perf_counter()
    stack.init_reason(layer, batch, devin, devin.h0)          # uploads int32 tuple + device CSR build
    torch.cuda.synchronize()
    csr_first_ms = (time.perf_counter() - t0) * 1e3

    graph = None
    if args.launch == "graph":
        with torch.no_grad():
            layer.local_entity_emb = devin.h0
            stack.run_layers(layer, cfg, devin)                   # builds layer._stack, raises launch attributes
            graph = layer._stack
            # the module runs hidden sizes that are not a multiple of 4 zero-padded (C1 / C3: 50 -> 56): the captured
            # sequence gets the operands in that form too
            P = layer._inference_params()
            gpad = (lambda t: t if P["Dp"] == P["D"] else torch.nn.functional.pad(t, (0, P["Dp"] - P["D"])))
            g_h0 = gpad(devin.h0).contiguous()
            g_ins = [gpad(devin.ins[t]).contiguous() for t in range(cfg.T)]
            graph.capture(g_h0, devin.seed_dist, g_ins[0].clone())
        h0_slot = graph.h[cfg.L - 1]

    def step():
        if graph is not None:
            # a step starts from h0 (like the eager step): the captured sequence reads its node state from h[L-1];
            # T iterations = T replays, the instructions of iteration t written into the captured buffer first
            h0_slot.copy_(g_h0.view_as(h0_slot), non_blocking=True)
            for t in range(cfg.T):
                if cfg.T > 1:
                    graph._graph_in[1].copy_(g_ins[t], non_blocking=True)
                d = graph.replay(first=(t == 0))[2][cfg.L - 1]      # relation projections once per step (= per forward)
        else:
            layer.local_entity_emb = devin.h0
            if layer._stack is not None:
                layer._stack.new_forward()        # a step is one forward of a batch: its first iteration projects the relations
            d, _ = stack.run_layers(layer, cfg, devin)
        if distributed:
            # the all-gather of this step's distribution is enqueued behind it and waited for one step later: it
            # overlaps the next step's kernels (an evaluation loop reads batch k's result after enqueueing batch k + 1)
            fin = shard.gather_rows_async(d, global_B, ranges=ranges)
            prev, pending[0] = pending[0], fin
            d = prev() if prev is not None else d
        return d

    pending = [None]

    def drain():
        if pending[0] is not None:
            out = pending[0]()
            pending[0] = None
            return out
        return None

    # An idle chip needs ~20 steps (tens of ms of load) before its clocks - and the step time - settle (5-10 % slower
    # until then: tools/probe/spread_probe.py).  A short warm-up (the driver runs --warmup 5) would leave that ramp in the
    # timed region, so the chip is first kept busy for --clock-ramp-ms with HBM copy kernels: NOT steps, no part of the
    # workload, nothing cached - it only puts the timed steps on a chip in the state a serving process keeps it in.
    if args.clock_ramp_ms > 0:
        n = 64 * 1024 * 1024
        src = torch.empty(n, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        ga = torch.empty((65536, 208), dtype=torch.float32, device=dev).normal_()      # a dummy product for the matrix
        gw = torch.empty((208, 208), dtype=torch.float32, device=dev).normal_()        # cores' share of the power state
        t_r = time.perf_counter()
        while (time.perf_counter() - t_r) * 1e3 < args.clock_ramp_ms:
            for _ in range(4):
                ops.stream_copy(src, dst)
                ops.linear(ga, gw)
            torch.cuda.synchronize()
        del src, dst, ga, gw
    # The interpreter's cyclic collector is off from the warm-up to the end of the timed region (collected right before,
    # switched back on right after): a full collection over this process's heap - the synthetic batch, torch, numpy - is a
    # 30-40 ms host pause, and in the many-launch workloads (C1 / C3: ~45 launches and a few hundred short-lived Python
    # objects per step) one landed inside a 30-step timed region (1.48 / 1.69 ms per step in the loop against 0.34 / 0.48
    # in the 200 single-step measurements behind it, profiles/r06j_other_workloads.json; a launch-count effect of the HIP
    # runtime was ruled out: tools/probe/launch_stall_probe.py, 30 000 launches without a pause).  A serving process
    # freezes its heap the same way (install.freeze_loaded_data); steps create no reference cycles that would need it.
    import gc
    gc_was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last = step()
        last = drain() if distributed else last                  # the last step's all-gather is inside the timed region
        torch.cuda.synchronize()
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    finally:
        if gc_was:
            gc.enable()
    if args.dump_outputs and rank == 0:
        # read before anything else runs on the layer: the node state is the one the last timed step left behind
        dump_outputs(args.dump_outputs, cfg, last, graph.h[cfg.L - 1] if graph is not None else layer.local_entity_emb)
    if distributed:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    assert torch.isfinite(last).all()

    # step-time spread: `spread_steps` further steps, each bracketed by its own HIP event pair (rank 0's device time)
    spread = None
    if args.full and args.spread_steps > 0:
        # a pool of 16 event pairs, read back every 16 steps: hundreds of timing events outstanding at once made the
        # HIP runtime grow its signal pool in the middle of the loop (one 30-60 ms host stall, seen as a "step")
        pool = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(16)]
        ts, hs = [], []
        done = 0
        gc_was = gc.isenabled()
        gc.collect()
        gc.disable()             # a collection in the middle of a step is a host pause the GPU then waits out
        try:
            while done < args.spread_steps:
                n = min(16, args.spread_steps - done)
                for a, b in pool[:n]:
                    h0 = time.perf_counter()
                    a.record()
                    step()
                    b.record()
                    hs.append((time.perf_counter() - h0) * 1e3)          # host time to ENQUEUE the step
                torch.cuda.synchronize()
                ts += [a.elapsed_time(b) for a, b in pool[:n]]
                done += n
        finally:
            if gc_was:
                gc.enable()
        drain()
        ts, hs = np.array(ts), np.array(hs)
        worst = int(ts.argmax())
        spread = {"n": int(len(ts)), "p05": float(np.percentile(ts, 5)), "p50": float(np.percentile(ts, 50)),
                  "p95": float(np.percentile(ts, 95)), "max": float(ts.max()), "mean": float(ts.mean()),
                  "unit": "ms per step, device time between HIP events (rank 0)",
                  # where an outlier comes from: the host's time to enqueue the SAME step (an outlier that shows on both
                  # clocks is a host pause - interpreter, allocator, driver call - that the GPU waited out, not a slow kernel)
                  "host_enqueue_ms": {"p50": float(np.percentile(hs, 50)), "max": float(hs.max()),
                                      "at_the_slowest_device_step": float(hs[worst])},
                  "slowest_step_index": worst}

    # parity in the run itself ("same inputs both sides ... in the same run"): the results of the
    # TIMED configuration - every layer's distribution and the final node state of one more step on the same batch, which
    # must reproduce the timed loop's last result bit for bit - are kept and compared further down with the reference's
    # own ReasonGNNLayer run on the identical batch by the cpu_baseline leg
    gpu_results = {}
    want_parity = args.full and rank == 0 and world == 1 and graph is None and not args.no_cpu_baseline

    def record_results(lay):
        with torch.no_grad():
            lay.local_entity_emb = devin.h0
            if lay._stack is not None:
                lay._stack.new_forward()
            d, rec = stack.run_layers(lay, cfg, devin, record=True)
        return {"dist": rec["dist"], "h": rec["h"][-1], "last": d}

    if want_parity:
        gpu_results[math_name] = record_results(layer)
        gpu_results[math_name]["timed_loop_last_step_bit_identical"] = bool(torch.equal(gpu_results[math_name].pop("last"), last))

    # the same step in EXACT fp32 (v_mfma_f32_16x16x4_f32 everywhere; the default 'mixed' mode runs the two large
    # products as bf16x3): a second, shorter timed loop on a layer object bound to that math mode
    ms_per_step_fp32 = None
    if args.full and rank == 0 and graph is None and ops.get_dense_math() != ops.MATH_FP32 and args.fp32_steps > 0:
        old_math = ops.set_dense_math(ops.MATH_FP32)
        try:
            layer32 = stack.build_layer(cfg, batch, params, dev)
            stack.init_reason(layer32, batch, devin, devin.h0)
            with torch.no_grad():
                for _ in range(10):
                    layer32.local_entity_emb = devin.h0
                    stack.run_layers(layer32, cfg, devin)
                torch.cuda.synchronize()
                t32 = time.perf_counter()
                for _ in range(args.fp32_steps):
                    layer32.local_entity_emb = devin.h0
                    stack.run_layers(layer32, cfg, devin)
                torch.cuda.synchronize()
                ms_per_step_fp32 = (time.perf_counter() - t32) * 1e3 / args.fp32_steps
            if want_parity:
                gpu_results["fp32"] = record_results(layer32)
                gpu_results["fp32"].pop("last")
            del layer32
        finally:
            ops.set_dense_math(old_math)

    # structure-build timings AFTER the timed loops: this leg allocates and frees hundreds of device blocks (one
    # structure per question) and thousands of Python objects; run before the timed region it was followed by a one-off
    # ~45 ms pause inside the timed loop of the workloads with many launches per step (C3: 2.06 instead of 0.50 ms per step;
    # tools/c3_probe.sh) - round 6 found such pauses to be full collections of the interpreter's cyclic collector, which is
    # now off across the timed region (see above); the order is kept
    csr_build_ms = csr_cached_ms = csr_concat_ms = overlapped = None
    if args.full:
        et = batch.edge_tuple
        t0 = time.perf_counter()
        for _ in range(3):
            ops.CsrPlan(et[0], et[1], et[2], cfg.B, cfg.N, cfg.R1, dev, validate=False)
        torch.cuda.synchronize()
        csr_build_ms = (time.perf_counter() - t0) * 1e3 / 3
        csr_cached_ms, csr_concat_ms = (cached_structure_ms(batch, dev, ops)
                                        if rank == 0 and not os.environ.get("BENCH_SKIP_STRUCTURE_TIMING") else (None, None))
        # (single process only: `step` enqueues the ranks' all-gather when a process group is up - rank 0 alone must not call it)
        if rank == 0 and not distributed and graph is None and not strong and not os.environ.get("BENCH_SKIP_STRUCTURE_TIMING"):
            try:
                overlapped = build_plus_step_ms(batch, dev, step, 48)
            except Exception as e:                       # never fail the bench on the side measurement
                overlapped = {"error": repr(e)[:300]}

    ms_per_step = elapsed * 1e3 / args.steps
    typed_edges = global_B * cfg.E * cfg.L * cfg.T
    facts = (F * world if not strong else sum(int(x) for x in strong_facts(ranges, gbatch))) * cfg.L * cfg.T
    value = typed_edges / (elapsed / args.steps)

    out = {
        "metric": "kg_edges_aggregated_per_sec", "value": value, "unit": "typed-edge*layers/s",
        "n_gpus": world, "n_ranks_seen": (dist.get_world_size() if distributed else 1),
        "rccl_version": (".".join(str(x) for x in torch.cuda.nccl.version()) if distributed else None),
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "%s: synthetic Freebase-shaped subgraphs, %d nodes / %d typed edges (+%d self loops) "
                               "per question, batch %d per GPU, %d layers, hidden %d, %d instructions"
                               % (cfg.name, cfg.N, cfg.E, cfg.N, cfg.B, cfg.L, cfg.D, cfg.I),
                   "B_per_gpu": cfg.B, "N": cfg.N, "E": cfg.E, "F_per_question": F_g, "R1": cfg.R1,
                   "D": cfg.D, "I": cfg.I, "L": cfg.L, "parallelism": "question-sharded x%d" % world},
        "fact_layers_per_sec": facts / (elapsed / args.steps),
        "csr_build_ms": csr_build_ms, "csr_first_call_ms": csr_first_ms,
        # f-1: per-question id blocks resident on the GPU (data/fact_mat.DeviceFactCache), batch = device concatenation
        "csr_build_from_device_cache_ms": csr_cached_ms,
        # f-1 as SURVEY 8f words it: per-question sorted structures cached on the GPU, batch = concatenation with offsets
        # (gnnrag_csr_concat: no upload, no sort, no stream wait) - what an evaluation run pays per batch from its
        # second pass over a split on (GNNRAG_DEVICE_STRUCTURES=1)
        "csr_concat_from_structure_cache_ms": csr_concat_ms,
        "value_incl_structure_concat": (typed_edges / (elapsed / args.steps + csr_concat_ms["wall_ms_incl_device"] * 1e-3)
                                        if csr_concat_ms else None),
        # host-buffer boundary: int64 tuple -> int32 upload over PCIe + device structure build, once per batch,
        # amortised over ONE step (a ReaRev forward runs num_iter steps on the same structure); never `value`
        "value_incl_upload_and_build": (typed_edges / (elapsed / args.steps + csr_build_ms * 1e-3)
                                        if csr_build_ms is not None else None),
        # a fresh structure every step, built in line from the device fact cache WITHOUT a stream wait (the cache knows the
        # relation counts): build + step in one loop
        "structure_build_in_line": overlapped,
        "value_incl_device_cache_build": (typed_edges / (overlapped["ms_per_build_plus_step"] * 1e-3)
                                          if overlapped and "ms_per_build_plus_step" in overlapped else None),
        "dense_math": math_name,
        "pre_run": ("%.0f ms of HBM copy kernels and dummy matrix products before the warm-up steps (clock ramp of an idle chip; not steps, nothing of "
                    "the workload is computed or cached)" % args.clock_ramp_ms) if args.clock_ramp_ms > 0 else None,
        "host_collector": "the interpreter's cyclic collector is off from the warm-up to the end of the timed region (a full "
                          "collection is a 30-40 ms host pause; a serving process freezes its heap: install.freeze_loaded_data)",
        "ms_per_step_fp32": ms_per_step_fp32,      # the same step with every product in exact fp32 MFMA (rank 0, 20 steps)
        "step_ms_spread": spread,
        "launch": ("hipGraph replay of the captured L-layer sequence (+ one D2D copy of h0 per step)"
                   if graph is not None else "eager: one gnnrag_reason_stack call per step"),
    }

    if rank == 0 and args.full:
        out.update(roofline_leg(cfg, layer, devin, ops, F_g, args.steps))
        if not args.no_cpu_baseline and world == 1:     # rank 0 at N = 1 only (the other ranks would idle)
            sample_b = args.cpu_sample_b
            if sample_b is None:     # ~0.8 M facts per pass is ~10 s on the host cores: C2's whole batch, 4 questions of C5
                sample_b = max(1, min(cfg.B, int(64 * 12000 // max(F_g, 1)), 64))
            keep = {} if (want_parity and min(sample_b, cfg.B) == cfg.B and cfg.T == 1) else None
            out["cpu_baseline"] = cpu_baseline_leg(cfg, min(sample_b, cfg.B), keep)
            if keep:
                out["parity_in_run"] = parity_in_run(gpu_results, keep, cfg)
            elif want_parity:
                out["parity_in_run"] = {"skipped": "the CPU leg ran a %d-question sample, not the whole %d-question batch "
                                                   "(--cpu-sample-b %d compares all of them)" % (min(sample_b, cfg.B), cfg.B, cfg.B)}
        if args.workload == "C2" and world == 1 and not distributed and args.other_workloads and graph is None:
            torch.cuda.empty_cache()                      # the legs run in processes of their own
            out["other_workloads"] = other_workloads_leg([w for w in args.other_workloads.split(",") if w], args.math)
        if not args.no_e2e and not args.no_cpu_baseline and world == 1:
            try:
                out["e2e"] = e2e_leg()
            except Exception as e:               # the staged reference is test infrastructure: never fail the bench on it
                out["e2e"] = {"error": repr(e)[:400]}
        if not args.no_e2e and not args.no_cpu_baseline and world == 1 and args.workload == "C2":
            try:
                out["train_step"] = train_step_leg()
            except Exception as e:
                out["train_step"] = {"error": repr(e)[:400]}
    if distributed:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # RCCL writes its version banner to C stdio (flushed at exit): flush it now so the JSON line is the last one
        import ctypes
        ctypes.CDLL(None).fflush(None)
        sys.stdout.flush()
        print(json.dumps(out))
        sys.stdout.flush()
        par = out.get("parity_in_run") or {}
        if par.get("ok") is False:
            # a fast step whose results differ from the reference's is not a measurement: the line above says where
            sys.stderr.write("bench.py: parity_in_run FAILED (bar %g): %s\n" % (PARITY_BAR, json.dumps(
                {k: v for k, v in par.items() if k != "note"})))
            raise SystemExit(3)


def self_launch(n):
    """``python bench.py --gpus N`` without a launcher: run the same command line under ``torch.distributed.run``
    (one rank per GPU, ``--standalone``: the launcher's own c10d rendezvous on 127.0.0.1 picks a free port itself - no
    bind / close / reuse race).  stdout / stderr are the children's, the return code too."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # a rank drives one GPU and needs no OpenMP team: a few threads each, inside the container's CPU quota
    per_rank = max(1, min(8, _cpu_budget() // (2 * n)))
    for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        env[k] = str(min(per_rank, int(env[k])) if env.get(k, "").isdigit() else per_rank)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           "--nproc-per-node", str(n), os.path.abspath(__file__)] + sys.argv[1:]
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        raise SystemExit(rc)


def other_workloads_leg(names, math):
    """The other BASELINE shapes (C3: WebQSP-dev-shaped batch of 32, D = 50, 3 x 3 layer calls; C4: CWQ-shaped, 4 layers;
    C5: the per-GPU share of the Freebase-scale config) in the driver-run line: each in a process of its own (a fresh HIP
    runtime and allocator; C5 alone holds ~10 GB) running THIS file with --workload W - 20 timed steps after a 200 ms
    clock ramp (the chip is warm from the main run) and 10 warm-up steps, the same roofline leg as the main run, no CPU
    baseline, no spread loop, no structure timings.  What is kept of each line: ms_per_step, value, and the walk's
    roofline (kernel, frac, avg launch, PMC traffic when profiles/pmc_traffic_<W>.json matches the kernel sources)."""
    import subprocess
    out = {}
    for w in names:
        cmd = [sys.executable, os.path.abspath(__file__), "--full", "--workload", w, "--steps", "20", "--warmup", "10",
               "--no-cpu-baseline", "--no-e2e", "--spread-steps", "0", "--fp32-steps", "0", "--clock-ramp-ms", "200",
               "--other-workloads", "", "--math", math]
        t0 = time.perf_counter()
        try:
            r = subprocess.run(cmd, env=dict(os.environ, BENCH_SKIP_STRUCTURE_TIMING="1"), capture_output=True, text=True,
                               timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                out[w] = {"error": (r.stdout + r.stderr)[-400:]}
                continue
            d = json.loads(line[-1])
        except Exception as e:                       # a side leg never fails the main line
            out[w] = {"error": repr(e)[:300]}
            continue
        rf = d.get("roofline") or {}
        out[w] = {"ms_per_step": d["ms_per_step"], "value": d["value"], "unit": d["unit"], "steps": d["steps"],
                  "layer_calls_per_step": d["config"]["L"] * synth_T(w), "config": d["config"]["workload"],
                  "path": d.get("path"), "dense_math": d.get("dense_math"),
                  "roofline": {k: rf.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic",
                                                      "avg_launch_ms", "algorithmic_bytes_per_launch", "real_traffic_frac",
                                                      "frac_incl_tables", "traffic_source")},
                  "kernel_ms": d.get("kernel_ms"), "process_wall_s": time.perf_counter() - t0}
    return out


def synth_T(name):
    from gnnrag_amd import synth
    return synth.CONFIGS[name].T


DUMP_STATE_ROWS = 16384      # node-state rows kept by --dump-outputs: 16384 x D=200 fp32 = 13 MB (C2's whole state is 102 MB)


def dump_outputs(out_dir, cfg, pred_dist, node_state):
    """--dump-outputs: what the last timed step handed its caller, as float32 .npy files - the answer distribution of the
    last layer call (``pred_dist.npy``, [B, N], whole) and the node state that call left in the layer
    (``node_state.npy``): all B x N rows of D (zero padding of the hidden size cut off) when they fit
    DUMP_STATE_ROWS, otherwise a fixed seeded sample of them in ascending order, whose flat row indices go to
    ``node_state_rows.npy``.  The inputs are seeded: the same arguments give the same files on every build."""
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    d = pred_dist.detach().float().cpu().numpy()
    np.save(os.path.join(out_dir, "pred_dist.npy"), d)
    h = node_state.detach().reshape(cfg.B, cfg.N, -1)[..., :cfg.D].reshape(-1, cfg.D)      # (this rank's questions)
    if h.shape[0] > DUMP_STATE_ROWS:
        rows = np.sort(np.random.default_rng(0).choice(h.shape[0], DUMP_STATE_ROWS, replace=False))
        np.save(os.path.join(out_dir, "node_state_rows.npy"), rows.astype(np.float64))
        h = h[torch.from_numpy(rows).to(h.device)]
    np.save(os.path.join(out_dir, "node_state.npy"), h.float().cpu().numpy())


def cached_structure_ms(batch, dev, ops):
    """Batch tuple + structure from per-question [3, F_g] int32 blocks that already live on the GPU
    (``gnnrag_amd.data.fact_mat.DeviceFactCache`` - what an evaluation run sees from its second epoch / second pass
    on): device concatenation + node offsets + the device structure build, wall clock per batch."""
    import torch
    from gnnrag_amd.data import fact_mat
    cfg = batch.cfg
    et = batch.edge_tuple
    bid = np.asarray(et[3])
    bounds = np.searchsorted(bid, np.arange(cfg.B + 1))

    class _Loader:                                  # the three loader fields the cache reads (dataset_load.py:452-527)
        max_local_entity, data_eff, use_self_loop, num_kb_relation = cfg.N, False, False, cfg.R1
        kb_adj_mats = [tuple((np.asarray(et[k][bounds[b]:bounds[b + 1]]) - (b * cfg.N if k != 1 else 0)) for k in range(3))
                       for b in range(cfg.B)]
        global2local_entity_maps = [()] * cfg.B

    fc = fact_mat.DeviceFactCache(_Loader(), dev)
    ids = list(range(cfg.B))
    fc.batch(ids)                                   # first use uploads the blocks
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        bf = fc.batch(ids)
        ops.CsrPlan(bf[0], bf[1], bf[2], cfg.B, cfg.N, cfg.R1, dev, validate=False, hrt_device=bf.hrt_device,
                    rel_counts=bf.rel_counts)
    cached_host_ms = (time.perf_counter() - t0) * 1e3 / 3   # the call no longer waits for its stream: host time to enqueue
    torch.cuda.synchronize()
    cached_ms = (time.perf_counter() - t0) * 1e3 / 3
    # per-question sorted STRUCTURES on the GPU, batch = concatenation with offsets (gnnrag_csr_concat)
    sc = fact_mat.DeviceStructureCache(_Loader(), dev)
    sc.loader.num_kb_relation = cfg.R1 - 1
    sc.batch(ids)                                   # first use sorts every question once
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        bf = sc.batch(ids)
        ops.CsrPlan.concat(bf.plans, cfg.N, cfg.R1, dev)
    host_ms = (time.perf_counter() - t0) * 1e3 / 5      # the call does not wait for the stream: host time to enqueue
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / 5
    return {"host_enqueue_ms": cached_host_ms, "wall_ms_incl_device": cached_ms}, {"host_enqueue_ms": host_ms, "wall_ms_incl_device": wall_ms}


def build_plus_step_ms(batch, dev, step, steps):
    """A fresh structure for EVERY step, built in line from the device-resident fact cache (what an evaluation run's first
    pass over a split pays per batch): the cache knows each question's relation count, so the build is told the counts and
    only ENQUEUES its kernels (gnnrag_csr_build_counts: no wait for the stream) - the host runs ahead of the GPU and the
    build's kernels queue behind the previous step's.  Wall clock per (build + step) pair."""
    import torch
    from gnnrag_amd.data import fact_mat
    from gnnrag_amd.modules.kg_reasoning.base_gnn import plan_for
    cfg = batch.cfg
    et = batch.edge_tuple
    bid = np.asarray(et[3])
    bounds = np.searchsorted(bid, np.arange(cfg.B + 1))
    reps = 8                                           # the loader walks `reps` batches of the same questions

    class _Loader:
        max_local_entity, data_eff, use_self_loop, num_kb_relation = cfg.N, False, False, cfg.R1 - 1
        kb_adj_mats = [tuple((np.asarray(et[k][bounds[b]:bounds[b + 1]]) - (b * cfg.N if k != 1 else 0)) for k in range(3))
                       for b in range(cfg.B)] * reps
        global2local_entity_maps = [()] * (cfg.B * reps)
        num_data = cfg.B * reps
        batches = np.arange(cfg.B * reps)

    ld = _Loader()
    fact_mat.patch_loader(ld, cache=True, device=dev)
    for r in range(reps):                              # first use uploads the questions' blocks
        ld._build_fact_mat(np.arange(r * cfg.B, (r + 1) * cfg.B), 0.0)
    torch.cuda.synchronize()
    n = 0
    t0 = time.perf_counter()
    for _ in range(max(1, steps // reps)):
        for r in range(reps):
            bf = ld._build_fact_mat(np.arange(r * cfg.B, (r + 1) * cfg.B), 0.0)
            plan_for(bf, cfg.B, cfg.N, cfg.R1, dev)
            step()
            n += 1
    torch.cuda.synchronize()
    return {"ms_per_build_plus_step": (time.perf_counter() - t0) * 1e3 / n,
            "note": "device-resident fact cache; every iteration builds a fresh structure in line; the build is told the "
                    "relation counts (gnnrag_csr_build_counts) and does not wait for its stream"}


def strong_shard(gbatch, gfeats, rank, world):
    """This rank's contiguous question range of ONE global batch, balanced by facts (shard.shard_ranges)."""
    from gnnrag_amd import shard, synth
    cfg = gbatch.cfg
    ref = (gbatch.local_entity, gbatch.query_entities, gbatch.edge_tuple, np.zeros((cfg.B, 1)), gbatch.seed_dist, None,
           np.zeros((cfg.B, cfg.N)))
    ranges = shard.shard_ranges(ref, world, "facts")
    lo, hi = ranges[rank]
    sb = shard.shard_batch(ref, rank, world, "facts")
    sub = synth.Batch(cfg=synth.GraphConfig(**{**cfg.__dict__, "B": hi - lo}), local_entity=sb[0], query_entities=sb[1],
                      seed_dist=sb[4], edge_tuple=sb[2], num_entity=gbatch.num_entity, n_real=gbatch.n_real[lo:hi])
    feats = dict(gfeats)
    feats["h0"] = gfeats["h0"][lo:hi]
    feats["ins"] = gfeats["ins"][:, lo:hi]
    return sub, feats, ranges


def strong_facts(ranges, gbatch):
    from gnnrag_amd import shard
    f = shard.facts_per_question(gbatch.edge_tuple, gbatch.cfg.B)
    return [f[lo:hi].sum() for lo, hi in ranges]


def dry_run_cpu(args, world, rank):
    """CI skeleton (tests/test_shard_gloo.py): everything of the multi-rank path that is not a kernel - rendezvous,
    sharding, the all-gather of the scored nodes, barrier-bracketed timing with the MAX over ranks, one JSON line -
    on CPU over gloo with a tiny workload and the CPU restatement as the per-rank step."""
    import torch.distributed as dist
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import shard, synth
    import oracle.rearev_torch_cpu as otorch
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    if os.environ.get("GNNRAG_DRYRUN_FAIL") == "1" and rank == world - 1:      # CI: a rank that dies fails the launcher
        raise SystemExit(7)
    gcfg = synth.GraphConfig(name="dry", B=6, N=24, E=60, R=5, D=16, I=2, L=2, T=1, seed=9, n_real_min=3)
    gbatch, gfeats = synth.make_batch(gcfg), synth.make_features(gcfg)
    params = synth.make_layer_params(gcfg)
    strong = args.scaling == "strong" and world > 1
    if strong:
        batch, feats, ranges = strong_shard(gbatch, gfeats, rank, world)
        global_B = gcfg.B
    else:
        batch, feats, ranges, global_B = gbatch, gfeats, None, gcfg.B * world

    def step():
        d = torch.from_numpy(otorch.run_stack(batch, feats, params)["dist"][-1])
        return shard.gather_rows(d, global_B, ranges=ranges) if world > 1 else d

    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    ok = None
    if strong:
        full = otorch.run_stack(gbatch, gfeats, params)["dist"][-1]
        ok = bool(np.array_equal(last.numpy(), full))
    out = {"metric": "kg_edges_aggregated_per_sec", "value": global_B * gcfg.E * gcfg.L / (elapsed / args.steps),
           "unit": "typed-edge*layers/s", "n_gpus": world,
           "n_ranks_seen": (dist.get_world_size() if world > 1 else 1), "collective_backend": "gloo",
           "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": elapsed * 1e3 / args.steps, "higher_is_better": True,
           "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "dry run on CPU (gloo): NOT a measurement"}, "gathered_matches_unsharded": ok}
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out))


def kernel_sources_digest():
    """sha256 over the CODE of the aggregation path's HIP sources (what profiles/pmc_traffic.json is valid for):
    comments and whitespace do not count, so that editing a comment does not declare a measurement stale."""
    import hashlib
    import re
    h = hashlib.sha256()
    for f in ("aggregate.hip", "csr_plan.hip", "frontier.hip", "gnnrag_common.h"):
        with open(os.path.join(REPO, "gnn-rag_amd", "csrc", f), "r") as fh:
            src = fh.read()
        src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
        src = re.sub(r"//[^\n]*", " ", src)
        h.update(" ".join(src.split()).encode())
    return h.hexdigest()


def _events_ms(fn, reps):
    """Average device time of fn() over reps launches, HIP events on torch's current stream
    (the stream the library launches on)."""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def _lib_frontier_ok(plan, D):
    import ctypes as C
    from gnnrag_amd import _lib
    return bool(_lib.load().gnnrag_frontier_supported(C.byref(plan.c), int(D)))


def roofline_leg(cfg, layer, devin, ops, F_g, steps):
    """Per-kernel device times with HIP events (torch.cuda.Event on the stream the library
    launches on), op by op, same kernels and arguments as the one-call gnnrag_reason_layer:
      * the sparse aggregation against the HBM roofline with the pinned algorithmic byte count
         - for the kernel the timed steps actually use (fused walk when the
        library picks the fused path) and for the unfused walk the formula literally describes;
      * the dense projections against the fp32 MFMA roofline.
    A step runs 1 layer call with the sparse seed prior + (L-1) with dense priors; averages use
    that mix, the dense-only numbers are reported next to them."""
    B, N, D, I, L = cfg.B, cfg.N, cfg.D, cfg.I, cfg.L
    plan = layer.plan
    reps = max(5, min(steps, 20))
    with torch.no_grad():
        layer.local_entity_emb = devin.h0
        dense, _ = layer(devin.seed_dist, devin.ins[0], step=0)      # a realistic dense prior
        P = layer._inference_params()
    seed = devin.seed_dist
    # the operands as the module hands them to the kernels: hidden sizes that are not a multiple of 4 (D = 50 of the
    # released checkpoints) are zero-padded to the next multiple of 8 inside the module (byte / flop counts below keep
    # the NOMINAL D: padding is this implementation's business)
    Dk = P["Dp"]
    padc = (lambda t: t if Dk == D else torch.nn.functional.pad(t, (0, Dk - D)).contiguous())
    h = padc(devin.h0.reshape(B * N, D))
    W_rel, b_rel, W_e2e, b_e2e = P["layers"][1][:4]

    class _Lin:                                  # parameter views in the shapes the kernels get
        def __init__(self, w, b):
            self.weight, self.bias = w, b
    rl, e2e = _Lin(W_rel, b_rel), _Lin(W_e2e, b_e2e)
    sf = _Lin(P["w_score"], P["b_score"])
    ins = padc(devin.ins[0])
    relf, relf_inv = P["relfeat"], P["relfeat_inv"]
    box = {}

    stalls = {}

    def t(fn, name=None):
        fn()                                                          # warm
        ts = np.asarray(_events_ms(fn, reps))
        # the event pair brackets the host's enqueue as well: a one-off host pause inside it (the HIP runtime's ~45 ms
        # stall every few thousand launches, tools/c3_probe.sh) would pass for a 20 x slower kernel - repetitions above
        # 3 x the median are left out of the average and counted
        keep = ts[ts <= 3.0 * np.median(ts)]
        if len(keep) < len(ts):
            stalls[name or "launch_%d" % len(stalls)] = {"dropped": int(len(ts) - len(keep)), "largest_ms": float(ts.max())}
        return float(keep.mean())

    ms = {}
    # relation projections of ALL L layers and both directions: one launch per step (rel_transform.hip)
    rel_layers = [(lp[0], lp[1], None, None) for lp in P["layers"]]
    # the V-form table kernel (k_tables_vq) is what a step runs when its shapes apply and the math mode is not fp32:
    # then the projections also write its bf16 planes
    vq = (ops.get_dense_math() != ops.MATH_FP32 and Dk % 8 == 0 and 193 <= Dk <= 208 and plan.rel_total >= 1024)
    if vq:
        ms["rel_transform_all_layers"] = t(lambda: box.__setitem__("T", ops.rel_transform(relf, relf_inv, rel_layers,
                                                                                          planes=True)))
        Tall, planes = box["T"]
    else:
        ms["rel_transform_all_layers"] = t(lambda: box.__setitem__("T", ops.rel_transform(relf, relf_inv, rel_layers)))
        Tall, planes = box["T"], None
    Tf, Ti = Tall[0, 0], Tall[0, 1]
    ms["aggregate_dense"] = t(lambda: box.__setitem__("agg", ops.aggregate(plan, dense, ins, Tf, Ti)))
    ms["aggregate_seed"] = t(lambda: ops.aggregate(plan, seed, ins, Tf, Ti))
    agg = box["agg"]
    ms["update_score"] = t(lambda: box.__setitem__("hs", ops.update_score(h, agg, e2e.weight, e2e.bias, sf.weight,
                                                                          sf.bias, layer.local_entity_mask, I)))
    del agg
    box.pop("agg")
    if vq:
        e2e0 = P["layers"][0][2]
        ms["relation_tables"] = t(lambda: box.__setitem__("P", ops.relation_tables_planes(plan, planes[0], ins, e2e0)))
        ms["relation_tables_without_planes"] = t(lambda: ops.relation_tables(plan, Tf, Ti, ins, e2e0))
    else:
        ms["relation_tables"] = t(lambda: box.__setitem__("P", ops.relation_tables(plan, Tf, Ti, ins, e2e.weight)))
    P = box["P"]
    ms["aggregate_fused_dense"] = t(lambda: box.__setitem__("nbr", ops.aggregate_fused(plan, dense, P)), "aggregate_fused_dense")
    ms["aggregate_fused_seed"] = t(lambda: ops.aggregate_fused(plan, seed, P))
    # the seed-prior launch as the timed steps run it (layer 0 of every iteration): frontier of the prior, the table
    # rows and neighbour sums of the frontier only (csrc/frontier.hip)
    seed_form_ms = None
    if getattr(layer, "seed_prior", False) and _lib_frontier_ok(plan, Dk):
        ms["frontier_build"] = t(lambda: box.__setitem__("fr", ops.Frontier(plan, seed)))
        fr = box["fr"]
        e2e_0 = layer._inference_params()["layers"][0][2]
        ms["relation_tables_frontier"] = t(lambda: box.__setitem__("Pf", fr.relation_tables(Tf, Ti, ins, e2e_0, P=box.get("Pf"))))
        nbr_f = torch.zeros((B * N, Dk), dtype=torch.float32, device=h.device)
        ms["aggregate_fused_frontier"] = t(lambda: fr.aggregate(box["Pf"], out=nbr_f))
        seed_form_ms = ms["frontier_build"] + ms["relation_tables_frontier"] + ms["aggregate_fused_frontier"]
        del nbr_f
        box.pop("Pf")
        box.pop("fr")
    nbr = box["nbr"]
    ms["update_score_fused"] = t(lambda: ops.update_score_fused(h, nbr, e2e.weight, e2e.bias, sf.weight, sf.bias,
                                                                layer.local_entity_mask, I))
    score = box["hs"][1]
    ms["softmax"] = t(lambda: ops.masked_softmax(score, B, N))

    # achievable streaming ceiling on this box (float4 copy: reads + writes)
    n = 256 * 1024 * 1024 // 4
    src = torch.empty(n, dtype=torch.float32, device=devin.h0.device).normal_()
    dst = torch.empty_like(src)
    ops.stream_copy(src, dst)
    tc = _events_ms(lambda: ops.stream_copy(src, dst), 10)
    copy_gbps = 2 * n * 4 / (np.median(tc) * 1e-3) / 1e9

    fused = layer.path == 2 or (layer.path == 0 and 2.0 * plan.rel_total * I * Dk * Dk + B * N * Dk * Dk
                                < 0.8 * B * N * (2 * I + 1) * Dk * Dk)
    ba = bytes_agg(cfg, F_g)

    def hbm(kernel, dense_ms, seed_ms, extra=None, seed_form=None):
        # `achieved` / `frac`: the NAMED kernel on the launches it really runs in a step.  Since round 3 the fused path's
        # seed-prior launch (layer 0 of every iteration) is a different, much shorter kernel sequence (frontier form), so
        # the LDS walk only runs the L - 1 dense-prior launches: its figure is the dense-prior one.  The mix over all L
        # aggregation launches of an iteration (same pinned byte count per launch) is reported next to it.
        avg = dense_ms if seed_form is not None else (seed_ms + (L - 1) * dense_ms) / L
        ach = ba / (avg * 1e-3) / 1e9
        mix = ((seed_form if seed_form is not None else seed_ms) + (L - 1) * dense_ms) / L
        o = {"kernel": kernel, "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
             "frac": ach / HBM_PEAK_GBPS, "traffic": None, "algorithmic_bytes_per_launch": ba,
             "avg_launch_ms": avg, "launches_timed": reps if seed_form is not None else 2 * reps,
             "dense_prior": {"avg_launch_ms": dense_ms, "achieved": ba / (dense_ms * 1e-3) / 1e9,
                             "frac": ba / (dense_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS},
             "seed_prior": {"avg_launch_ms": seed_ms, "note": "the same kernel on the seed prior (not what a step runs "
                                                              "when the frontier form applies)"},
             "all_aggregation_launches_of_an_iteration": {
                 "avg_launch_ms": mix, "equivalent_work_frac": ba / (mix * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                 "note": "1 seed-prior launch + (L-1) dense-prior launches, each priced at the pinned byte count"},
             "measured_copy_ceiling_GBps": copy_gbps}
        if seed_form is not None:
            o["seed_prior_frontier_form"] = {
                "kernels": "k_frontier_build + k_tables_frontier + k_walk_frontier (csrc/frontier.hip)",
                "avg_ms": seed_form, "replaces_ms": seed_ms + ms["relation_tables"],
                "note": "layer 0 of every iteration: frontier of the seed prior, relation-table rows and neighbour sums of "
                        "the frontier only; replaces the full table launch + the walk on the seed prior"}
        if extra:
            o.update(extra)
        o["traffic_source"] = pmc_note
        if o.get("traffic"):
            # what the memory system really moved per launch (the fused walk never writes agg): the honest HBM rate
            o["real_traffic_GBps"] = o["traffic"] / (avg * 1e-3) / 1e9
            o["real_traffic_frac"] = o["real_traffic_GBps"] / HBM_PEAK_GBPS
            o["real_traffic_frac_of_copy_ceiling"] = o["real_traffic_GBps"] / copy_gbps
        return o

    # HBM traffic of the aggregation kernels comes from rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE cannot be read
    # from inside the process); tools/refresh_profiles.sh stores them in profiles/pmc_traffic.json together with the
    # digest of the kernel sources they were measured on.  A figure measured on OTHER sources is not reported.
    pmc, pmc_note = {}, "profiles/pmc_traffic.json absent"
    ppath = os.path.join(REPO, "profiles", "pmc_traffic_%s.json" % cfg.name)      # one file per workload, else the default
    if not os.path.exists(ppath):
        ppath = os.path.join(REPO, "profiles", "pmc_traffic.json")
    if os.path.exists(ppath):
        try:
            pmc = json.load(open(ppath))
            cur = kernel_sources_digest()
            if pmc.get("workload", "C2") != cfg.name:
                pmc, pmc_note = {}, "pmc_traffic.json was measured on workload %s" % pmc.get("workload", "C2")
            elif pmc.get("kernel_sources_sha256") != cur:
                pmc_note = ("STALE: measured on kernel sources %s, current %s - not reported"
                            % (str(pmc.get("kernel_sources_sha256"))[:12], cur[:12]))
                pmc = {}
            else:
                pmc_note = "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (x2 FETCH correction), commit %s, same kernel sources" % pmc.get("commit", "?")
        except Exception as e:
            pmc, pmc_note = {}, "unreadable: %r" % (e,)
    r_fused = hbm("gnnrag_aggregate_fused: " + ops.WALK_KERNEL_NAMES[ops.aggregate_fused_variant(plan, Dk)] +
                  ("" if Dk == D else " [hidden size %d zero-padded to %d]" % (D, Dk)), ms["aggregate_fused_dense"],
                  ms["aggregate_fused_seed"], seed_form=seed_form_ms, extra=
                  {"note": "fused walk: e2e_linear is pushed into per-question relation tables, so agg [BN,2I*D] is "
                           "never written; `achieved` still uses the pinned unfused byte count (SURVEY 8d), i.e. it "
                           "is an equivalent-work rate and may exceed what an unfused kernel can reach; real HBM "
                           "traffic is in `traffic`",
                   "traffic": pmc.get("aggregate_fused_hbm_bytes_per_launch")})
    r_unf = hbm("gnnrag_aggregate (k_walk_light<REASON> + heavy chunks)", ms["aggregate_dense"], ms["aggregate_seed"],
                {"note": "the unfused walk the byte formula literally describes (writes agg [BN,2I*D])",
                 "traffic": pmc.get("aggregate_hbm_bytes_per_launch")})

    b3_mode = ops.get_dense_math() != ops.MATH_FP32

    def mfma(kernel, flops, t_ms, b3=False):
        # a bf16x3 kernel runs on the bf16 pipe (6 plane products per fp32-equivalent one): its peak in fp32-equivalent
        # flops is 2500 / 6 = 417 TFLOP/s; `frac` is against the pipe the kernel really uses, the fraction of the fp32
        # pipe's peak (a pipe it does not use; can exceed what an exact-fp32 kernel could reach) is kept beside it
        ach = flops / (t_ms * 1e-3) / 1e12
        peak = BF16_MFMA_PEAK_TFLOPS / 6.0 if b3 else FP32_MFMA_PEAK_TFLOPS
        o = {"kernel": kernel, "bound": "mfma", "achieved": ach, "peak": peak,
             "unit": "TFLOP/s (fp32-equivalent)", "frac": ach / peak, "avg_launch_ms": t_ms,
             "flops_per_launch": flops, "pipe": "bf16 MFMA, 6 plane products per product (peak 2500 / 6)" if b3 else
             "fp32 MFMA"}
        if b3:
            o["bf16_flops_per_launch"] = 6.0 * flops
            o["achieved_bf16_TFLOPs"] = 6.0 * ach
            o["frac_of_fp32_mfma_peak"] = ach / FP32_MFMA_PEAK_TFLOPS
        return o

    # the relation-table launch exists only because e2e_linear was pushed into per-question
    # tables - charge it to the aggregation next to `frac`
    if fused and "relation_tables" in ms:
        t_all = ms["aggregate_fused_dense"] + ms["relation_tables"]
        r_fused["frac_incl_tables"] = ba / (t_all * 1e-3) / 1e9 / HBM_PEAK_GBPS
        r_fused["frac_incl_tables_note"] = ("pinned algorithmic bytes / (dense-prior walk %.1f us + relation-table launch %.1f us)"
                                            % (ms["aggregate_fused_dense"] * 1e3, ms["relation_tables"] * 1e3))
        r_fused["guide_copy_ceiling_GBps"] = 6290.0          # MI355X_MICROARCH.md: float4 copy, 79 % of 8 TB/s
    out = {
        "path": "fused" if fused else "unfused",
        "roofline": r_fused if fused else r_unf,
        "roofline_aggregate_unfused" if fused else "roofline_aggregate_fused": r_unf if fused else r_fused,
        "roofline_dense": {
            # flops are the fp32-equivalent ones of the reference's products ([2*rel_total, I*D]x[I*D, D] for the
            # tables whichever form computes them); the bf16x3 kernels issue 6 bf16 MFMAs per fp32-equivalent one, so
            # `frac` of the fp32 peak can exceed what an exact-fp32 kernel could reach
            "update_score": mfma("gnnrag_update_score [BN,(2I+1)D]x[(2I+1)D,D] (k_gemm_f32, k-tiled)", flops_update(cfg),
                                 ms["update_score"], b3=b3_mode),
            "relation_tables": mfma("gnnrag_relation_tables%s [2*rel_total, I*D]x[I*D, D] (%s)"
                                    % ("_planes" if vq else "", "k_tables_vq, bf16x3 V form" if vq else
                                       "k_tables_b3 / k_gemm_f32 generated-A"),
                                    2.0 * 2 * plan.rel_total * I * D * D, ms["relation_tables"], b3=b3_mode),
            "update_score_fused": mfma("gnnrag_update_score_fused [BN,D]x[D,D] + nbr (%s)"
                                       % ("k_gemm_wres, exact fp32" if ops.get_dense_math() == ops.MATH_FP32
                                          else "k_update_b3, bf16x3, where its shapes apply"),
                                       2.0 * B * N * D * D, ms["update_score_fused"],
                                       b3=b3_mode and 193 <= Dk <= 208 and B * N >= 8192),
        },
        "kernel_ms": ms,
        "kernel_ms_host_stalls_left_out": stalls or None,
    }
    # the self-block update streams h, nbr and h' (3 x BN x D x 4 B): it sits nearer its HBM roof than its MFMA roof -
    # both fractions are reported
    upd = out["roofline_dense"]["update_score_fused"]
    upd_bytes = 3.0 * B * N * D * 4 + B * N * 8 + D * D * 4
    upd["hbm"] = {"algorithmic_bytes_per_launch": upd_bytes,
                  "achieved_GBps": upd_bytes / (ms["update_score_fused"] * 1e-3) / 1e9,
                  "frac": upd_bytes / (ms["update_score_fused"] * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                  "traffic": pmc.get("update_score_fused_hbm_bytes_per_launch"),
                  "note": "h read + nbr read + h' write; `frac` of 8 TB/s"}
    upd["frac_mfma"] = upd["frac"]
    upd["frac_hbm"] = upd["hbm"]["frac"]
    return out


def e2e_leg():
    """End to end through the reference's OWN entry point (SURVEY 8d "for C1 use the real entry"):
    the unmodified ``gnn/main.py --is_eval`` (staged by oracle/stage_ref.py into the git-ignored oracle/_ref/, which travels
    to the GPU box) on the staged synthetic dataset, driven by tools/run_reference.py -
      * on the MI355X with this package's modules underneath (all 160 dev + 520 test questions), with the per-stage split
        get_batch / structure build / forward / Evaluator tail (device-synchronised timers at the reference's seams);
      * the PURE reference on the host cores (GNNRAG_PURE_REFERENCE=1, no substitution) on a bounded sample: the first 32
        test questions (data/synth_sample), same checkpoint, same flags;
      * BASELINE config 1 as SURVEY 8d words it: ``Evaluator.evaluate`` with ``test_batch_size=1`` and the
        released-checkpoint dims (variant d50), GPU on the full splits, CPU on the sample.
    Questions/s = questions of the TEST split / wall time of its ``Evaluator.evaluate`` call (get_batch, forward,
    candidate selection, metrics, .info writing - everything the reference does per batch; model construction, checkpoint
    and dataset loading are not in it)."""
    import shutil
    import subprocess
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import stage_ref
    if not stage_ref.staged():
        return {"skipped": "oracle/_ref not staged (python oracle/stage_ref.py in the build container)"}
    from gnnrag_amd.install import host_cpu_budget
    ncpu = os.cpu_count() or 1
    # the CPU leg gets the cores the container may really use (cgroup CFS quota): more OpenMP threads than that are parked
    # by the kernel for the rest of every 100 ms period and the baseline would be slower than the reference can be here
    cpu_threads = min(32, ncpu, host_cpu_budget())

    def run(variant, pure, batch, data=None, extra_env=None):
        argv = list(stage_ref.variant_argv(variant))
        if data:                                       # the variant's bounded sample (first 32 test questions)
            argv = [stage_ref.sample_folder(variant) if a == stage_ref.data_folder(variant) else a for a in argv]
        i = argv.index("--test_batch_size")
        argv[i + 1] = str(batch)
        ck = tempfile.mkdtemp(prefix="gnnrag_e2e_") + "/"
        shutil.copyfile(os.path.join(stage_ref.CKPT, stage_ref.ckpt_name(variant)), ck + stage_ref.ckpt_name(variant))
        cmd = [sys.executable, os.path.join(REPO, "tools", "run_reference.py"), stage_ref.GNN] + argv + [
            "--is_eval", "--load_experiment", stage_ref.ckpt_name(variant), "--checkpoint_dir", ck, "--experiment_name", "e2e"]
        env = dict(os.environ, GNNRAG_E2E_TIMES="1")
        if pure:
            env.update(GNNRAG_PURE_REFERENCE="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS=str(cpu_threads),
                       MKL_NUM_THREADS=str(cpu_threads))
        else:
            env.update(GNNRAG_DEVICE_FACTS="1")
        env.update(extra_env or {})
        t0 = time.perf_counter()
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        shutil.rmtree(ck, ignore_errors=True)
        log = r.stdout + r.stderr
        line = [l for l in log.splitlines() if l.startswith("GNNRAG_E2E ")]
        if r.returncode != 0 or not line:
            return {"error": log[-600:]}
        T = json.loads(line[-1][len("GNNRAG_E2E "):])
        test = T["evaluate_calls"][-1]                    # evaluate_single: valid split first, test split last
        import re
        h1 = re.findall(r"TEST F1: ([0-9.]+), H1: ([0-9.]+)", log)
        nb = max(test["batches"], 1)
        fwd = test["forward_s"] - test["structure_s"]
        tail = test["seconds"] - test["get_batch_s"] - test["forward_s"]
        return {"questions": test["questions"], "seconds": test["seconds"], "questions_per_s": test["questions"] / test["seconds"],
                "test_batch_size": batch, "batches": test["batches"], "padded_nodes_per_question": test["max_local_entity"],
                "stages_ms_per_batch": {"get_batch": 1e3 * test["get_batch_s"] / nb, "structure_build": 1e3 * test["structure_s"] / nb,
                                        "forward_without_structure": 1e3 * fwd / nb, "evaluator_tail": 1e3 * tail / nb},
                "test_f1_h1": [float(x) for x in h1[-1]] if h1 else None, "process_wall_s": wall,
                "threads": T.get("threads"),
                # the tail is the reference's own per-candidate Python (metrics, json.dumps of every retrieved candidate):
                # its cost follows the number of RETRIEVED candidates.  This synthetic model is unsure about a third of its
                # questions and retrieves hundreds of near-tied candidates for them; WebQSP's released model retrieves 8.1
                # per question on average - `evaluator_tail_at_8_per_question_ms` rescales by that ratio
                "retrieved_candidates": _tail_stats(T.get("retrieved"), 1e3 * tail / nb, batch)}

    out = {"host_cpu_quota_cores": host_cpu_budget(),
           "host_threads": "GPU legs: install.limit_host_threads() (min(8, quota / 2) intra-op threads: the driving process "
                           "needs no OpenMP team, and a spinning one exhausts the CPU quota - 68-78 ms pauses of every thread, "
                           "profiles/r05i_forward_host_time.txt); CPU leg: min(32, quota) threads",
           "evaluator_tail": "the reference's own per-candidate Python (evaluate.py:188-226).  Default: it runs in a process forked "
                             "before the GPU is touched (eval_tail.start_tail_server) and a split costs max(scoring side, tail "
                             "side) per batch; the stage figure is what the scoring process still waits for",
           "entry": "unmodified gnn/main.py --is_eval via tools/run_reference.py; staged synthetic datasets (oracle/stage_ref.py: "
                    "a relation path from the seed determines the answer; 520 test questions, subgraphs up to 2000 entities; 24 "
                    "relation types for d50, 12 for d200)",
           "host_cores": ncpu}
    out["d200_batch16"] = {"gpu": run("d200", False, 16),
                           "cpu_reference_sample32": run("d200", True, 16, True)}
    # BASELINE config 2's batch (64 questions per forward): the host's per-batch costs spread over four times the questions.
    # "gpu": as tools/run_reference.py runs it - the reference's per-candidate tail in a process of its own
    # (gnnrag_amd.eval_tail.start_tail_server, forked before the GPU is touched; `evaluator_tail` is then what the scoring
    # process still waits for); "gpu_tail_in_line": GNNRAG_EVAL_PIPELINE=0, both halves in one interpreter (rounds 4-5)
    out["d200_batch64"] = {"gpu": run("d200", False, 64),
                           "gpu_tail_in_line": run("d200", False, 64, extra_env={"GNNRAG_EVAL_PIPELINE": "0"})}
    # the same checkpoint with main.py's --eps 0.3: the top-p cut retrieves ~10 candidates per question instead of ~115
    # (WebQSP's released model: 8.1) - the tail at a realistic length, measured instead of rescaled
    if stage_ref.staged_variant("d200eps"):
        out["d200_batch64_eps03"] = {"gpu": run("d200eps", False, 64),
                                     "gpu_tail_in_line": run("d200eps", False, 64, extra_env={"GNNRAG_EVAL_PIPELINE": "0"})}
    out["c1_d50_batch1"] = {"gpu": run("d50", False, 1),
                            "cpu_reference_sample32": run("d50", True, 1, True)}
    for k in ("d200_batch16", "c1_d50_batch1"):
        g, c = out[k]["gpu"], out[k]["cpu_reference_sample32"]
        if "questions_per_s" in g and "questions_per_s" in c:
            out[k]["gpu_over_cpu_questions_per_s"] = g["questions_per_s"] / c["questions_per_s"]
    return out


def train_step_leg():
    """One training step as the reference's trainer runs it (Trainer_KBQA.train_epoch, train_model.py:209-233: get_batch,
    zero_grad, model(batch, training=True), loss.backward(), clip_grad_norm_, Adam.step, loss.item()) on the staged
    dataset at hidden size 200, batch 16 - the reference's own trainer, model code and optimiser in both legs
    (tools/time_train_step.py): on the MI355X with this package's modules underneath (autograd form, HIP backward of the
    typed-edge aggregation), and the pure reference on the host cores.  Two flag sets: the reference's defaults
    (linear_dropout 0.2: the unfused autograd form, as dropout acts between aggregation and e2e_linear) and all dropouts
    off (the fused training form; there both legs see the same numbers, so the first step's losses are comparable)."""
    import subprocess
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import stage_ref
    if not stage_ref.staged():
        return {"skipped": "oracle/_ref not staged"}
    cpu_threads = min(32, os.cpu_count() or 1, _cpu_budget())

    def run(pure, extra, steps, warm):
        cmd = [sys.executable, os.path.join(REPO, "tools", "time_train_step.py"), stage_ref.GNN, "--variant", "d200",
               "--steps", str(steps), "--warm", str(warm)] + (["--pure"] if pure else []) + list(extra)
        env = dict(os.environ)
        if pure:
            env.update(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS=str(cpu_threads), MKL_NUM_THREADS=str(cpu_threads))
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        line = [l for l in (r.stdout + r.stderr).splitlines() if l.startswith("GNNRAG_TRAIN ")]
        if r.returncode != 0 or not line:
            return {"error": (r.stdout + r.stderr)[-500:]}
        return json.loads(line[-1][len("GNNRAG_TRAIN "):])

    out = {"config": "staged synthetic dataset (oracle/stage_ref.py, 12 relation types, 1200 train questions, subgraphs padded to "
                     "the split's largest), ReaRev --entity_dim 200 --num_iter 3 --num_ins 2 --num_gnn 3 --batch_size 16, Adam, "
                     "gradient clip 1.0, from the staged checkpoint; median wall per step, seams synchronised",
           "cpu_threads": cpu_threads}
    for tag, extra in (("default_flags", []), ("dropout_off", ["--linear_dropout", "0", "--lm_dropout", "0"])):
        g = run(False, extra, 20, 5)
        c = run(True, extra, 5, 1)
        o = {"gpu": g, "reference_cpu": c}
        if "ms_per_step" in g and "ms_per_step" in c:
            o["gpu_ms"], o["reference_cpu_ms"] = g["ms_per_step"], c["ms_per_step"]
            o["reference_cpu_over_gpu"] = c["ms_per_step"] / g["ms_per_step"]
            if tag == "dropout_off":
                o["loss_first_step"] = {"gpu": g["losses"][0], "reference_cpu": c["losses"][0],
                                        "abs_diff": abs(g["losses"][0] - c["losses"][0])}
        out[tag] = o
    d = out["default_flags"]
    if "gpu_ms" in d:
        out["gpu_ms"], out["reference_cpu_ms"] = d["gpu_ms"], d["reference_cpu_ms"]
    return out


def _tail_stats(st, tail_ms_per_batch, batch):
    if not st or not st.get("questions"):
        return None
    per_q = st["retrieved"] / st["questions"]              # (both splits of the run: valid + test)
    return {"per_question_mean": per_q, "largest": st["retrieved_max"],
            "tail_us_per_retrieved_candidate": 1e3 * tail_ms_per_batch / max(per_q * batch, 1e-9),
            "evaluator_tail_at_8_per_question_ms": tail_ms_per_batch * min(1.0, 8.1 / max(per_q, 1e-9))}


def reference_cpu_leg(cfg, sample_b, keep=None):
    """The REAL reference layer (`ReasonGNNLayer` from the sources staged into the git-ignored oracle/_ref/gnn by
    oracle/stage_ref.py - /root/reference itself does not exist on the GPU box) on the host cores, on a bounded sample:
    sample_b questions of the same shape, same parameters, eval mode, no_grad; `build_matrix` timed separately.
    Returns None when the staged sources are absent."""
    ref = os.path.join(REPO, "oracle", "_ref", "gnn")
    if not os.path.isfile(os.path.join(ref, "modules", "kg_reasoning", "reasongnn.py")):
        return None
    from gnnrag_amd import synth
    sys.path.insert(0, ref)
    try:
        from modules.kg_reasoning.reasongnn import ReasonGNNLayer as RefLayer
    finally:
        sys.path.remove(ref)
    sub = synth.GraphConfig(**{**cfg.__dict__, "B": sample_b, "name": cfg.name + "-cpu-sample"})
    batch, feats, params = synth.make_batch(sub), synth.make_features(sub), synth.make_layer_params(sub)
    args = dict(use_cuda=False, normalized_gnn=sub.normalized_gnn, num_ins=sub.I, num_gnn=sub.L, pos_emb=sub.pos_emb,
                linear_dropout=0.0)
    layer = RefLayer(args, batch.num_entity, sub.num_kb_relation, sub.D, "bfs")
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items() if not k.startswith("type_layer.")})
    layer.eval()
    tens = dict(local_entity=torch.from_numpy(batch.local_entity), local_entity_emb=torch.from_numpy(feats["h0"]),
                rel_features=torch.from_numpy(feats["rel_features"]), rel_features_inv=torch.from_numpy(feats["rel_features_inv"]),
                query_entities=torch.from_numpy(batch.query_entities).float())
    seed = torch.from_numpy(batch.seed_dist).float()
    ins = torch.from_numpy(feats["ins"][0])
    import warnings

    def one_pass():
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            layer.init_reason(kb_adj_mat=batch.edge_tuple, **tens)       # build_matrix (base_gnn.py:19-51)
            t1 = time.perf_counter()
            dist = seed
            dists = []
            for j in range(sub.L):
                dist, _ = layer(dist, ins, step=j)
                dists.append(dist)
            t2 = time.perf_counter()
            if keep is not None:                      # (after the clock is read) the pass's results, for parity_in_run
                keep["dist"] = [d.numpy().copy() for d in dists]
                keep["h"] = layer.local_entity_emb.numpy().copy()
            return t1 - t0, t2 - t1

    from gnnrag_amd.install import host_cpu_budget
    ncpu = os.cpu_count() or 1
    best = None
    for nt in sorted({c for c in (host_cpu_budget(), 16, 32, 64) if c <= ncpu} or {ncpu}):
        torch.set_num_threads(nt)
        _, dt = one_pass()
        if best is None or dt < best[0]:
            best = (dt, nt)
    torch.set_num_threads(best[1])
    one_pass()                                   # SURVEY 8d protocol: 1 warm-up + 5 timed passes, median
    runs = [one_pass() for _ in range(5)]
    t = float(np.median([r[1] for r in runs]))
    return {"value": sub.B * sub.E * sub.L / t, "unit": "typed-edge*layers/s", "cores": best[1], "kind": "reference",
            "sample": "%d questions of the same %s shape (N=%d, E=%d, D=%d, I=%d, L=%d) through the reference's own "
                      "ReasonGNNLayer (sources staged by oracle/stage_ref.py), torch CPU, thread count chosen by a probe, "
                      "1 warm-up + 5 timed passes, median %.2f s/pass (min %.2f, max %.2f); build_matrix %.2f s per batch on top"
                      % (sub.B, cfg.name, sub.N, sub.E, sub.D, sub.I, sub.L, t, min(r[1] for r in runs), max(r[1] for r in runs),
                         float(np.median([r[0] for r in runs]))),
            "scaling_assumption": "rate of the %d-question sample taken as the rate of the %d-question batch: questions are "
                                  "independent subgraphs and every reference op is linear in the number of facts / node "
                                  "slots (the survey's full-batch run, 11.7 s per pass on 8 vCPUs, is quoted beside it); "
                                  "--cpu-sample-b %d times the whole batch" % (sub.B, cfg.B, cfg.B),
            "seconds_per_pass": t, "build_matrix_seconds": float(np.median([r[0] for r in runs]))}


def cpu_baseline_leg(cfg, sample_b, keep=None):
    """The reference's CPU path on a bounded sample of the same workload: the REAL reference layer when its sources were
    staged (kind "reference"), with the torch-CPU restatement (oracle/rearev_torch_cpu.py, kind "port") timed beside it;
    only the port when they were not."""
    out = port_cpu_leg(cfg, sample_b)
    try:
        ref = reference_cpu_leg(cfg, sample_b, keep)
    except Exception as e:                       # the staged reference is test infrastructure: never fail the bench on it
        ref = None
        out["reference_error"] = repr(e)[:300]
    if ref is not None:
        ref["port"] = {k: out[k] for k in ("value", "cores", "seconds_per_pass", "sample")}
        ref["live_reference_survey"] = out["live_reference_survey"]
        return ref
    return out


def port_cpu_leg(cfg, sample_b):
    """The reference's CPU op sequence (oracle/rearev_torch_cpu.py, a port: /root/reference is not
    on the GPU box) on a bounded sample of the same workload: sample_b questions of the same
    shape, all host cores, 1 warm-up + 2 timed L-layer passes."""
    import oracle.rearev_torch_cpu as otorch
    from gnnrag_amd import synth
    sub = synth.GraphConfig(**{**cfg.__dict__, "B": sample_b, "name": cfg.name + "-cpu-sample"})
    batch = synth.make_batch(sub)
    feats = synth.make_features(sub)
    params = synth.make_layer_params(sub)
    ncpu = os.cpu_count() or 1
    cores = ncpu
    p = otorch.to_torch_params(params)
    relfeat = torch.from_numpy(feats["rel_features"])
    relfeat_inv = torch.from_numpy(feats["rel_features_inv"])
    ins = torch.from_numpy(feats["ins"][0])
    mask = torch.from_numpy((batch.local_entity != batch.num_entity).astype(np.float32))
    seed = torch.from_numpy(batch.seed_dist.astype(np.float32))
    t0 = time.perf_counter()
    st = otorch.Structure(batch.edge_tuple, sub.B, sub.N, sub.normalized_gnn)
    build_s = time.perf_counter() - t0

    def one_pass():
        h = torch.from_numpy(feats["h0"])
        dist = seed
        with torch.no_grad():
            for j in range(sub.L):
                _, dist, h = otorch.layer_forward(st, h, mask, dist, ins, p, j, relfeat, relfeat_inv, sub.pos_emb)
        return dist

    # torch-CPU does not scale to every core of a big host (256 threads ran 2x slower than 32 on
    # the GPU box): probe a few thread counts on one pass each and keep the fastest
    from gnnrag_amd.install import host_cpu_budget
    best = None
    for nt in sorted({c for c in (host_cpu_budget(), 16, 32, 64) if c <= ncpu} or {ncpu}):
        torch.set_num_threads(nt)
        t0 = time.perf_counter()
        one_pass()
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, nt)
    cores = best[1]
    torch.set_num_threads(cores)
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        one_pass()
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    return {"value": sub.B * sub.E * sub.L / t, "unit": "typed-edge*layers/s", "cores": cores, "kind": "port",
            "sample": "%d questions of the same %s shape (N=%d, E=%d, D=%d, I=%d, L=%d), torch-CPU restatement of "
                      "the reference op sequence, thread count chosen by a probe, 2 timed passes, median %.2f s/pass; "
                      "structure build %.2f s" % (sub.B, cfg.name, sub.N, sub.E, sub.D, sub.I, sub.L, t, build_s),
            "seconds_per_pass": t,
            # the LIVE reference on the same C2 shape, full batch (/root/reference is not on
            # the GPU box, so it cannot be re-timed here): 11.7 s per 3-layer pass on 8 vCPUs
            "live_reference_survey": {"seconds_per_pass": 11.7, "typed_edge_layers_per_sec": 1.64e5, "cores": 8,
                                      "source": "BASELINE.md section 3: reference ReasonGNNLayer, torch 2.10 CPU, "
                                                "C2 shapes (B=64), survey container"}}


if __name__ == "__main__":
    main()
