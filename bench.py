#!/usr/bin/env python3
"""Benchmark of the adversarial_learner hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W
  (N>1: one process per GPU -- either under a launcher, python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
   127.0.0.1 ... bench.py --gpus N ..., or plainly as above: without WORLD_SIZE in the environment the script starts that launcher itself)

One step = PWC-Net flow + mask-generator fwd + 3x recover fwd + generator-loss backward + recover-loss backward +
both clipped-Adam updates on 4 DAVIS-480p-shaped synthetic frame pairs per GPU (BASELINE.json configs[1]/[2]).
Inputs are resident in HBM (reader preprocessing done before the timed region).  Prints ONE JSON line.

A plain run sets up (plan, weights, kernel configurations, resident inputs), runs W warm-up and K timed steps and prints the
headline line (value, ms_per_step and the per-step distribution).  `--dump-outputs DIR` also writes what the last timed step computed
as DIR/<name>.npy (float32).  Inputs are seeded and the kernel configurations of the headline workload are the committed ones
(SHIPPED_TUNE), so every run of the same arguments computes the same outputs and two builds can be compared output for output.

`--full` adds everything else the line has carried: the CPU-oracle leg and both parity checks, the reference schedule, the
ensemble workload, the per-launch profiling pass (roofline, hbm_kernels) and, with N > 1, the gradient-exchange timings.
The GPU leg and the CPU-oracle leg (`cpu_baseline`, rank 0 at N=1) run the SAME seeded weights on the SAME frame pairs;
their first (untimed) step is compared -- `parity_check` in the JSON line -- and the process exits non-zero when the HIP path
is more than 1e-3 (north_star tolerance) away from the oracle."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ALG_GFLOP_PER_PAIR = 217.945  # 871.78 GFLOP per 4-pair step (fwd 551.06 + gen bwd 210.35 + rec bwd 110.36)
ENSEMBLE_GFLOP_PER_FRAME = 1983.5  # 16 x (PWC-Net + generator forward at batch 1)
PEAK_FP32_MFMA_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md chip table
PEAK_HBM_GBS = 8000.0
PARITY_TOL = 1e-3
DUMP_LIMIT_BYTES = 64 * 10 ** 6
# The kernel configurations the autotuner picked for this build on the headline workload (fp32, batch 4), on an MI355X.  Timing picks
# between near-equal candidates differently from run to run, and another split count or kernel family rounds differently -- which
# Adam turns into step-sized weight differences within a few steps.  Loaded before the autotune pass (which then times only the
# shapes the file lacks: other batch sizes, fp16 convolutions), they make every run of the same arguments compute the same outputs.
SHIPPED_TUNE = os.path.join(ROOT, "profiles", "r06_tune.txt")


def cpu_baseline(weights, i1, i2, gpu_first, reps: int, threads: int = 0, tol: float = None):
    """The oracle (PyTorch-CPU restatement, oracle/oracle_torch.py) on the host cores, on the weights / frame pairs of the
    GPU leg.  Step 0 is untimed and is the parity check: oracle PWC flow vs the HIP flow, then generator / recover / losses on
    the HIP flow vs the HIP results (`gpu_first`).  Steps 1..reps are timed full adversarial steps (fwd + both backward +
    clipped Adam) -- a bounded sample of the workload."""
    from oracle import oracle_torch as O
    batch = i1.shape[0]
    # measured on the MI355X host (256 logical CPUs), B=1: 16 threads 2.36 pairs/s, 32 -> 1.47, 64 -> 0.59: use 16
    cores = threads or min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)
    pp, pg, pr = ({k: v.clone() for k, v in d.items()} for d in weights)

    class C(O.Flags):
        batch_size = batch
    opt = O.TFAdam()
    times = []
    parity = None
    for r in range(reps + 1):
        for d in (pg, pr):
            for k in d:
                d[k] = d[k].detach().requires_grad_(True)
        t0 = time.time()
        with torch.no_grad():
            image, flow, _ = O.prepare_inputs(pp, i1, i2, C)
        if r == 0:
            gflow = gpu_first["flow"]
            rel = lambda a, b: float((a - b).abs().max()) / max(1e-6, float(b.abs().max()))
            parity = {"flow_rel_err": rel(gflow, flow), "image_max_abs_err": float((gpu_first["image"] - image).abs().max())}
            out = O.forward_from_flow(pg, pr, image, gflow, C)  # the HIP flow: PWC rounding must not leak into what follows
            parity["mask_max_abs_err"] = float((gpu_first["mask"] - out["mask"]).abs().max())
            ref_pred = torch.cat([out["pred"], out["pred_c"], out["pred_img"]], 0)
            parity["pred_rel_err"] = rel(gpu_first["pred"], ref_pred.detach())
            parity["max_rel_loss_err"] = max(abs(gpu_first["losses"][k] - float(out[k])) / max(1.0, abs(float(out[k])))
                                             for k in gpu_first["losses"])
            parity["losses_oracle"] = {k: round(float(out[k]), 6) for k in ("generator", "recover")}
            parity["losses_hip"] = {k: round(gpu_first["losses"][k], 6) for k in ("generator", "recover")}
            parity["tolerance"] = tol or PARITY_TOL
            parity["ok"] = all(parity[k] <= (tol or PARITY_TOL) for k in ("flow_rel_err", "mask_max_abs_err", "pred_rel_err", "max_rel_loss_err"))
        else:
            out = O.forward_from_flow(pg, pr, image, flow, C)
        gg = O.grads_of(out["generator"], pg)
        gr = O.grads_of(out["recover"], pr)
        with torch.no_grad():
            cg, _ = O.clip_or_noise(gg, 0.2, True, lambda k, s: torch.rand(s) * 0.4 - 0.2)
            cr, _ = O.clip_or_noise(gr, 0.2, False)
            pgd = {k: v.detach() for k, v in pg.items()}
            prd = {k: v.detach() for k, v in pr.items()}
            opt.apply(pgd, cg)
            opt.apply(prd, cr)
            pg, pr = pgd, prd
        if r > 0:
            times.append(time.time() - t0)
    times.sort()
    med = times[len(times) // 2]
    base = {"value": round(batch / med, 4), "unit": "frame-pairs/s", "cores": cores, "host_cpu_count": os.cpu_count(), "kind": "port",
            "sample": f"{reps} full adversarial steps (PWC fwd + gen fwd + 3x recover fwd + both backward + clipped Adam) at "
                      f"batch {batch}, 384x640 -> 192x384, median; PyTorch-CPU oracle with {cores} threads of the host's "
                      f"{os.cpu_count()} logical CPUs (more threads are slower; TF-1.13 itself is not installable here); same weights "
                      "and frame pairs as the GPU leg"}
    return base, parity


def parity_after(gpu_after, i1, i2, steps_done, tol=None):
    """Second parity check, on the weights the warm-up + timed steps produced: oracle forward / losses / both gradient passes on those
    weights against what the HIP path computes from them right after the timed region (same engine, same tuned kernels).

    The oracle runs in float64 from the flow on (the PWC flow itself is checked against the fp32 oracle, as at step 0): the checker has to be
    more accurate than what it checks.  It runs a second time in float32, as the YARDSTICK: how far a plain fp32 evaluation of the same graph
    on the same weights is from float64.  On freshly initialised weights that is ~1e-6; a trained state can be far worse conditioned (round 6,
    3 005 steps on the four synthetic pairs: the fp32 PyTorch oracle's mask is 4.2e-3 from float64 and its generator gradient 3.5e-3 in the
    norm -- the HIP path 2.7e-3 / 2.1e-3).  Every quantity is therefore gated at max(tol, 2 x the fp32 oracle's own deviation)."""
    from oracle import oracle_torch as O
    tol = tol or PARITY_TOL
    pp = {k: v.clone() for k, v in gpu_after["weights"][0].items()}
    batch = i1.shape[0]

    class C(O.Flags):
        batch_size = batch
    with torch.no_grad():
        image, flow, _ = O.prepare_inputs(pp, i1, i2, C)

    def evaluate(dt):
        pg, pr = ({k: v.detach().clone().to(dt).requires_grad_(True) for k, v in d.items()} for d in gpu_after["weights"][1:])
        out = O.forward_from_flow(pg, pr, image.to(dt), gpu_after["flow"].to(dt), C)
        return {"mask": out["mask"].detach().double(), "pred": torch.cat([out["pred"], out["pred_c"], out["pred_img"]], 0).detach().double(),
                "losses": {k: float(out[k]) for k in gpu_after["losses"]},
                "grads": {"generator": {k: v.double() for k, v in O.grads_of(out["generator"], pg).items()},
                          "recover": {k: v.double() for k, v in O.grads_of(out["recover"], pr).items()}}}

    ref, f32 = evaluate(torch.float64), evaluate(torch.float32)
    hip = {"mask": gpu_after["mask"].double(), "pred": gpu_after["pred"].double(), "losses": gpu_after["losses"],
           "grads": {"generator": {k: v.double() for k, v in gpu_after["grads"][0].items()},
                     "recover": {k: v.double() for k, v in gpu_after["grads"][1].items()}}}
    rel = lambda a, b: float((a.double() - b.double()).abs().max()) / max(1e-6, float(b.abs().max()))

    def deviation(x):  # x against the float64 oracle
        d = {"mask_max_abs_err": float((x["mask"] - ref["mask"]).abs().max()), "pred_rel_err": rel(x["pred"], ref["pred"]),
             "max_rel_loss_err": max(abs(x["losses"][k] - ref["losses"][k]) / max(1.0, abs(ref["losses"][k])) for k in ref["losses"]),
             "grad_max_rel_err": {}, "grad_worst_variable": {}, "grad_rel_l2_err": {}, "grad_elements_over_tolerance": {}}
        # every parameter gradient of both networks: |x - oracle| relative to max(max|ref tensor|, 1e-3 x the network's largest element)
        for tag, g in ref["grads"].items():
            got = x["grads"][tag]
            scale = max(float(v.abs().max()) for v in g.values())
            floor = {k: max(float(g[k].abs().max()), 1e-3 * scale) for k in g}
            errs = {k: float((got[k] - g[k]).abs().max()) / floor[k] for k in g}
            wv = max(errs, key=errs.get)
            d["grad_worst_variable"][tag] = wv
            d["grad_max_rel_err"][tag] = float("%.3e" % errs[wv])
            d["grad_rel_l2_err"][tag] = float("%.3e" % (sum(float((got[k] - g[k]).pow(2).sum()) for k in g) /
                                                        max(sum(float(g[k].pow(2).sum()) for k in g), 1e-60)) ** 0.5)
            d["grad_elements_over_tolerance"][tag] = "%d of %d" % (sum(int(((got[k] - g[k]).abs() > tol * floor[k]).sum()) for k in g),
                                                                    sum(g[k].numel() for k in g))
        return d

    res = {"after_steps": steps_done, "adam_step": gpu_after["adam_step"],
           "weights_rel_change_since_step0": {k: float("%.3e" % v) for k, v in gpu_after["weights_rel_change"].items()},
           "flow_rel_err": rel(gpu_after["flow"], flow),
           "oracle_dtype": "float64 (generator, recover, losses, both backward passes) on the HIP path's flow; the flow itself against the fp32 oracle"}
    dh, dy = deviation(hip), deviation(f32)
    res.update(dh)
    res["fp32_oracle_vs_float64"] = {k: dy[k] for k in ("mask_max_abs_err", "pred_rel_err", "max_rel_loss_err", "grad_max_rel_err", "grad_rel_l2_err")}
    detail = {}
    for tag, wv in dh["grad_worst_variable"].items():  # (diagnostic: the deviating tensor itself, when it is small)
        if dh["grad_max_rel_err"][tag] > tol and ref["grads"][tag][wv].numel() <= 512:
            detail[tag] = {"hip": [float("%.4e" % v) for v in hip["grads"][tag][wv].flatten().tolist()],
                           "oracle": [float("%.4e" % v) for v in ref["grads"][tag][wv].flatten().tolist()]}
    if detail:
        res["grad_worst_values"] = detail
    res["tolerance"] = tol
    moved = all(v > 0.0 for v in gpu_after["weights_rel_change"].values()) and gpu_after["adam_step"] >= 2 * steps_done
    res["optimizer_ran_every_step"] = moved
    # Gates.  Forward quantities and the relative L2 error of each network's whole gradient: <= max(tol, 2 x the fp32 oracle's deviation); no
    # single gradient element further than max(50 x tol, 2 x the fp32 oracle's worst element) from the float64 oracle.  The element-wise
    # maximum, the variable it sits in and the number of elements beyond tol are reported beside it.  Why not "every element <= tol" (what the
    # parity TESTS hold at step 0, tests/test_config2_gpu.py): legitimate cases exceed it on trained weights -- (a) fp32, 505 steps:
    # FlownetS/flow2/biases, a sum over 55 296 pixels with sum|dU| = 0.12 that cancels to 1.9e-4: the HIP path is 2.2e-6 off (1.2e-2 of the
    # element, 1.8e-5 of sum|dU|; the fp32 PyTorch oracle itself 5e-7), fp32 rounding of the forward chain entering through prediction -
    # target; 4 of 3.4 M recover elements beyond 1e-3, L2 of the network's gradient 8.6e-5; (b) fp16 convolutions: a leaky-ReLU unit whose
    # pre-activation lies within fp16 rounding of 0 takes the other slope (FlownetS/bconv4 channel 99 on the flow-free recover input: its bias
    # gradient halves, L2 3.4e-3) -- profiles/NOTES.md, round 6.  A skipped or wrong launch moves whole tensors: L2 and elements of order 1.
    lim = lambda own, k=1.0: max(k * tol, 2.0 * own)
    fwd_ok = res["flow_rel_err"] <= tol and all(dh[k] <= lim(dy[k]) for k in ("mask_max_abs_err", "pred_rel_err", "max_rel_loss_err"))
    grads_ok = all(dh["grad_rel_l2_err"][t] <= lim(dy["grad_rel_l2_err"][t]) and dh["grad_max_rel_err"][t] <= lim(dy["grad_max_rel_err"][t], 50.0)
                   for t in dh["grad_rel_l2_err"])
    res["gate"] = "flow <= %g; mask / predictions / losses / relative L2 error of each network's gradient <= max(%g, 2 x the fp32 oracle's own " \
                  "deviation from float64); every gradient element <= max(%g, 2 x the fp32 oracle's worst element) of max(max|tensor|, 1e-3 x " \
                  "the network's largest gradient element)" % (tol, tol, 50 * tol)
    res["ok"] = bool(moved and fwd_ok and grads_ok)
    return res


def ensemble_workload(eng, frames_u8, shifts, reps):
    """BASELINE.json configs[3] (test_generator_ensemble.py:47-114, adversarial_learner.py:525-592): per frame, the four
    central crops x `shifts` temporal partners, PWC-Net + generator forward each.  The four crops are the batch of one plan.
    Timed: crop / resize kernels + forward of every (frame, shift); returns frames/s."""
    from unsupervised_detection_amd import data
    crops = (0.85, 0.9, 0.95, 1.0)
    n = frames_u8.shape[0]
    imgs = data.preprocess_image(frames_u8)  # reader preprocessing (before the timed region, as in the headline)

    def pairs_of(t):
        for s in shifts:
            yield imgs[t:t + 1], imgs[(t + s) % n:(t + s) % n + 1]

    def stage(pair):  # crop / resize kernels + the frozen PWC-Net of this pair on the plan's prefetch lanes
        a, b = pair
        eng.prefetch_flow(torch.cat([data.central_cropping(a, c) for c in crops], 0), torch.cat([data.central_cropping(b, c) for c in crops], 0))

    def run(frames):  # as learner.inference() does it: PWC flow of pair k+1 beside the generator pass of pair k
        todo = [p for t in frames for p in pairs_of(t)]
        stage(todo[0])
        for k in range(len(todo)):
            eng.prefetch_consume()
            if k + 1 < len(todo):
                stage(todo[k + 1])
            eng.forward_in_place(0)
    run([0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run([r % n for r in range(reps)])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"workload": "BASELINE.json configs[3]: 4 central crops x %d temporal shifts, PWC flow + generator forward, 384x640 -> 192x384, "
                        "crops batched as one plan (B=4)" % len(shifts),
            "frames": reps, "frames_per_s": round(reps / dt, 3), "ms_per_frame": round(dt / reps * 1e3, 3),
            "alg_gflop_per_frame": ENSEMBLE_GFLOP_PER_FRAME * len(shifts) / 4.0,
            "tflops_algorithmic": round(ENSEMBLE_GFLOP_PER_FRAME * len(shifts) / 4.0 * reps / dt / 1e3, 2)}


def dump_outputs(out_dir, eng, st):
    """--dump-outputs: what the last timed step computed, as float32 DIR/<name>.npy -- its losses, the flow, mask and predictions of
    its forward pass, both networks' gradients and the weights its optimizer left.  Must run before any other work on the plan (the
    buffers are overwritten by the next forward).  Above DUMP_LIMIT_BYTES in all (batches above 8) every array becomes the same fixed,
    seeded sample of its flattened elements (the losses stay whole)."""
    import numpy as np
    arrays = {"losses": eng.buffer("losses").reshape(-1), "flow": eng.buffer("flow"), "mask": eng.buffer("mask"), "pred": eng.buffer("pred"),
              "grad_generator": st.g_gen, "grad_recover": st.g_rec, "weights_generator": st.w_gen, "weights_recover": st.w_rec}
    total = sum(4 * t.numel() for t in arrays.values())
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach().float().cpu()
        if total > DUMP_LIMIT_BYTES and t.numel() > 4096:
            keep = t.numel() * (DUMP_LIMIT_BYTES - 65536) // total  # (room for the files' headers)
            idx = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))[:keep].sort().values
            t = t.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), t.numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true", help="after the timed steps, also run every extra measurement and check of the line: "
                    "CPU-oracle leg and parity checks, reference schedule, ensemble workload, profiling pass (roofline, hbm_kernels), "
                    "gradient-exchange timings (--no-cpu-baseline, --cpu-reps, --cycles, --ensemble-frames, --pmc-json and --save-state act only "
                    "with --full)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the last timed step computed (losses, flow, mask, "
                    "predictions, gradients, updated weights) to DIR/<name>.npy in float32, at most 64 MB in all")
    ap.add_argument("--batch", type=int, default=0, help="frame pairs per GPU (BASELINE.json: 4; 2 with --fp16-convs)")
    ap.add_argument("--fp16-convs", action="store_true", help="BASELINE.json configs[4]: the convolution GEMMs multiply in fp16 with fp32 "
                    "accumulation (udet_config.conv_fp16), batch 2/GPU, SegTrackV2-shaped pairs (its reader resizes to the same 384x640); "
                    "not a reference capability -- parity tolerance 2e-2.  The default run is the fp32 headline.")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU-oracle leg (and with it the parity check)")
    ap.add_argument("--no-pipeline", action="store_true", help="no cross-step prefetch of the PWC flow (every step serial in itself)")
    ap.add_argument("--extra-streams", type=int, default=0, help="robustness probe: create (and use once) this many PyTorch streams before "
                    "the plan is built, which shifts ROCm's stream -> hardware-queue assignment the way a process group's streams do; the "
                    "plan's lane placement (udet_plan_lane_queues) must keep the step time unchanged")
    ap.add_argument("--no-autotune", action="store_true", help="use the built-in tile heuristics instead of the one-off autotune pass")
    ap.add_argument("--tune-cache", default="", help="file of tuned configurations: loaded when it exists (no tuning pass), written otherwise")
    ap.add_argument("--trace-only", action="store_true", help="warm-up + timed steps and nothing else (for rocprofv3 kernel traces: "
                    "with --tune-cache of an earlier run the trace holds steps only)")
    ap.add_argument("--allow-experiment-build", action="store_true", help="tools/knob_bench.py only: accept libudet_exp.so (the -DUDET_EXPERIMENT "
                    "build with the lane / work-skipping knobs); the line then says so and its numbers are not product numbers")
    ap.add_argument("--save-state", default="", help="diagnostics: torch.save the trained flat weights (generator, recover) and the HIP path's "
                    "gradients on them after the timed region -- for inspecting a post-region parity deviation offline with the oracle")
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=3, help="reference-schedule cycles (1 recover step + 3 generator steps each) timed "
                    "after the headline region; 0 skips that extra measurement")
    ap.add_argument("--ensemble-frames", type=int, default=12, help="frames of the configs[3] ensemble workload timed after the headline "
                    "region (extra field `ensemble`); 0 skips it")
    ap.add_argument("--pmc-json", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r06_pmc_step.json"),
                    help="PMC counters of whole steps collected offline with tools/pmc_step.py (separate rocprofv3 --pmc passes); fills "
                         "roofline.traffic with the convolution kernels' HBM bytes per step")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.trace_only:
        args.no_cpu_baseline, args.cycles, args.ensemble_frames = True, 0, 0
    if args.batch <= 0:
        args.batch = 2 if args.fp16_convs else 4

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if "WORLD_SIZE" not in os.environ and args.gpus > 1:
            # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, the command the module
            # docstring shows) and hand their output / exit code through -- rank 0 of the children prints the one JSON line
            import socket
            import subprocess
            with socket.socket() as so:
                so.bind(("127.0.0.1", 0))
                port = so.getsockname()[1]
            env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
                   "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
            return subprocess.run(cmd, env=env).returncode
        raise SystemExit(f"--gpus {args.gpus} != WORLD_SIZE {world}")
    # UDET_BENCH_ONE_GPU=1 (testing aid for a 1-GPU box): every rank uses cuda:0 and the collectives run over gloo, which
    # exercises the multi-process control flow of this script; the numbers of such a run mean nothing.
    one_gpu = os.environ.get("UDET_BENCH_ONE_GPU") == "1"
    if one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    import torch.distributed as dist
    # UDET_DP_WORLD1=1 (one-GPU box): a process group of ONE rank on the RCCL backend, and the gradient exchange issued although there is
    # nobody to exchange with (trainer._dp_active) -- the N > 1 code path of this script, call for call: init_process_group("nccl",
    # device_id), both all-reduces on their streams, the event hand-over, allreduce_ms, destroy.  It says nothing about scaling.
    dp = world > 1 or os.environ.get("UDET_DP_WORLD1") == "1"
    json_out = sys.stdout
    if dp:
        # RCCL (ROCm 7) prints a version banner with printf on fd 1 when the first communicator comes up; it is flushed at process exit, i.e.
        # BEHIND the JSON line.  The contract is ONE JSON line on stdout: keep a private handle on the real stdout for that line and point
        # fd 1 at stderr for everything else (native libraries included).
        sys.stdout.flush()
        json_out = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if world == 1 and "MASTER_PORT" not in os.environ:
            import socket
            with socket.socket() as so:
                so.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(so.getsockname()[1])
        if world == 1:
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from unsupervised_detection_amd import data
    from unsupervised_detection_amd import weights as W
    from unsupervised_detection_amd._ffi import lib
    from unsupervised_detection_amd.engine import BOTH, Engine, EngineConfig
    from unsupervised_detection_amd.trainer import TrainState, exchange_alone, flush_weights, train_step

    # The work-skipping ablation mask and the lane knobs of earlier rounds are compiled out of libudet.so (csrc/plan.h: plan_knob() is a
    # constant 0 without -DUDET_EXPERIMENT); the only build that has them exports udet_exp_knob.  A headline number from that build is
    # refused here, so the line itself says which library produced it.
    from unsupervised_detection_amd import _ffi as _ffi_mod
    experiment_build = hasattr(lib, "udet_exp_knob")
    if experiment_build and not args.allow_experiment_build:
        raise SystemExit("bench.py: the loaded library exports udet_exp_knob (libudet_exp.so): not the release library")
    release_library = {"file": os.path.basename(getattr(_ffi_mod, "LIB_PATH", "?")),
                       "experiment_knobs": "PRESENT (libudet_exp.so: not a product number)" if experiment_build else "compiled out",
                       "debug_hooks_loaded": "unsupervised_detection_amd._devel" in sys.modules}

    extra_streams = [torch.cuda.Stream() for _ in range(args.extra_streams)]
    for s_ in extra_streams:
        with torch.cuda.stream(s_):
            torch.zeros(16, device="cuda").add_(1.0)
    torch.cuda.synchronize()
    eng = Engine(EngineConfig(batch_size=args.batch, conv_fp16=args.fp16_convs), device=f"cuda:{local_rank}")
    loaded, shipped = 0, 0
    if args.tune_cache and os.path.exists(args.tune_cache):
        loaded = max(0, int(lib.udet_tune_load(args.tune_cache.encode())))  # < 0: a file of another build -> tune again
    elif not args.tune_cache and not args.no_autotune:
        shipped = int(lib.udet_tune_load(SHIPPED_TUNE.encode()))
        if shipped < 0:  # (a build whose tuning ABI moved on: every shape is timed, and runs may differ in their last bits)
            print("bench.py: %s is not a tuning file of this build; autotuning every shape" % os.path.relpath(SHIPPED_TUNE, ROOT),
                  file=sys.stderr, flush=True)
            shipped = 0
    # (N > 1: rank 0 tunes and the other ranks load its configurations -- TrainState._autotune_shared -- so every GPU runs the same kernels)
    st = TrainState(eng, seed=8964, autotune=not (args.no_autotune or loaded > 0))  # identical weights on every rank; kernels autotuned once
    if args.tune_cache and not loaded and not args.no_autotune and rank == 0:
        lib.udet_tune_save(args.tune_cache.encode())
    w0 = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:  # the oracle leg starts from the same weights
        w0 = tuple(W.as_dict(t.cpu().clone(), n) for t, n in ((st.w_pwc, W.NET_PWC), (st.w_gen, W.NET_GEN), (st.w_rec, W.NET_REC)))
    # NPAIRS distinct resident batches per rank, visited round-robin (distinct data per rank: weak scaling); batch 0 is the one
    # the parity check and the CPU-oracle leg use
    NPAIRS = 4
    batches = []
    for i in range(NPAIRS):
        f1, f2 = data.synthetic_davis_pairs(args.batch, 8964 + rank + 1000 * i)
        batches.append((data.preprocess_image(torch.from_numpy(f1).cuda()), data.preprocess_image(torch.from_numpy(f2).cuda())))
    img1, img2 = batches[0]

    # every launch of the step goes to one explicitly created stream (not the legacy null stream, whose implicit
    # synchronisation with blocking streams would serialise the plan's side streams on some runtimes)
    torch.cuda.synchronize()
    work_stream = torch.cuda.Stream()
    torch.cuda.set_stream(work_stream)

    def barrier():
        if dp:
            dist.barrier()
        torch.cuda.synchronize()

    def stage(msg):  # UDET_BENCH_TRACE=1: progress markers on stderr (debugging a multi-process launch)
        if os.environ.get("UDET_BENCH_TRACE") == "1":
            print("[bench rank %d] %s" % (rank, msg), file=sys.stderr, flush=True)

    # the step-0 forward of the HIP path on the initial weights: what the oracle leg is compared with (untimed)
    gpu_first = None
    if w0 is not None:
        eng.forward(img1, img2, 3)
        torch.cuda.synchronize()
        gpu_first = {k: eng.buffer(k).cpu().clone() for k in ("image", "flow", "mask", "pred")}
        gpu_first["losses"] = eng.losses()

    # cross-step pipelining (trainer.train_step): every step enqueues the frozen PWC-Net's flow of the NEXT pair beside
    # its own backward pass.  The pipeline is primed before the timed region (>= 1 warm-up step or an explicit prefetch),
    # so the K timed steps contain exactly K PWC forwards, K generator/recover forwards, K x both backward, K x 2 applies.
    pipelined = not args.no_pipeline
    nxt = (img1, img2) if pipelined else None  # (the later, single-batch measurements keep re-using batch 0)
    kstep = [0]  # running step index: step k trains on batches[k % NPAIRS] and prefetches batches[(k + 1) % NPAIRS]

    def run_step(which=BOTH, group=None):
        a, b = batches[kstep[0] % NPAIRS]
        n = batches[(kstep[0] + 1) % NPAIRS] if pipelined else None
        kstep[0] += 1
        train_step(st, a, b, which, group=group, next_pair=n)
    if pipelined and args.warmup == 0:
        eng.prefetch_flow(img1, img2)
        st._prefetched = (img1, img2)
    stage("plan built, weights packed, autotuned")
    for _ in range(args.warmup):
        run_step()
    barrier()
    lane_nq, lane_q = eng.lane_queues()  # (placed by the first warm-up step on this stream; this call only reads the layout)
    stage("warm-up done")
    # per-step completion events on the stream every launch of the step is issued from (the plan's side streams are joined to
    # it before the optimizer applies): step k's duration = event k - event k-1 -> the distribution behind the mean
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for k in range(args.steps):
        run_step()
        marks[k + 1].record()
    barrier()
    dt = time.perf_counter() - t0
    step_ms = sorted(marks[k].elapsed_time(marks[k + 1]) for k in range(args.steps))
    pct = lambda q: step_ms[min(len(step_ms) - 1, int(round(q * (len(step_ms) - 1))))] if step_ms else None
    tmax = torch.tensor([dt], device="cuda", dtype=torch.float64)
    if dp:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    ms = dt / args.steps * 1e3
    pairs_per_s = args.batch * world * args.steps / dt
    losses = eng.losses()
    stage("timed region done")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, eng, st)
    headline = {
        "metric": "frame-pairs/sec per adversarial step, DAVIS 480p batch4, 1/2/4/8 GPU",
        "value": round(pairs_per_s, 3), "unit": "frame-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms, 3),
        # SURVEY 8d protocol: per-step times from HIP events on the launch stream over the same K timed steps
        "ms_per_step_median": round(pct(0.5), 3), "ms_per_step_p95": round(pct(0.95), 3), "ms_per_step_min": round(step_ms[0], 3),
        "ms_per_step_max": round(step_ms[-1], 3), "value_at_median": round(args.batch * world / (pct(0.5) * 1e-3), 3),
        "resident_batches": NPAIRS,
        "lanes": {"hardware_queues_in_use": lane_nq, "queue_of_lane": lane_q, "extra_streams": args.extra_streams},
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f16 x f16 -> f32 in the convolution MFMAs (fp32 tensors, losses, reductions, optimizer)" if args.fp16_convs else "f32",
        "data": "synthetic (DAVIS-480p-shaped pairs, reader preprocessing applied before timing; random-init weights)",
        "config": {"workload": ("BASELINE.json configs[4]: SegTrackV2-shaped pairs -> 384x640 (PWC) -> 192x384, batch %d/GPU, fp16 convs with "
                                "fp32 loss accumulation, PWC flow + generator + 3x inpainter fwd + both backward + clipped Adam" % args.batch)
                               if args.fp16_convs else
                               "BASELINE.json configs[%d]: DAVIS2016 480p -> 384x640 (PWC) -> 192x384, batch %d/GPU, "
                               "PWC flow + generator + 3x inpainter fwd + both backward + clipped Adam" % (1 if world == 1 else 2, args.batch),
                   "global_batch": args.batch * world, "parallelism": "dp%d" % world,
                   "alg_gflop_per_pair": ALG_GFLOP_PER_PAIR},
        "step_tflops_algorithmic": round(ALG_GFLOP_PER_PAIR * 1e9 * args.batch * world / (ms * 1e-3) / 1e12, 2),
        "execution": {"autotuned_shapes": getattr(st, "tuned_shapes", 0) or loaded, "tuned_configurations_loaded": loaded,
                      "shipped_configurations_loaded": shipped,
                      "tune_rejected": int(lib.udet_tune_rejected()), "pipelined": nxt is not None,
                      "note": "step = forward(prefetched PWC flow) + PWC flow of the next pair beside both backward passes "
                              "+ 2 applies; every timed step contains all of that work exactly once"},
        "process_group": ({"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                           "forced_at_world_size_one": world == 1} if dp else None),
        "losses": {k: round(v, 5) for k, v in losses.items()},
        "release_library": release_library,
    }
    if not args.full and not args.trace_only:  # a plain run: the headline and nothing else
        if rank == 0:
            print(json.dumps(headline), file=json_out, flush=True)
        if dp:
            dist.barrier()
            dist.destroy_process_group()
        return 0
    # Parity AFTER the timed region (the step-0 check alone does not show that the timed steps did their work): the weights the
    # K + W steps left behind are the starting point of a second comparison with the oracle -- forward, losses and BOTH backward passes of
    # the HIP path on them, by the very calls the timed loop makes (eng.forward / eng.backward inside train_step), against the CPU oracle on
    # the same weights.  Also: how far the timed steps moved the weights (an optimizer that did not run leaves 0).
    gpu_after = None
    if w0 is not None:
        if getattr(st, "_prefetched", None) is not None:  # (drain the pipeline: the check runs its own forward)
            eng.forward_prefetched(3)
            st._prefetched = None
        torch.cuda.synchronize()
        wa = tuple(W.as_dict(t.cpu().clone(), n) for t, n in ((st.w_pwc, W.NET_PWC), (st.w_gen, W.NET_GEN), (st.w_rec, W.NET_REC)))
        delta = {}
        for name, d0, d1 in (("generator", w0[1], wa[1]), ("recover", w0[2], wa[2])):
            num = sum(float((d1[k] - d0[k]).double().pow(2).sum()) for k in d0) ** 0.5
            den = sum(float(d0[k].double().pow(2).sum()) for k in d0) ** 0.5
            delta[name] = num / max(den, 1e-30)
        flush_weights(st)  # (re-layout of the networks the last step updated -- what the next train_step would do first)
        eng.forward(img1, img2, 3)
        g_gen_chk, g_rec_chk = torch.zeros_like(st.w_gen), torch.zeros_like(st.w_rec)
        eng.backward(BOTH, st.w_gen, st.w_rec, g_gen_chk, g_rec_chk)
        torch.cuda.synchronize()
        gpu_after = {k: eng.buffer(k).cpu().clone() for k in ("image", "flow", "mask", "pred")}
        gpu_after["losses"] = eng.losses()
        gpu_after["grads"] = (W.as_dict(g_gen_chk.cpu(), W.NET_GEN), W.as_dict(g_rec_chk.cpu(), W.NET_REC))
        gpu_after["weights"] = wa
        gpu_after["weights_rel_change"] = delta
        gpu_after["adam_step"] = int(eng.adam_step)
        if args.save_state:
            torch.save({"w_gen": st.w_gen.cpu(), "w_rec": st.w_rec.cpu(), "g_gen": g_gen_chk.cpu(), "g_rec": g_rec_chk.cpu(),
                        "flow": gpu_after["flow"], "batch": args.batch, "fp16_convs": bool(args.fp16_convs)}, args.save_state)

    # the gradient exchange alone, timed after the headline region: the SAME two collectives a BOTH step issues (recover gradients on
    # the communication stream, generator gradients on the compute stream, the compute stream then waits) with nothing to hide behind
    allreduce_ms = None
    if dp:
        barrier()
        t0 = time.perf_counter()
        for _ in range(10):
            exchange_alone(st)
        barrier()
        ar = torch.tensor([(time.perf_counter() - t0) / 10 * 1e3], device="cuda", dtype=torch.float64)
        dist.all_reduce(ar, op=dist.ReduceOp.MAX)
        allreduce_ms = round(float(ar.item()), 4)
    # how much of that the step hides: the same K steps WITHOUT the exchange (group=False; the replicas drift apart from here on,
    # nothing below depends on them agreeing).  exposed = what the exchange adds to a step; hidden = the rest of its stand-alone time
    exchange = None
    if dp:
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            run_step(group=False)
        barrier()
        nx = torch.tensor([(time.perf_counter() - t0) / args.steps * 1e3], device="cuda", dtype=torch.float64)
        dist.all_reduce(nx, op=dist.ReduceOp.MAX)
        ms_noex = float(nx.item())
        exposed = max(0.0, ms - ms_noex)
        exchange = {"ms_per_step_without_exchange": round(ms_noex, 3), "exchange_exposed_ms": round(exposed, 4),
                    "overlap_hidden_ms": round(max(0.0, allreduce_ms - exposed), 4),
                    "how": "recover gradients reduced on a communication stream behind udet_stream_wait_grads (under the rest of the "
                           "generator-loss pass), generator gradients after the backward; allreduce_ms = those two collectives alone "
                           "(same streams, nothing to overlap with); hidden = allreduce_ms - exposed"}

    # the reference's own schedule (adversarial_learner.py:383-398 with iter_gen=3 / iter_rec=1): a 4-step cycle
    # = 16 pairs, 4 forwards, 1 recover-loss backward, 3 generator-loss backwards.  Reported beside the headline number.
    ref_cycle = None
    if args.cycles > 0:
        from unsupervised_detection_amd.engine import GEN, REC
        order = (REC, GEN, GEN, GEN)
        for w in order:  # one untimed cycle: the single-backward paths' first launches
            run_step(w)
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.cycles):
            for w in order:
                run_step(w)
        barrier()
        dc = torch.tensor([time.perf_counter() - t0], device="cuda", dtype=torch.float64)
        if dp:
            dist.all_reduce(dc, op=dist.ReduceOp.MAX)
        dc = float(dc.item())
        ref_cycle = {"schedule": "1 recover step + 3 generator steps (iter_rec=1, iter_gen=3)", "cycles": args.cycles,
                     "ms_per_step": round(dc / (4 * args.cycles) * 1e3, 3),
                     "frame_pairs_per_s": round(args.batch * world * 4 * args.cycles / dc, 3),
                     "alg_gflop_per_pair": 184.1}

    if getattr(st, "_prefetched", None) is not None:  # drain the pipeline: what follows is self-contained
        eng.forward_prefetched(3)
        st._prefetched = None
    if args.trace_only:
        if rank == 0:
            print(json.dumps({"metric": "frame-pairs/sec per adversarial step, DAVIS 480p batch4, 1/2/4/8 GPU", "value": round(pairs_per_s, 3),
                              "unit": "frame-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
                              "ms_per_step_median": round(pct(0.5), 3), "trace_only": True, "tuned_configurations_loaded": loaded}), file=json_out, flush=True)
        if dp:
            dist.barrier()
            dist.destroy_process_group()
        return 0

    ensemble = None
    if args.ensemble_frames > 0 and args.batch == 4 and rank == 0:
        fe, _ = data.synthetic_davis_pairs(8, 77)
        ensemble = ensemble_workload(eng, torch.from_numpy(fe).cuda(), (1, 2, 3, 4), args.ensemble_frames)

    # per-kernel timing with HIP events on the launch stream: ONE extra, untimed step executed serially (the plan collapses
    # its side streams while profiling, so every launch group's duration is its stand-alone duration).
    # every rank runs the profiled step (it contains the gradient all-reduces: a rank that skipped it would leave the
    # others waiting in the collective); only rank 0 keeps the per-layer dump and reports
    import csv
    layers = []
    keep = os.environ.get("UDET_PROF_DUMP") if rank == 0 else None  # a caller-provided path is kept (per-layer CSV for analysis)
    dump = keep or os.path.join(tempfile.gettempdir(), "udet_layers_%d.csv" % os.getpid())
    if os.path.exists(dump):
        os.remove(dump)
    os.environ["UDET_PROF_DUMP"] = dump
    stage("reference schedule done; profiling pass")
    st._prefetched = None
    prof = eng.profile(lambda: train_step(st, img1, img2, BOTH))
    stage("profiling pass done")
    os.environ.pop("UDET_PROF_DUMP", None)
    if os.path.exists(dump):
        with open(dump) as f:
            # category, layer, kernel ms (sum of the launches' own start -> stop times), algorithmic GFLOP, MB[, bracket ms, kernels]
            # (last column, round 4 on: GFLOP the matrix pipe really issues -- a Winograd launch multiplies 16 / 36 of its direct form)
            layers = [(int(r[0]), r[1], float(r[2]), float(r[3]), float(r[4]), float(r[8]) if len(r) > 8 else float(r[3])) for r in csv.reader(f)]
        if not keep:
            os.remove(dump)

    rc = 0
    if rank == 0:
        conv_ms = sum(prof[c]["ms"] for c in ("conv_fwd", "conv_dgrad", "conv_wgrad"))
        conv_bracket_ms = sum(prof[c]["bracket_ms"] for c in ("conv_fwd", "conv_dgrad", "conv_wgrad"))
        conv_groups = sum(prof[c]["groups"] for c in ("conv_fwd", "conv_dgrad", "conv_wgrad"))
        alg_flops = ALG_GFLOP_PER_PAIR * 1e9 * args.batch
        # FLOPs of the launches actually executed: below the algorithmic figure because the image encoder of the three recover
        # calls is evaluated once (identical input), not three times -- the kernel-efficiency numerator
        exe_flops = sum(l[3] for l in layers if l[0] < 3) * 1e9 or alg_flops
        achieved = exe_flops / (conv_ms * 1e-3) / 1e12
        mfma_flops = sum(l[5] for l in layers if l[0] < 3) * 1e9 or exe_flops
        alg_bytes = sum(l[4] for l in layers if l[0] < 3) * 1e6  # MB column of the per-layer dump (plan_exec.hip: layer_bytes)
        wino = [l for l in layers if l[0] < 3 and l[5] < l[3] * 0.99]
        top = max((l for l in layers if l[0] < 3), key=lambda l: l[3], default=None)
        traffic, traffic_source = None, None
        # (the committed counter file was collected on the headline workload: fp32, batch 4 -- other workloads report null)
        if args.pmc_json and os.path.exists(args.pmc_json) and args.batch == 4 and not args.fp16_convs:
            with open(args.pmc_json) as f:
                pmc = json.load(f)
            conv = ("conv_igemm", "conv_wino", "conv_tile", "conv_thin", "conv_wgrad", "wgrad_reduce", "conv_splitk_epilogue", "tap_gather", "bn_dot", "bn_finish")
            fam = [k for k in pmc.get("kernel_families", []) if any(c in k["kernel"] for c in conv)]
            if "traffic_bytes_per_launch" in pmc:  # tools/pmc_report.py: one launch
                traffic = pmc["traffic_bytes_per_launch"]
            elif fam:  # tools/pmc_step.py: FETCH_SIZE x 2 + WRITE_SIZE of every dispatch, summed over the convolution kernels of one step
                traffic = int(sum(k["hbm_MB_per_step"] for k in fam) * 1e6)
            traffic_source = "%s (offline rocprofv3 --pmc passes over serial steps, not re-collected by this run; unit: bytes per step = " \
                             "per pass of all convolution launches, like `achieved`)" % os.path.relpath(args.pmc_json, os.path.dirname(os.path.abspath(__file__)))
        peak_tf = 2500.0 if args.fp16_convs else PEAK_FP32_MFMA_TFLOPS  # dense MFMA peak of the multiplication dtype (MI355X_MICROARCH.md)
        # EFFECTIVE peak of a launch family = matrix peak x (multiply-adds of the direct form / multiply-adds the family issues): 157.3 for
        # the direct families, 157.3 x 36/16 = 353.9 for fused Winograd F(2x2,3x3) (forward, backward-data and, round 5, the filter
        # gradient).  A launch credited with its direct-equivalent work is priced against THAT, so no fraction of the line exceeds 1.
        def eff_peak(l):
            return peak_tf * (l[3] / l[5] if l[5] > 0 else 1.0)
        top_launch = None
        if top is not None:
            top_tf = top[3] / top[2] if top[2] > 0 else 0.0  # GFLOP / ms = TFLOP/s
            top_launch = {"layer": top[1], "alg_gflop": round(top[3], 3), "ms": round(top[2], 4), "achieved": round(top_tf, 2),
                          "achieved_note": "direct-equivalent TFLOP/s (the reference algorithm's multiply-adds over the launch's duration)",
                          "effective_peak": round(eff_peak(top), 1), "frac": round(top_tf / eff_peak(top), 4),
                          "frac_note": "of effective_peak = matrix peak x 36/16 for a Winograd launch (it issues 16 of the direct form's 36 "
                                       "multiplications); equals the launch's matrix-pipe occupancy"}
        direct = [l for l in layers if l[0] < 3 and not l[5] < l[3] * 0.99]
        def fam_row(ls, scale):
            t, g, m = sum(l[2] for l in ls), sum(l[3] for l in ls), sum(l[5] for l in ls)
            return {"launch_groups_per_step": len(ls), "ms_per_step_serial": round(t, 3), "executed_gflop": round(g, 2),
                    "achieved": round(g / max(t, 1e-9), 2), "effective_peak": round(peak_tf * scale, 1),
                    "frac_of_effective_peak": round(m / max(t, 1e-9) / peak_tf, 4)}
        roofline = {"bound": "mfma",
                    "kernel": "conv_igemm_dma_kernel / conv_igemm_kernel / conv_wino_kernel (fused Winograd F(2x2,3x3), 3x3 stride-1 layers) / "
                              "conv_tile_kernel / conv_wgrad_kernel (v_mfma_f32_32x32x2_f32, "
                              "16x16x4 for <=16 output channels; conv_thin_* direct kernels for the 2-channel heads): every convolution "
                              "launch of one step, executed serially; duration = "
                              "the launch's own start -> stop HIP events (carried by its dispatch packet on the launch stream: the "
                              "kernel execution time rocprofv3 --kernel-trace reports)",
                    "achieved": round(achieved, 2), "peak": peak_tf, "unit": "TFLOP/s",
                    "frac": round(achieved / peak_tf, 4),
                    # the same executed GFLOP over the TIMED step (kernels of several lanes overlap there): what fraction of the
                    # chip's matrix peak the headline region itself sustains
                    "frac_step": round(exe_flops / (ms * 1e-3) / 1e12 / peak_tf, 4),
                    "frac_step_algorithmic": round(alg_flops / (ms * 1e-3) / 1e12 / peak_tf, 4),
                    "numerator": "executed GFLOP of the launches (recover encoder A once instead of three times; the generator's NN x2 + 3x3 "
                                 "layers as four 2x2 convolutions: 16 of 36 tap products; the recover decoder's bilinear x2 + 4x4 layers of levels 1-3 as four "
                                 "3x3 convolutions on the low-resolution source: 9 of 16) -- `achieved_algorithmic` / `frac_algorithmic` divide "
                                 "the reference graph's 871.78 GFLOP by the same time",
                    "executed_gflop_per_step": round(exe_flops / 1e9, 2), "alg_gflop_per_step": round(alg_flops / 1e9, 2),
                    # Winograd F(2x2,3x3) launches (conv_wino_kernel) are credited with the multiply-adds of the DIRECT convolution they
                    # replace (the reference's algorithm: `achieved` / `frac` above); what the matrix pipe itself issues is 16 / 36 of
                    # that for those launches -- the pipe-occupancy view of the same time:
                    "winograd": {"launch_groups_per_step": len(wino), "ms_per_step_serial": round(sum(l[2] for l in wino), 3),
                                 "direct_equivalent_gflop": round(sum(l[3] for l in wino), 2),
                                 "achieved_direct_equivalent": round(sum(l[3] for l in wino) / max(sum(l[2] for l in wino), 1e-9), 2)},
                    "mfma_issued_gflop_per_step": round(mfma_flops / 1e9, 2),
                    "frac_mfma_issued": round(mfma_flops / (conv_ms * 1e-3) / 1e12 / peak_tf, 4),
                    # one statement per family and for the whole step: work credited / (time x effective peak).  For the whole step the
                    # effective peak is the time-weighted mix of the two, so frac_of_effective_peak == frac_mfma_issued by construction.
                    "families": {"direct": fam_row(direct, 1.0), "winograd_f2x2_3x3": fam_row(wino, 36.0 / 16.0)},
                    "effective_peak": round(peak_tf * exe_flops / max(mfma_flops, 1.0), 1),
                    "frac_of_effective_peak": round(mfma_flops / (conv_ms * 1e-3) / 1e12 / peak_tf, 4),
                    "achieved_algorithmic": round(alg_flops / (conv_ms * 1e-3) / 1e12, 2),
                    "frac_algorithmic": round(alg_flops / (conv_ms * 1e-3) / 1e12 / peak_tf, 4),
                    # HBM bytes from PMC counters are collected offline (tools/pmc_step.py, separate rocprofv3 --pmc passes, summaries
                    # under profiles/): the committed collection of this build, or the file given with --pmc-json; null without one
                    "traffic": traffic, "traffic_source": traffic_source,
                    # the comparator of `traffic`: SURVEY Appendix A's per-layer figure (input + output + weights in fp32, nothing fused;
                    # identical for a layer's forward, backward-data and backward-filter passes) summed over every convolution launch of
                    # the step -- the executed launches (recover encoder A once) and the reference graph's
                    "alg_bytes_per_step": int(alg_bytes), "alg_bytes_forward": int(sum(l[4] for l in layers if l[0] == 0) * 1e6),
                    "traffic_over_algorithmic": round(traffic / alg_bytes, 3) if traffic and alg_bytes else None,
                    "launch_groups_per_step": int(conv_groups), "avg_group_ms": round(conv_ms / max(conv_groups, 1), 4),
                    "conv_ms_per_step_serial": round(conv_ms, 3),
                    # the same launch groups bracketed by hipEventRecord before / after (adds event packets + dispatch gaps)
                    "conv_bracket_ms_per_step_serial": round(conv_bracket_ms, 3),
                    "frac_on_bracket_time": round(exe_flops / (conv_bracket_ms * 1e-3) / 1e12 / peak_tf, 4) if conv_bracket_ms > 0 else None,
                    "top_launch": top_launch}
        hbm = {}
        pmc_wcv = None
        if args.pmc_json and os.path.exists(args.pmc_json) and args.batch == 4 and not args.fp16_convs:
            with open(args.pmc_json) as f:
                pj = json.load(f)
            if "warp_cost_volume_MB_per_step" in pj:  # tools/pmc_step.py (round 4 on): the fused kernel's dispatches, whatever their rank
                pmc_wcv = pj
        p = prof["cost_volume"]
        if p["ms"] > 0:
            gbs = p["bytes"] / (p["ms"] * 1e-3) / 1e9
            hbm["warp_cost_volume"] = {"kernel": "warp_cost_volume_kernel (dense_image_warp + cost_volume + c1 slab segment in one launch per "
                                                 "pyramid level)",
                                       "alg_MB_per_step": round(p["bytes"] / 1e6, 2), "ms_per_step": round(p["ms"], 4), "launches": int(p["groups"]),
                                       "achieved_GBs": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK_HBM_GBS, 4)}
            if pmc_wcv is not None:
                w = hbm["warp_cost_volume"]
                w["traffic"] = int(pmc_wcv["warp_cost_volume_MB_per_step"] * 1e6)  # PMC: FETCH_SIZE x 2 + WRITE_SIZE, bytes per step
                w["traffic_over_algorithmic"] = round(w["traffic"] / max(p["bytes"], 1.0), 3)
                w["traffic_per_level"] = pmc_wcv["warp_cost_volume_dispatches_of_one_step"]
                w["traffic_source"] = os.path.relpath(args.pmc_json, os.path.dirname(os.path.abspath(__file__)))
            big = max((l for l in layers if l[0] == 4), key=lambda l: l[4], default=None)
            if big is not None and big[2] > 0:
                hbm["warp_cost_volume"]["largest_launch"] = {"level": big[1], "alg_MB": round(big[4], 2), "ms": round(big[2], 4),
                                                             "achieved_GBs": round(big[4] / big[2], 1),
                                                             "frac_of_8TBs": round(big[4] / big[2] / PEAK_HBM_GBS, 4)}
        out = dict(headline)
        out.update({
            "roofline": roofline, "hbm_kernels": hbm,
            "profile_ms_per_step_serial": {k: round(v["ms"], 3) for k, v in prof.items() if v["groups"] > 0},
            "allreduce_ms": allreduce_ms, "gradient_exchange": exchange,
            "reference_schedule": ref_cycle,
            "ensemble": ensemble,
        })
        if w0 is not None:
            out["cpu_baseline"], out["parity_check"] = cpu_baseline(w0, img1.cpu(), img2.cpu(), gpu_first, args.cpu_reps,
                                                                    tol=2e-2 if args.fp16_convs else None)
            if not out["parity_check"]["ok"]:
                rc = 1
            out["parity_check_after_timed_region"] = parity_after(gpu_after, img1.cpu(), img2.cpu(), args.steps + args.warmup,
                                                                  tol=2e-2 if args.fp16_convs else None)
            if not out["parity_check_after_timed_region"]["ok"]:
                rc = 1
        else:
            out["cpu_baseline"], out["parity_check"] = None, None
        print(json.dumps(out), file=json_out, flush=True)
        if rc:
            print("bench.py: PARITY CHECK FAILED: %s" % json.dumps(out["parity_check"]), file=sys.stderr, flush=True)
    if dp:
        dist.barrier()
        dist.destroy_process_group()
    return rc


if __name__ == "__main__":
    sys.exit(main())
