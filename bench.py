#!/usr/bin/env python3
"""bench.py -- samples/s of the MLA alternating-unimodal training step (main.py:419-476) on MI355X.

    python bench.py --gpus 1 --steps K --warmup W [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]; configs[2] for N>1): CREMA-D, --gs_flag, ResNet-18 audio+visual,
per-GPU batch 64 of synthetic (1x1024x128 spectrogram + 3x3x224x224 frames), fp32, weak scaling.
One "step" = joint encoder forward + 2 x {head fwd/CE/bwd, encoder backward, GS projection, SGD}.
Inputs are resident in HBM before the timed region.  Prints ONE JSON line on rank 0.  A plain run sets up, warms up,
times the K steps and reports `value` / `ms_per_step` only.  --dump-outputs DIR writes what the last timed step left the
caller (losses, logits, features, head, GS projector, a fixed sample of the updated encoder state) as DIR/<name>.npy.
--full adds, after the timed region,
`roofline` (dominant kernel = the implicit-GEMM convolution of the selected arithmetic, HIP events in a serialized pass after the
timed region; peak = bf16 MFMA rate / 6 products for split, the fp32 MFMA rate for f32),
`alt_math` (the same steps with the other conv arithmetic: --math split, the shipped default = exact 3-way bf16 operand
split, 6 bf16 MFMAs per fp32 product, fp32 in / out / accumulate, fp32-equivalent accuracy; f32 = the fp32 MFMA; N=1 only)
and `cpu_baseline` (the CPU oracle = "port" of the reference path, timed on this host's cores, N=1 only).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))

import torch  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3       # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_HBM_GBPS = 8000.0             # MI355X_MICROARCH.md: HBM3E ~8 TB/s
PEAK_SPLIT_TFLOPS = 16 * 157.3 / 6  # conv_math=split: bf16 MFMA (16x the fp32 rate, ~2.5 PF dense), six products per fp32 product
SPEC_HW, FRAMES, IMG_HW, N_CLASSES = (1024, 128), 3, (224, 224), 6


class Args:
    fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", True, "Normal"


def usable_cores() -> int:
    """CPU cores this process may really use: min(affinity, cgroup quota) -- the GPU box exposes far more
    cores than its CPU share, and oversubscribing torch's thread pool stalls for minutes."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, q // per))
            break
        except Exception:
            continue
    return max(1, min(n, 64))


def cpu_baseline(batch: int = 8, max_steps: int = 5, budget_s: float = 25.0, threads: int = 0) -> dict:
    """The CPU oracle (oracle/mla_oracle.py: the reference path restated on torch-CPU ATen kernels),
    timed on this host: bounded sample = up to `max_steps` MLA steps at batch `batch` (about `budget_s`
    seconds of CPU work) after one warm-up step.  threads = 0: every core this process may use."""
    from oracle import mla_oracle as O
    cores = min(threads, usable_cores()) if threads > 0 else usable_cores()
    torch.set_num_threads(cores)
    print(f"[bench] cpu_baseline: {cores} threads, batch {batch}", file=sys.stderr, flush=True)
    st = O.MLAState(O.make_resnet18_params("audio", 1), O.make_resnet18_params("visual", 2), O.make_head_params(512, 6, 3))
    g = torch.Generator().manual_seed(0)
    spec = torch.randn((batch,) + SPEC_HW, generator=g) * 4.4849 - 5.081
    image = torch.randn((batch, 3, FRAMES) + IMG_HW, generator=g)
    label = torch.randint(0, N_CLASSES, (batch,), generator=g)
    t_start = time.perf_counter()
    O.mla_step(st, spec, image, label, 0, 100)
    print(f"[bench] cpu_baseline warm-up step {time.perf_counter() - t_start:.2f} s", file=sys.stderr, flush=True)
    ts = []
    for s in range(max_steps):
        t0 = time.perf_counter()
        O.mla_step(st, spec, image, label, s + 1, 100)
        ts.append(time.perf_counter() - t0)
        print(f"[bench] cpu_baseline step {s}: {ts[-1]:.2f} s", file=sys.stderr, flush=True)
        if time.perf_counter() - t_start > budget_s:
            break
    med = sorted(ts)[len(ts) // 2]
    return {"value": round(batch / med, 3), "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{len(ts)} MLA steps at batch {batch} (same shapes, fp32, torch-CPU ATen), median, after 1 warm-up"}


STATE_SAMPLE = 1 << 20      # elements of each encoder's updated state written by --dump-outputs (fixed, seeded positions)


def collect_outputs(trainer, model) -> dict:
    """What train_step leaves its caller after the last timed step, as host float32 arrays: the three losses it returns,
    each modality's logits and pooled features, the updated head and GS projector, and STATE_SAMPLE fixed positions
    (numpy seed 0, sorted) of each encoder's updated parameters + BatchNorm buffers, reference layout, keys sorted."""
    import numpy as np
    trainer.join()
    torch.cuda.synchronize()
    host = lambda t: t.detach().float().cpu().numpy()
    out = {k: host(v) for k, v in trainer.losses.items()}
    for tag, _g, _e in trainer.encoders:
        out["out_" + tag], out["feat_" + tag] = host(trainer.last["out_" + tag]), host(trainer.last[tag])
    head = model.fusion_module.fc_out
    out["head_weight"], out["head_bias"], out["gs_Pl"] = host(head.weight), host(head.bias), host(trainer.gs_plugin.Pl)
    for _t, grp, enc in trainer.encoders:
        sd = enc.state_dict()
        flat = torch.cat([sd[k].detach().reshape(-1).float() for k in sorted(sd) if sd[k].is_floating_point()])
        n = flat.numel()
        idx = np.sort(np.random.default_rng(0).choice(n, size=min(n, STATE_SAMPLE), replace=False))
        out[grp + "_state_sample"] = host(flat[torch.from_numpy(idx).to(flat.device)])
    return out


def dump_outputs(d: str, outputs: dict) -> None:
    import numpy as np
    os.makedirs(d, exist_ok=True)
    total = sum(v.nbytes for v in outputs.values())
    assert total <= 64 << 20, f"--dump-outputs: {total} bytes"
    for k, v in outputs.items():
        np.save(os.path.join(d, k + ".npy"), np.ascontiguousarray(v, dtype=np.float32))
    print(f"[bench] wrote {len(outputs)} arrays ({total / 1e6:.1f} MB) to {d}", file=sys.stderr, flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="per-GPU batch (BASELINE: 64)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also run the roofline / BatchNorm / exchange-timing passes, the other conv "
                         "arithmetic (alt_math) and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs to DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-overlap", action="store_true", help="disable the per-encoder stream pipeline (serialized kernels)")
    ap.add_argument("--no-alt", action="store_true", help="--full without the second measurement with the other conv arithmetic (N=1 only)")
    ap.add_argument("--no-unfused", action="store_true", help="--full without the extra serialized pass that times the un-fused BatchNorm reductions (profiling runs)")
    ap.add_argument("--math", choices=["f32", "split"], default=os.environ.get("MLA_CONV_MATH", "split"),
                    help="conv forward/dgrad arithmetic: f32 = exact fp32 MFMA; split = exact 3-way bf16 operand split, "
                         "6 bf16 MFMAs per fp32 product (fp32-equivalent accuracy, see DESIGN.md)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        if world == 1 and a.gpus > 1:
            sys.exit("bench.py --gpus N>1 must be launched with torch.distributed.run (one rank per GPU)")
        a.gpus = world
    import torch.distributed as dist
    ndev = max(torch.cuda.device_count(), 1)
    backend = os.environ.get("MLA_DIST_BACKEND", "nccl")      # "gloo": rehearse N ranks on a box with fewer GPUs than ranks
    if world > ndev and backend == "nccl":
        sys.exit(f"bench.py: {world} ranks but {ndev} GPU(s): RCCL needs one device per rank")
    torch.cuda.set_device(local_rank % ndev)
    dev = torch.device("cuda", local_rank % ndev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)    # RCCL over xGMI
        else:
            dist.init_process_group(backend)

    from mla_hip import AVClassifier, Comm, MLATrainer, ops

    model = AVClassifier(Args(), device=dev, seed=1234, conv_math=a.math)   # weight_init distributions (utils/utils.py:106-114)
    comm = Comm()
    for buf in (model.audio_net.flat, model.visual_net.flat, model.fusion_module.fc_out.flat):
        comm.broadcast_(buf, 0)                                 # replicas start identical (once, at init)
    trainer = MLATrainer(model, lr=1e-3, momentum=0.9, weight_decay=1e-4, gs_mode="as_intended", comm=comm)
    if a.no_overlap:
        trainer.set_overlap(False)

    B = a.batch
    g = torch.Generator(device=dev).manual_seed(1000 + rank)
    spec = torch.randn((B,) + SPEC_HW, device=dev, generator=g) * 4.4849 - 5.081     # SURVEY 8d synthetic stats
    image = torch.randn((B, 3, FRAMES) + IMG_HW, device=dev, generator=g)
    label = torch.randint(0, N_CLASSES, (B,), device=dev, generator=g)
    len_dl = 105                                                # CREMA-D: 6698 train clips / 64

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    for s in range(a.warmup):
        trainer.train_step(spec, image, label, s % len_dl, len_dl)
    sync()
    if rank == 0:
        print(f"[bench] warm-up done ({a.warmup} steps); timing {a.steps} steps", file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    for s in range(a.steps):
        trainer.train_step(spec, image, label, (a.warmup + s) % len_dl, len_dl)
    sync()
    dt = time.perf_counter() - t0
    if rank == 0:
        print(f"[bench] timed region {dt:.3f} s", file=sys.stderr, flush=True)
    loss = float(trainer.losses["loss"].item())
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, collect_outputs(trainer, model))
    overlapped = trainer.overlap_forward
    timer, timer_unfused, dt_serial, dist_diag = ops.KernelTimer(), ops.KernelTimer(), 0.0, None
    if a.full:
        # Roofline pass: the same K steps again with HIP events around every conv / BN call.  In the timed region the encoder
        # chains co-run on their own streams, so a launch's elapsed time there includes CU sharing; per-kernel durations are
        # therefore taken with the pipeline off (kernels serialized), immediately after the timed region, in this same process.
        trainer.set_overlap(False)
        trainer.train_step(spec, image, label, 0, len_dl)
        sync()
        ops.TIMER = timer
        t1 = time.perf_counter()
        for s in range(a.steps):
            trainer.train_step(spec, image, label, (a.warmup + s) % len_dl, len_dl)
        sync()
        dt_serial = time.perf_counter() - t1
        ops.TIMER = None
        # SURVEY 8d's un-fused BatchNorm accounting needs the time of the reduction passes that normally run inside the input-gradient
        # epilogues: measured here, in this run, by a second serialized event-instrumented pass with those fusions switched off
        # (every BatchNorm backward then runs its own reduce kernel; encoder.FUSE_BN_REDUCE is read at call time).
        from mla_hip import encoder as _enc
        if world == 1 and not a.no_unfused:
            _enc.FUSE_BN_REDUCE = False
            trainer.train_step(spec, image, label, 0, len_dl)
            sync()
            ops.TIMER = timer_unfused
            for s in range(a.steps):
                trainer.train_step(spec, image, label, (a.warmup + s) % len_dl, len_dl)
            sync()
            ops.TIMER = None
            _enc.FUSE_BN_REDUCE = True
        trainer.set_overlap(overlapped)
    per_rank_ms = [round(dt / a.steps * 1e3, 3)]
    if a.full and world > 1:
        # self-diagnosing multi-GPU record: a few more pipelined steps with HIP events around the packed head exchange (critical
        # path) and around the wait for each encoder's gradient all-reduce in front of its SGD, per rank
        trainer.dist_events = {}
        for s in range(min(a.steps, 10)):
            trainer.train_step(spec, image, label, (a.warmup + s) % len_dl, len_dl)
        sync()
        ev = trainer.dist_event_ms()
        trainer.dist_events = None
        mine2 = torch.tensor([ev.get("head_exchange", (0, 0.0))[1], ev.get("grad_wait", (0, 0.0))[1]], device=dev, dtype=torch.float64)
        all2 = [torch.zeros_like(mine2) for _ in range(world)]
        dist.all_gather(all2, mine2)
        dist_diag = {"head_exchange_ms_per_phase_per_rank": [round(float(x[0]), 4) for x in all2],
                     "encoder_grad_wait_ms_before_sgd_per_rank": [round(float(x[1]), 4) for x in all2],
                     "note": "HIP events on the stream each wait is enqueued on, pipelined steps after the timed region; the head exchange "
                             "(14 KB, own high-priority communicator) is on the step's critical path twice per step, the gradient wait "
                             "(44.7 MB per encoder in 16 MB buckets, issued right after that encoder's backward) only delays that encoder's SGD"}
    if world > 1:
        # MAX over ranks is the reported time; the per-rank values and the serialized (no stream pipeline) pass travel along so
        # that a first real multi-GPU run shows by itself whether a rank lags or the exchange serialises behind the backward
        mine = torch.tensor([dt, dt_serial], device=dev, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank_ms = [round(float(x[0]) / a.steps * 1e3, 3) for x in allr]
        dt = max(float(x[0]) for x in allr)
        dt_serial = max(float(x[1]) for x in allr)
    assert loss == loss, "loss is NaN"

    alt = None
    if a.full and world == 1 and not a.no_alt:
        # the same K steps with the other conv arithmetic (fresh model, same seeds / inputs), after the main measurement
        other = "split" if a.math == "f32" else "f32"
        m2 = AVClassifier(Args(), device=dev, seed=1234, conv_math=other)
        t2 = MLATrainer(m2, lr=1e-3, momentum=0.9, weight_decay=1e-4, gs_mode="as_intended", comm=comm)
        if a.no_overlap:
            t2.set_overlap(False)
        for s in range(a.warmup):
            t2.train_step(spec, image, label, s % len_dl, len_dl)
        sync()
        ta = time.perf_counter()
        for s in range(a.steps):
            t2.train_step(spec, image, label, (a.warmup + s) % len_dl, len_dl)
        sync()
        dta = time.perf_counter() - ta
        alt = {"conv_math": other, "value": round(B * a.steps / dta, 2), "unit": "samples/s",
               "ms_per_step": round(dta / a.steps * 1e3, 3), "final_loss": round(float(t2.losses["loss"].item()), 5)}
        del t2, m2
    if rank == 0:
        out = {
            "metric": "samples/sec per MLA alternating step, CREMA-D A+V bs=64",
            "value": round(B * world * a.steps / dt, 2), "unit": "samples/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "conv_math": a.math,
            "config": {"workload": "CREMA-D MLA step (--gs_flag, --lorb base ResNet18 audio+visual, GS projection as_intended), "
                                   "per-GPU batch %d: spec 1x1024x128 + frames 3x3x224x224, 6 classes" % B,
                       "global_batch": B * world, "parallelism": "dp%d" % world},
            "ranks": {"world_size": world, "backend": ("rccl" if backend == "nccl" else backend) if world > 1 else "none",
                      "collective_ranks": dist.get_world_size() if world > 1 else 1, "ms_per_step_per_rank": per_rank_ms,
                      "head_exchange": "packed dW|db|feature-sum|loss, one all-reduce per modality phase on its own communicator",
                      "encoder_gradients": "flat 44.7 MB buffer per encoder, 16 MB buckets, async all-reduce on RCCL's stream",
                      "exchange_timing": dist_diag},
            "final_loss": round(loss, 5),
        }
        if a.full:
            summ = timer.summary()
            ig = {"ms": 0.0, "ms_raw": 0.0, "work": 0.0, "launches": 0}
            for k in ("conv_fwd", "conv_dgrad"):                    # both are igemm_kernel launches
                for f in ig:
                    ig[f] += summ.get(k, {}).get(f, 0)
            achieved = ig["work"] / (ig["ms"] * 1e-3) / 1e12 if ig["ms"] > 0 else 0.0
            split = a.math == "split"
            peak = PEAK_SPLIT_TFLOPS if split else PEAK_F32_MFMA_TFLOPS
            kname = ("igemm_split_kernel + patch_split_kernel + patch64p_kernel (conv forward + input gradient of the 64..512-channel layers, 6 x "
                     "v_mfma_f32_32x32x16_bf16 per fp32 product; peak = bf16 MFMA rate / 6)") if split else \
                    "igemm_kernel (conv forward + input gradient, v_mfma_f32_32x32x2_f32)"
            traffic, traffic_src = None, None
            tpath = os.path.join(ROOT, "profiles", "r03_igemm_traffic.json")
            for older in ("r02_igemm_traffic.json", "r01f_igemm_traffic.json"):
                if not os.path.exists(tpath):
                    tpath = os.path.join(ROOT, "profiles", older)
            if os.path.exists(tpath):     # PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE) of this same command, per conv call
                tj = json.load(open(tpath))
                traffic = round(tj["split" if split else "f32"]["hbm_bytes_per_call"])
                traffic_src = "profiles/" + os.path.basename(tpath) + " (PMC counters cannot be read inside this process; measured by " \
                              "separate rocprofv3 --pmc passes over this same command): " + tj["method"] + "; " + tj["note"]
            per_kind = {k: {"launches_per_step": v["launches"] // a.steps, "ms_per_step": round(v["ms"] / a.steps, 3),
                            "tflops": round(v["work"] / (v["ms"] * 1e-3) / 1e12, 2)} for k, v in summ.items()
                        if k.startswith("conv") or k.startswith("stem")}      # stem_*: the persistent split-arithmetic stem kernels (stem_split.hip)
            # HBM family: BatchNorm forward / backward against 8 TB/s; `achieved` = algorithmic bytes / time
            # the fused flow needs (forward 8-12 B/elem: the statistics come out of the conv epilogue; backward 12 B/elem where the
            # reduction pass runs in the input-gradient epilogue, 20 B/elem otherwise; stem: the ReLU output and its gradient are never
            # materialised), `moved` = what these kernels really read + write.
            hbm = {"ms": 0.0, "work": 0.0, "moved": 0.0}
            for k in ("bn_fwd", "bn_bwd"):
                for f in hbm:
                    hbm[f] += summ.get(k, {}).get(f, 0.0)
                v = summ.get(k)
                if v and v["ms"] > 0:
                    per_kind[k] = {"launches_per_step": v["launches"] // a.steps, "ms_per_step": round(v["ms"] / a.steps, 3),
                                   "algorithmic_GBps": round(v["work"] / (v["ms"] * 1e-3) / 1e9, 1),
                                   "moved_GBps": round(v["moved"] / (v["ms"] * 1e-3) / 1e9, 1)}
            hbm_roof = None
            if hbm["ms"] > 0:
                ach = hbm["work"] / (hbm["ms"] * 1e-3) / 1e9
                hbm_roof = {"bound": "hbm", "kernels": "BatchNorm family (bn_finalize / bn_apply / bn_relu_maxpool_fwd / bn_reduce / bn_bwd_apply / bn_bwd_pooled; the reduction pass of 36 of the 40 backwards runs in the input-gradient epilogue and is not counted here, neither as bytes nor as time)",
                            "achieved": round(ach, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": round(ach / PEAK_HBM_GBPS, 4),
                            "moved_GBps": round(hbm["moved"] / (hbm["ms"] * 1e-3) / 1e9, 1),
                            "algorithmic_GB_per_step": round(hbm["work"] / a.steps / 1e9, 2), "ms_per_step": round(hbm["ms"] / a.steps, 3)}
                # SURVEY 8d's accounting of the same BatchNorm layers for the UN-fused algorithm (12 B/elem forward + 20 B/elem backward
                # over every conv output element) over the BatchNorm-family time MEASURED in this run with the epilogue reductions
                # switched off (second serialized pass above: every backward runs its own reduce kernel).  Not the `frac` above.
                su = timer_unfused.summary()
                t_unf = sum(su.get(k, {}).get("ms", 0.0) for k in ("bn_fwd", "bn_bwd")) / a.steps
                if t_unf > 0:
                    elems = 0
                    for enc in (model.audio_net, model.visual_net):
                        ws_e = enc._ws
                        elems += ws_e["y_stem"].numel() + sum(blk[k].numel() for blk in ws_e["blocks"] for k in ("y1", "y2", "yd") if k in blk)
                    survey_gb = 32.0 * elems / 1e9
                    hbm_roof["survey_8d_accounting"] = {"GB_per_step": round(survey_gb, 2), "ms_per_step_unfused_reductions_measured": round(t_unf, 3),
                                                        "GBps": round(survey_gb / (t_unf * 1e-3), 1),
                                                        "frac": round(survey_gb / (t_unf * 1e-3) / PEAK_HBM_GBPS, 4),
                                                        "stalled_brackets_replaced_by_median": sum(v.get("stalls", 0) for v in su.values())}
            conv_flop = sum(v["work"] for k, v in summ.items() if k.startswith("conv") or k.startswith("stem")) / a.steps
            t_min_ms = conv_flop / (peak * 1e12) * 1e3 + (hbm["work"] / a.steps) / (PEAK_HBM_GBPS * 1e9) * 1e3
            out.update({
                "roofline": {"bound": "mfma", "kernel": kname,
                             "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                             "frac": round(achieved / peak, 4), "frac_of_f32_mfma_peak": round(achieved / PEAK_F32_MFMA_TFLOPS, 4),
                             "traffic": traffic,
                             "avg_launch_ms": round(ig["ms"] / max(ig["launches"], 1), 4),
                             "avg_launch_ms_raw": round(ig["ms_raw"] / max(ig["launches"], 1), 4),
                             "stalled_brackets_replaced_by_median": sum(v.get("stalls", 0) for v in summ.values()),
                             "algorithmic_gflop_per_launch": round(ig["work"] / max(ig["launches"], 1) / 1e9, 2),
                             "measured": "HIP events around every conv launch over %d steps run right after the timed region "
                                         "with the stream pipeline off (serialized, event-instrumented: %.3f ms/step); in the timed "
                                         "region the encoder chains share the CUs" % (a.steps, dt_serial / a.steps * 1e3),
                             "traffic_source": traffic_src},
                "overlap": {"stream_pipeline": bool(overlapped), "ms_per_step_serialized_instrumented": round(dt_serial / a.steps * 1e3, 3),
                            "conv_tflops_in_timed_region": round(sum(v["work"] for k, v in summ.items() if k.startswith("conv") or k.startswith("stem")) / dt / 1e12, 2)},
                "roofline_hbm": hbm_roof,
                "step_vs_t_min": {"t_min_ms": round(t_min_ms, 2), "frac": round(t_min_ms / (dt / a.steps * 1e3), 4),
                                  "definition": "T_min = conv FLOPs / MFMA peak + BN bytes / HBM peak (SURVEY 8d)"},
                "kernels": per_kind,
            })
            if alt is not None:
                out["alt_math"] = alt
            if world == 1 and not a.no_cpu_baseline:
                # headline CPU figure: configs[0]'s batch 8 on all usable cores (~25 s); BASELINE.md section 4 also asks for the
                # batch-64 step and an 8-thread run (comparable with BASELINE.md's reference CPU figure, 7.0 samples/s at batch 8): bounded to
                # one warm-up + one / three steps each so that the whole baseline leg stays around a minute
                out["cpu_baseline"] = cpu_baseline()
                out["cpu_baseline"]["variants"] = [cpu_baseline(batch=8, max_steps=3, budget_s=8.0, threads=8),
                                                   cpu_baseline(batch=64, max_steps=1, budget_s=1.0)]
        print(json.dumps(out), flush=True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    sys.stdout.flush()
    sys.stderr.flush()


if __name__ == "__main__":
    main()
