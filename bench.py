#!/usr/bin/env python
"""bench.py — UNet denoising steps/sec on synthetic 12x256x256 clips (BASELINE.json metric).

A *step* = one classifier-free-guidance UNet forward for one clip (UNet batch 2 = [null-audio, audio]) +
guidance combine + scheduler update (DDIM-50 coefficients), i.e. one iteration of the loop at
pipeline_audio_cond_animation.py:330-365.  Workload = BASELINE.json configs[1] (AVSync15 shape: SD1.5-shaped
1.17 B-parameter AudioUNet3D, random-init weights, latents 12x32x32, audio guidance 4.0, bf16).
Inputs are resident in HBM before the timed region.  One process per GPU; clips are independent, so N GPUs
run N clips with no collective in the loop (weak scaling): RCCL is used once for the packed-weight broadcast
and once for the metric all-gather.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]   # N=1
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints ONE JSON line on rank 0 (metric, value, unit,
higher_is_better, dtype, ms_per_step = wall milliseconds of one timed step, ...).
--dump-outputs DIR writes rank 0's latents after the last timed step as DIR/latents.npy (float32); the weights
and inputs are seeded, so two builds run with the same arguments can be compared output for output.
--full adds the legs beyond the headline figure (each can still be switched off with its --no-* option):
  vae_decode    the SD1.5 VAE decoder on the denoised clip
  roofline      dominant kernel family = the bf16 MFMA GEMM/conv kernels: algorithmic FLOPs of all their
                launches in one step / their summed HIP-event durations (instrumented eager step)
  batched       --also-clips clips per forward and the {2, 4, 8} clips sweep (N=1 only)
  precise       the in-tolerance precision modes with their rel-L2 against the reference output (N=1 only)
  cpu_baseline  the oracle (oracle/unet_ref.py, fp32, torch CPU) timed on this box's host cores on the same
                CFG forward (rank 0, N=1 only)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

# ROCm runtime knob (must be set before HIP initialises): kernel arguments are written straight to device memory, which
# shortens every dispatch of the ~630-kernel graph a little (+0.5 % steps/s measured); honoured if the caller set it.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SD15 = dict(block_out_channels=(320, 640, 1280, 1280), attention_head_dim=8, norm_num_groups=32,
            cross_attention_dim=768, audio_cross_attention_dim=768, sample_size=32)
SD15_VAE = dict(in_channels=3, out_channels=3, latent_channels=4, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                norm_num_groups=32, scaling_factor=0.18215, act_fn="silu", sample_size=512)      # SD1.5 vae/config.json
ALGORITHMIC_TFLOP_PER_STEP = 5.427     # SURVEY.md §8(d), (2,12,32x32)
PEAK_BF16_TFLOPS = 2500.0              # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0
VAE_TFLOP_PER_CLIP = 7.47                # AutoencoderKL.decode of 12 x 256 x 256
VAE_GB_PER_CLIP = 6.4


def build_unet(device, rank, world, seed=0):
    """Rank 0 creates random-init weights on its GPU and packs them; the other ranks build the layout only
    (meta parameters) and receive the packed blob by one RCCL broadcast."""
    from asva_amd import dist as adist
    from asva_amd.unet import AudioUNet3DConditionModel

    if rank == 0:
        torch.manual_seed(seed)
        with torch.device(device):
            unet = AudioUNet3DConditionModel(**SD15).eval()
            # the reference zero-initialises its temporal paths; give them weights so no product is trivially 0
            with torch.no_grad():
                for n, p in unet.named_parameters():
                    if "conv_temp" in n or n.endswith("attn_temp.to_out.0.weight"):
                        p.normal_(0.0, 0.02)
        pk = unet.pack(device)
    else:
        with torch.device("meta"):
            unet = AudioUNet3DConditionModel(**SD15).eval()
        pk = unet.pack(device)
    adist.broadcast_blob(pk.blob, src=0)
    return unet


def synthetic_clip(device, seed, n=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    lat = torch.randn(n, 4, 12, 32, 32, generator=g)
    lat[:, :, 0] *= 0.18215                       # frame 0 = VAE image latent scale
    text = torch.randn(n, 77, 768, generator=g)
    audio = torch.randn(n, 229, 768, generator=g)
    null_audio = torch.randn(1, 229, 768, generator=g)
    return [t.to(device) for t in (lat, text, audio, null_audio)]


def build_id() -> str:
    """sha256 over the kernel library and the tile table that produced the timed kernels (first 16 hex digits): lets a
    PMC summary under profiles/ be tied to the build it was collected from."""
    import hashlib

    from asva_amd import _lib, ops

    h = hashlib.sha256()
    for path in (_lib.LIB_PATHS["bf16"], os.environ.get("AVSD_TILE_CACHE") or ops.DEFAULT_TILE_TABLE):
        if path and os.path.isfile(path):
            with open(path, "rb") as f:
                h.update(f.read())
    return h.hexdigest()[:16]


def spawn_ranks(n: int) -> int:
    """`python bench.py --gpus N` outside a launcher: re-executes itself as N ranks (one per GPU) under
    torch.distributed.run on 127.0.0.1, with the dmabuf IPC mode RCCL needs on this host driver."""
    import socket
    import subprocess

    from asva_amd import dist as adist

    if torch.cuda.device_count() < n and not adist.same_device():
        raise SystemExit(f"--gpus {n} but only {torch.cuda.device_count()} GPU(s) are visible "
                         "(tests: AVSD_DIST_SAME_DEVICE=1 AVSD_DIST_BACKEND=gloo run the ranks on one GPU)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    return subprocess.run(cmd, env=env).returncode


def vae_decode_leg(device, latents, reps=5):
    """VAE decode of the clip each rank just denoised (pipeline_audio_cond_animation.py:206-213, :368-370): SD1.5
    AutoencoderKL decoder, random-init weights, 12 x (4, 32, 32) latents -> 12 x (3, 256, 256), uint8 frames made on the
    device.  Algorithmic work per clip: 7.47 TFLOP, >= 6.4 GB of HBM traffic."""
    from asva_amd import dist as adist
    from asva_amd.vae import AutoencoderKL

    torch.manual_seed(1)
    with torch.device(device):
        vae = AutoencoderKL(**SD15_VAE).eval()
    vae.decode_to_uint8_frames(latents)          # warm-up: packs the weights
    torch.cuda.synchronize()
    adist.barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        vae.decode_to_uint8_frames(latents)
    torch.cuda.synchronize()
    adist.barrier()
    return time.perf_counter() - t0


def cpu_baseline(unet, clip):
    """Oracle (fp32 torch CPU restatement of the reference UNet) on the same CFG forward: 1 warm-up + 3 timed, median
    (BASELINE.md 4)."""
    from asva_amd.conditioning import audio_segment_mask
    from oracle.unet_ref import unet_forward

    # pick the thread count that is fastest on this host for a representative conv (many-core boxes are
    # slower with every hardware thread); `cores` reports the threads actually used
    import torch.nn.functional as F

    best, cores = None, 1
    xc, wc = torch.randn(24, 320, 32, 32), torch.randn(320, 320, 3, 3)
    for n in sorted({min(c, os.cpu_count() or 1) for c in (8, 16, 32, 64, 128)}):
        torch.set_num_threads(n)
        F.conv2d(xc, wc, padding=1)
        t0 = time.perf_counter()
        for _ in range(3):
            F.conv2d(xc, wc, padding=1)
        dt = time.perf_counter() - t0
        if best is None or dt < best:
            best, cores = dt, n
    torch.set_num_threads(cores)
    sd = {k: v.detach().float().cpu() for k, v in unet.state_dict().items()}
    lat, text, audio, null_audio = [t.float().cpu()[:1] for t in clip]
    x = torch.cat([lat, lat])
    txt = torch.cat([text, text])[:, None].expand(2, 12, 77, 768)
    aud = torch.cat([null_audio, audio])[:, None].expand(2, 12, 229, 768)
    mask = audio_segment_mask(12)[None].expand(2, -1, -1)
    cfg = dict(unet.config)
    times = []
    with torch.no_grad():
        for _ in range(4):
            t0 = time.perf_counter()
            unet_forward(sd, cfg, x, 981, txt, aud, mask)
            times.append(time.perf_counter() - t0)
    med = sorted(times[1:])[1]
    return {"value": 1.0 / med, "unit": "steps/s", "cores": cores, "host_cores": os.cpu_count(), "kind": "port",
            "sample": "oracle/unet_ref.py fp32 torch-CPU CFG UNet forward (B=2x12x32x32), 1 warm-up + 3 timed, median",
            "seconds_per_step": med, "seconds_all": [round(t, 3) for t in times[1:]]}


def precise_rel_l2(device):
    """rel-L2 of ONE CFG forward in the current precision mode against the REFERENCE's fp32 output at BASELINE cfg-2 shape:
    tests/golden/unet_sd15_forward.pt holds the output of the reference's own AudioUNet3DConditionModel (imported from
    /root/reference by oracle/gen_golden.py) with the closed-form filler weights; the same weights are rebuilt here by
    asva_amd/filler.py (no weight file travels).  This is the number north_star's 1e-3 is about, measured inside the bench run."""
    from asva_amd.conditioning import audio_segment_mask
    from asva_amd.filler import fill_module_, seeded_randn
    from asva_amd.unet import AudioUNet3DConditionModel

    gdir = os.path.join(ROOT, "tests", "golden")
    g = torch.load(os.path.join(gdir, "unet_sd15_forward.pt"), map_location="cpu", weights_only=True)
    with open(os.path.join(gdir, "unet_sd15_config.json")) as f:
        cfg = json.load(f)
    m = AudioUNet3DConditionModel.from_config(cfg).eval()
    fill_module_(m)
    m = m.to(device)
    lat = seeded_randn(1, 1, 4, 12, 32, 32)                  # the inputs the fixture was generated with (oracle/gen_golden.py)
    x = torch.cat([lat, lat]).to(device)
    text = seeded_randn(2, 1, 77, 768).expand(2, 77, 768).to(device)
    audio = torch.cat([seeded_randn(4, 1, 229, 768), seeded_randn(3, 1, 229, 768)]).to(device)
    with torch.no_grad():
        out = m(x, g["timestep"], text, audio, audio_attention_mask=audio_segment_mask(12)).sample
    ref = g["full32"].float()
    err = ((out.float().cpu() - ref).norm() / ref.norm()).item()
    del m
    torch.cuda.empty_cache()
    return err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay")
    ap.add_argument("--save-tiles", default="", help="write the autotuned tile table here (reload with AVSD_TILE_CACHE=<file>)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write the latents of the last step (rank 0) as DIR/latents.npy, float32")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beyond the headline figure: VAE decode, roofline, batched clips, precision modes, "
                         "CPU baseline (the --no-* options below switch single legs off again)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-vae", action="store_true", help="skip the VAE-decode leg")
    ap.add_argument("--no-precise", action="store_true", help="skip the split-precision leg")
    ap.add_argument("--also-clips", type=int, default=4,
                    help="with --full, after the headline measurement, also time this many clips batched into one forward per GPU "
                         "(BASELINE cfg 3 runs 4 per GPU); 0 = skip")
    ap.add_argument("--fp8-attention", action="store_true",
                    help="BASELINE cfg 5: e4m3 Q/K/V in the first-frame and cross attentions (f32 softmax / accumulation)")
    ap.add_argument("--f32-residual", action="store_true", help="keep the residual stream in f32 (precision mode; slower)")
    ap.add_argument("--clips-per-gpu", type=int, default=1,
                    help="independent clips batched into one UNet forward per GPU (BASELINE cfg 3 uses 4); "
                         "the default 1 is BASELINE cfg 2 / the reference's one-clip-per-call")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not a.full:
        # a plain run measures the headline figure only
        a.no_vae = a.no_roofline = a.no_precise = a.no_cpu_baseline = True
        a.also_clips = 0

    from asva_amd import dist as adist
    from asva_amd import ops
    from asva_amd.conditioning import audio_segment_mask
    from asva_amd.engine import DenoiseEngine
    from asva_amd.schedulers import DDIMScheduler

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(a.gpus))         # one process per GPU; rank 0 of the child job prints the JSON line
    rank, local_rank, world = adist.env_rank_world()
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but the launcher started WORLD_SIZE={world} ranks")
    try:
        dev_index = adist.device_index(local_rank)
    except RuntimeError as e:
        raise SystemExit(str(e))
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    adist.init_process_group(adist.backend_name("nccl"))
    import torch.distributed as tdist

    world_observed = tdist.get_world_size() if tdist.is_initialized() else 1
    if world_observed != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but the RCCL communicator has {world_observed} ranks")

    unet = build_unet(device, rank, world)
    unet.fp8_attention = a.fp8_attention
    unet.f32_residual = a.f32_residual
    cpg = a.clips_per_gpu
    clip = synthetic_clip(device, seed=adist.clip_seed(rank), n=cpg)      # clip id = rank: inputs are seeded by clip, not by rank
    lat, text, audio, null_audio = clip
    sched = DDIMScheduler()
    eng = DenoiseEngine(unet, sched, audio_guidance_scale=4.0, use_graph=not a.no_graph)
    # self-validation of a multi-GPU run: EVERY rank first computes step 0 of clip id 0 (the witness clip) on the weights it
    # received by broadcast; the bit checksums travel in the metrics row and rank 0 requires them to be identical
    w_lat, w_text, w_audio, w_null = synthetic_clip(device, seed=adist.clip_seed(0), n=cpg)
    eng.set_conditioning(w_text, w_audio, w_null, audio_segment_mask(12), 12)
    eng.prepare(w_lat, 50)
    eng.step(w_lat, 0)
    torch.cuda.synchronize()
    witness = adist.bit_checksum(w_lat)
    del w_text, w_audio, w_null
    eng.set_conditioning(text, audio, null_audio, audio_segment_mask(12), 12)   # same geometry: refreshed in place, the graph stays
    latents = lat.clone()
    n_sched = 50
    eng.prepare(latents, n_sched)

    for i in range(a.warmup):
        eng.step(latents, i % n_sched)
    torch.cuda.synchronize()
    adist.barrier()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for i in range(a.steps):
        eng.step(latents, (a.warmup + i) % n_sched)
    ev1.record()
    torch.cuda.synchronize()
    adist.barrier()
    wall = time.perf_counter() - t0
    gpu_ms = ev0.elapsed_time(ev1)
    finite = bool(torch.isfinite(latents).all())
    if a.dump_outputs and rank == 0:
        # what a caller of the timed path receives: the latents, updated in place by the last step ((clips, 4, 12, 32, 32), 0.2 MB a clip)
        import numpy as np

        os.makedirs(a.dump_outputs, exist_ok=True)
        np.save(os.path.join(a.dump_outputs, "latents.npy"), latents.detach().float().cpu().numpy())

    vae_wall, vae_reps = 0.0, 5
    if not a.no_vae:
        vae_wall = vae_decode_leg(device, latents, vae_reps)
    rows = adist.gather_metrics([wall, gpu_ms, float(a.steps * cpg), float(finite), vae_wall, witness], device=device)
    if rank != 0:
        return
    if len({r[5] for r in rows}) != 1:
        raise SystemExit(f"ranks disagree on step 0 of the witness clip (bit checksums {[r[5] for r in rows]}): "
                         "the weight broadcast or a kernel is not deterministic across GPUs")
    per_rank = [r[2] / r[0] for r in rows]
    max_wall = max(r[0] for r in rows)
    total_steps = sum(r[2] for r in rows)
    value = total_steps / max_wall
    ms_per_step = max_wall / a.steps * 1e3
    out = {
        "metric": "UNet denoising steps/sec, 12x256x256 bf16, CFG on",
        "value": round(value, 3), "unit": "steps/s", "n_gpus": world, "world_size": world_observed,
        "dist_backend": (tdist.get_backend() if tdist.is_initialized() else None), "ranks_share_one_gpu": bool(adist.same_device() and world > 1),
        "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16" + (" (fp8 e4m3 attention Q/K/V)" if a.fp8_attention else "") + (" + f32 residual stream" if a.f32_residual else ""),
        "data": "synthetic",
        "config": {"workload": f"BASELINE configs[1]: AVSync15 shape, {cpg} clip(s) per GPU per forward, 12x256x256 (latent 12x32x32), "
                               "SD1.5-shaped AudioUNet3D 1.17B params random-init, CFG batch 2 (audio guidance 4.0), "
                               "DDIM-50 schedule, step = UNet forward + guidance + scheduler update",
                   "clips_per_gpu": cpg, "unet_batch": 2 * cpg, "frames": 12, "latent_hw": [32, 32],
                   "launch": "eager" if a.no_graph else "hipGraph replay", "parallelism": f"dp{world} (independent clips)"},
        "gpu_ms_per_step_rank0": round(rows[0][1] / a.steps, 4),
        "per_rank_steps_per_s": [round(v, 3) for v in per_rank], "per_rank_min_max": [round(min(per_rank), 3), round(max(per_rank), 3)],
        "ranks_agree_on_witness_clip": True, "witness_checksum": int(rows[0][5]),
        "all_finite": all(r[3] == 1.0 for r in rows),
        "step_tflops": round(ALGORITHMIC_TFLOP_PER_STEP * cpg / (ms_per_step * 1e-3), 2),
        "step_mfma_frac": round(ALGORITHMIC_TFLOP_PER_STEP * cpg / (ms_per_step * 1e-3) / PEAK_BF16_TFLOPS, 4),
        "build_id": build_id(),
    }
    if not a.no_vae:
        vmax = max(r[4] for r in rows)
        per_clip = vmax / (vae_reps * cpg)
        out["vae_decode"] = {"clips_per_s": round(world * vae_reps * cpg / vmax, 2), "ms_per_clip": round(per_clip * 1e3, 3),
                             "tflops": round(VAE_TFLOP_PER_CLIP / per_clip, 1), "gbs": round(VAE_GB_PER_CLIP / per_clip, 1),
                             "frac_mfma": round(VAE_TFLOP_PER_CLIP / per_clip / PEAK_BF16_TFLOPS, 4),
                             "frac_hbm": round(VAE_GB_PER_CLIP / per_clip / PEAK_HBM_GBS, 4),
                             "workload": f"SD1.5 AutoencoderKL decoder, {12 * cpg} x (4,32,32) latents -> uint8 256x256 frames, "
                                         f"{vae_reps} reps, random-init weights; 7.47 TFLOP and >= 6.4 GB per 12-frame clip (SURVEY 8d)"}

    def roofline_of(latents_, clips, model=None, n_branch=2):
        """instrumented eager forward (one forward = `clips` steps) -> (roofline dict of the GEMM family, per-family table).
        Every family's time is the GPU time of its launches of that forward re-issued back to back from ONE captured graph —
        the clock of a rocprofv3 trace of the graph-replayed step; the per-launch event pairs of the eager pass (each carries
        ~4 us of command-processor time) are kept beside it as `ms_event_pairs`.
        `achieved` = ALGORITHMIC flops (2 M N K of every product as the reference states it — the upsample convolutions at
        their 3x3 taps on the upsampled image, a three-pass product of the precision plan once) / time; `achieved_executed` counts the
        multiply-adds the launches execute at one pass per product (the sub-pixel form of the upsample convolutions runs 4 of the 9
        taps: 0.23 TFLOP per step fewer), `achieved_mfma_issued` every MFMA pass issued (three-pass products x 3)."""
        timer = ops.KernelTimer()
        ops.set_timer(timer)
        (model or unet).denoise_forward(latents_, torch.full((1,), 501.0, device=device), rep=n_branch)
        ops.set_timer(None)
        fam = timer.summary()
        gemm_fams = tuple(k for k in ("gemm_plain", "gemm_tmix", "gemm_conv3") if k in fam)
        mm = [fam[k] for k in gemm_fams]
        ms_events = sum(f["ms"] for f in mm)
        fl_issued = sum(f["flops"] for f in mm)
        fl_ref = sum(f["flops_ref"] for f in mm)
        fl = sum(f.get("flops_once", f["flops"]) for f in mm)
        launches = sum(f["launches"] for f in mm)
        fam_ms = {k: (timer.replay_ms((k,)) if not a.no_graph else v["ms"]) for k, v in fam.items()}
        ms = timer.replay_ms(gemm_fams) if not a.no_graph else ms_events
        ach = fl_ref / (ms * 1e-3) / 1e12
        roof = {"bound": "mfma", "kernel": "GEMM family: gemm4_kernel (hand-scheduled tiles) / gemm2_kernel<BM,BN,...,MODE> (linear / temporal-mix / strided and sub-pixel-upsample conv3x3 implicit GEMM) + conv3r_kernel (conv3x3, input tile resident in LDS) + nstream_kernel (GEGLU projections, A band resident), split-K reduce launches included",
                "achieved": round(ach, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_BF16_TFLOPS, 4),
                "achieved_executed": round(fl / (ms * 1e-3) / 1e12, 2), "frac_executed": round(fl / (ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                "achieved_mfma_issued": round(fl_issued / (ms * 1e-3) / 1e12, 2), "frac_mfma_issued": round(fl_issued / (ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                "traffic": None, "launches_per_step": launches // clips, "clips_per_forward": clips, "ms_per_step": round(ms / clips, 4),
                "ms_per_forward": round(ms, 4), "ms_per_step_event_pairs": round(ms_events / clips, 4),
                "family_ms_sum": round(sum(fam_ms[k] for k in gemm_fams) / clips, 4),
                "avg_launch_us": round(ms * 1e3 / launches, 2), "tflop_per_step": round(fl_ref / clips / 1e12, 4),
                "tflop_per_step_executed": round(fl / clips / 1e12, 4), "tflop_per_step_mfma_issued": round(fl_issued / clips / 1e12, 4),
                "algorithmic_bytes_per_launch": round(sum(f["bytes"] for f in mm) / launches)}
        table = {k: {"launches": v["launches"], "ms": round(fam_ms[k], 4), "ms_event_pairs": round(v["ms"], 4),
                     "tflops": round(v["flops"] / (fam_ms[k] * 1e-3) / 1e12, 2) if v["flops"] else None,
                     "gbs": round(v["bytes"] / (fam_ms[k] * 1e-3) / 1e9, 1)} for k, v in fam.items()}
        return roof, table

    if not a.no_roofline:
        out["roofline"], out["kernel_families"] = roofline_of(latents, cpg)
        # HBM-side traffic of the same family from rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE collected in separate
        # runs of this script, FETCH_SIZE doubled per the gfx950 correction); counters cannot be read from inside
        # the timed process, so the committed summary of the last profiled run is reported, with its provenance
        tpath = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "pmc_traffic.json")
        if os.path.isfile(tpath):
            with open(tpath) as f:
                tr = json.load(f)
            out["roofline"]["traffic"] = tr["hbm_bytes_per_launch"]
            out["roofline"]["traffic_detail"] = {k: tr[k] for k in ("fetch_bytes_x2_per_launch", "write_bytes_per_launch",
                                                                    "launches_profiled", "source", "build_id") if k in tr}
            # the counters were collected from the build whose id the summary carries; say so when this run's differs
            out["roofline"]["traffic_from_this_build"] = tr.get("build_id") == out["build_id"]

    if a.also_clips and a.also_clips != cpg and world == 1:
        # Several independent clips in one forward (UNet batch 2 x clips; BASELINE cfg 3 runs 4 per GPU) — same kernels, more rows
        # per launch; reported next to the headline, never instead of it.  `batched` = the --also-clips count with its own GEMM
        # roofline; `clips_sweep` = {2, 4, 8} clips per forward, the measured approach to north_star's >= 0.40 MFMA fraction.
        def batched_leg(n, with_roofline):
            lat_b, text_b, audio_b, null_b = synthetic_clip(device, seed=2000, n=n)
            eng_b = DenoiseEngine(unet, DDIMScheduler(), audio_guidance_scale=4.0, use_graph=not a.no_graph)
            eng_b.set_conditioning(text_b, audio_b, null_b, audio_segment_mask(12), 12)
            lb = lat_b.clone()
            eng_b.prepare(lb, n_sched)
            ks = max(10, a.steps // max(2, n // 2))
            for i in range(3):
                eng_b.step(lb, i)
            torch.cuda.synchronize()
            tb = time.perf_counter()
            for i in range(ks):
                eng_b.step(lb, (3 + i) % n_sched)
            torch.cuda.synchronize()
            tb = time.perf_counter() - tb
            row = {"clips_per_gpu": n, "unet_batch": 2 * n, "value": round(ks * n / tb, 3), "unit": "steps/s",
                   "ms_per_forward": round(tb / ks * 1e3, 4), "steps": ks,
                   "step_mfma_frac": round(ALGORITHMIC_TFLOP_PER_STEP * n / (tb / ks) / PEAK_BF16_TFLOPS, 4)}
            if with_roofline and not a.no_roofline:
                row["roofline"], _ = roofline_of(lb, n)
            del eng_b
            torch.cuda.empty_cache()
            return row

        out["batched"] = batched_leg(a.also_clips, True)
        out["batched"]["workload"] = f"BASELINE configs[2] per-GPU shape: {a.also_clips} clips per forward"
        out["clips_sweep"] = [{"clips_per_gpu": cpg, "value": out["value"], "step_mfma_frac": out["step_mfma_frac"]}]
        for n in (2, 4, 8):
            if n == cpg:
                continue
            r = out["batched"] if n == a.also_clips else batched_leg(n, False)
            out["clips_sweep"].append({k: r[k] for k in ("clips_per_gpu", "value", "ms_per_forward", "step_mfma_frac")})
    if world == 1 and not a.no_precise:
        # The modes that meet BASELINE.json's stated tolerance (<= 1e-3 rel-L2 vs the reference's fp32 output), same clip, same step
        # definition, reported beside the bf16 headline, never instead of it:
        #   precise        the per-layer precision plan (asva_amd/precision_plan.json): fp16 storage + f32 residual stream on the fast
        #                  one-pass kernels, three-pass split products only where the error budget needs them
        #   precise_split  every tensor two bf16 planes, every product three MFMA passes (round 3's mode): 40x inside the tolerance
        from asva_amd import precision as P

        def precise_leg(enter, leave, mode, passes, roofline=False, mode_id=""):
            enter()
            try:
                unet._invalidate()
                eng_p = DenoiseEngine(unet, DDIMScheduler(), audio_guidance_scale=4.0, use_graph=not a.no_graph)
                eng_p.set_conditioning(text[:1], audio[:1], null_audio, audio_segment_mask(12), 12)
                lp = lat[:1].clone()
                eng_p.prepare(lp, n_sched)
                kp = max(10, a.steps // 4)
                for i in range(3):
                    eng_p.step(lp, i)
                torch.cuda.synchronize()
                tp = time.perf_counter()
                for i in range(kp):
                    eng_p.step(lp, (3 + i) % n_sched)
                torch.cuda.synchronize()
                tp = time.perf_counter() - tp
                rel = precise_rel_l2(device)
                row = {"mode_id": mode_id, "mode": mode, "value": round(kp / tp, 3), "unit": "steps/s", "ms_per_step": round(tp / kp * 1e3, 4), "steps": kp,
                       "all_finite": bool(torch.isfinite(lp).all()),
                       "rel_l2": rel, "rel_l2_tolerance": 1e-3, "rel_l2_ok": bool(rel < 1e-3),
                       "rel_l2_of": "one CFG forward (2,4,12,32,32), filler weights, vs the REFERENCE's fp32 output "
                                    "(tests/golden/unet_sd15_forward.pt), measured in this run"}
                if passes:
                    row["mfma_frac_of_3x_work"] = round(passes * ALGORITHMIC_TFLOP_PER_STEP / (tp / kp) / PEAK_BF16_TFLOPS, 4)
                row["step_tflops"] = round(ALGORITHMIC_TFLOP_PER_STEP / (tp / kp), 2)
                row["step_mfma_frac"] = round(ALGORITHMIC_TFLOP_PER_STEP / (tp / kp) / PEAK_BF16_TFLOPS, 4)
                if roofline and not a.no_roofline:
                    # the same instrumented forward as the headline's, in THIS mode (graph-replay clock per family)
                    row["roofline"], row["kernel_families"] = roofline_of(lp, 1)
                del eng_p
                return row
            finally:
                leave()
                unet._invalidate()
                torch.cuda.empty_cache()

        # (`precise` has been the per-layer plan since round 5 — rounds 3-4 printed split precision under that key; `mode_id` says which)
        out["precise"] = precise_leg(lambda: P.set_plan(True), lambda: P.set_plan(False),
                                     "per-layer precision plan: fp16 storage + f32 residual stream, three-pass split products for "
                                     + ", ".join(sorted(json.load(open(P.PLAN_PATH))["three_pass"])), 0, roofline=True, mode_id="plan")
        if not out["precise"]["rel_l2_ok"]:
            out["precise"]["note"] = "OUTSIDE the stated tolerance: not a valid in-tolerance throughput number"
        out["precise_split"] = precise_leg(lambda: P.set_split(True), lambda: P.set_split(False),
                                           "bf16x2 split precision (main + rest planes, 3-pass MFMA)", 3, mode_id="split")
    if world == 1 and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(unet, clip)
        out["gpu_over_cpu"] = round(value / out["cpu_baseline"]["value"], 1)
    if a.save_tiles:
        ops.save_tile_cache(a.save_tiles)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    try:
        main()
    finally:
        import torch.distributed as _d

        if _d.is_available() and _d.is_initialized():
            _d.destroy_process_group()
