"""End-to-end clip generation on one MI355X with the reference's schedule (PNDM, num_inference_steps=50 -> 51 UNet
forwards, audio guidance 4.0) through AudioCondAnimationPipeline: SD1.5-shaped UNet + SD1.5 VAE decoder, random
weights, synthetic conditioning.  Reports per-clip latency split into denoising and VAE decode.

    python tools/clip_bench.py                                     # PNDM-50, the reference's schedule
    python tools/clip_bench.py --scheduler dpmsolver++ --steps 20  # DPM-Solver++ (2M), 20 UNet forwards
    python tools/clip_bench.py --scheduler unipc --steps 10        # UniPC (order 2, bh2), 10 UNet forwards
    python tools/clip_bench.py --scheduler sde-dpmsolver++ --steps 20   # SDE-DPM-Solver++ (2M): the step kernel draws its noise
    python tools/clip_bench.py --scheduler ddim --eta 1.0 --steps 50    # DDIM with eta > 0, likewise
    python tools/clip_bench.py --scheduler sde-dpmsolver++ --steps 20 --unfused-noise
                                  # the yardstick of profiles/stochastic.md: the same step as avsd_randn_philox_f32 + the
                                  # deterministic kernel + an add (three launches and a noise buffer instead of one launch)"""
import argparse, sys, os, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from asva_amd.pipeline import AudioCondAnimationPipeline, synthetic_clip
from asva_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler, SDEDPMSolverMultistepScheduler,
                                 UniPCMultistepScheduler)
from asva_amd.vae import AutoencoderKL
from asva_amd.conditioning import audio_segment_mask

ap = argparse.ArgumentParser()
ap.add_argument("--scheduler", choices=("pndm", "ddim", "dpmsolver++", "sde-dpmsolver++", "unipc"), default="pndm")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--eta", type=float, default=0.0, help="DDIM's eta (the other schedulers have none)")
ap.add_argument("--unfused-noise", action="store_true", help="stochastic steps as randn_philox + deterministic kernel + add")
args = ap.parse_args()
sched = {"pndm": PNDMScheduler, "ddim": DDIMScheduler, "dpmsolver++": DPMSolverMultistepScheduler,
         "sde-dpmsolver++": SDEDPMSolverMultistepScheduler,
         "unipc": UniPCMultistepScheduler}[args.scheduler]()
if args.eta and args.scheduler != "ddim":
    ap.error("--eta needs --scheduler ddim")
sched.set_timesteps(args.steps)
n_fwd = sched.num_forwards()
label = {"pndm": "PNDM", "ddim": "DDIM" + (f" eta {args.eta:g}" if args.eta else ""), "dpmsolver++": "DPM++ 2M",
         "sde-dpmsolver++": "SDE-DPM++ 2M", "unipc": "UniPC-2"}[args.scheduler]

if args.unfused_noise:
    from asva_amd import ops

    def unfused(det):
        def step(noise_pred, n_branch, g, x_in, x_out, *coef, c_noise=0.0, seed=0, stream=0, step=0, **kw):
            B, C, F, H, W = x_in.shape
            z = torch.stack([ops.randn_philox(C * (F - 1) * H * W, seed, stream + b, step).view(C, F - 1, H, W) for b in range(B)])
            det(noise_pred, n_branch, g, x_in, x_out, *coef, **kw)
            x_out[:, :, 1:].add_(z, alpha=c_noise)
        return step

    ops.guided_step_sde, ops.guided_multistep_sde = unfused(ops.guided_step), unfused(ops.guided_multistep)
    label += " (unfused noise)"

dev = torch.device("cuda", 0)
unet = bench.build_unet(dev, 0, 1)
with torch.device(dev):
    vae = AutoencoderKL().eval()
pipe = AudioCondAnimationPipeline(unet=unet, scheduler=sched, vae=vae).to(dev)
pipe.set_progress_bar_config(disable=True)

def run(seed):
    c = synthetic_clip(seed, device=dev)
    kw = dict(texts=[""], text_encodings=[c["text_encodings"][None]], image_latents=c["image_latents"][None], noise=c["noise"][None],
              audio_encodings=c["audio_encodings"][None], null_audio_encodings=c["null_audio_encodings"][None],
              audio_masks=audio_segment_mask(12), num_inference_steps=args.steps, audio_guidance_scale=4.0, eta=args.eta,
              generator=torch.Generator(device=dev).manual_seed(seed))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    lat = pipe(**kw, output_latents=True)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    vid = pipe.decode_latents(lat.permute(0, 2, 1, 3, 4).reshape(12, 4, 32, 32))
    torch.cuda.synchronize(); t2 = time.perf_counter()
    return t1 - t0, t2 - t1, vid

run(0)                        # autotune + graph capture
res = [run(s)[:2] for s in (1, 2, 3)]
den = sum(r[0] for r in res) / 3; dec = sum(r[1] for r in res) / 3
# device-only VAE time (decode_latents above includes the 9.4 MB device->host copy of the frames)
z = torch.randn(12, 4, 32, 32, device=dev)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(5): vae.decode(z, postprocess=True)
torch.cuda.synchronize(); vdev = (time.perf_counter() - t0) / 5
print(json.dumps({"clip": f"12x256x256, {label}-{args.steps} ({n_fwd} UNet CFG forwards), audio guidance 4.0", "denoise_s": round(den, 4),
                  "decode_incl_d2h_s": round(dec, 4), "vae_decode_device_s": round(vdev, 4), "vae_tflops": round(7.47 / vdev, 1),
                  "clips_per_s": round(1 / (den + dec), 3), "unet_steps_per_s": round(n_fwd / den, 2)}))
