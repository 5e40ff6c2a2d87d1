"""Does a storage mode cost audio-video synchronisation?  Generates the same synthetic clips in two modes and scores both with the
AVSync classifier (asva_amd/avsync.py): raw scores, and RelSync of the first mode with the second as the reference video.

    python tools/avsync_score.py --model checkpoints/avsync/.../modules      # a trained classifier (load_avsync_model layout)
    python tools/avsync_score.py --clips 4 --modes bf16 plan --steps 20      # the defaults; modes: bf16 fp16 split plan

Without --model the classifier gets seeded random weights and the numbers mean nothing: the run then only shows that the path works
and what it costs.  The UNet and VAE are the SD1.5-shaped random-weight models of tools/clip_bench.py (DPM-Solver++ 2M sampling;
--scheduler unipc: UniPC-2)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from asva_amd import avsync, precision  # noqa: E402
from asva_amd.audio_features import waveform_to_melspectrogram  # noqa: E402
from asva_amd.conditioning import audio_segment_mask  # noqa: E402
from asva_amd.pipeline import AudioCondAnimationPipeline, synthetic_clip  # noqa: E402
from asva_amd.schedulers import DPMSolverMultistepScheduler, UniPCMultistepScheduler  # noqa: E402
from asva_amd.vae import AutoencoderKL  # noqa: E402

MODES = {"bf16": lambda: precision.set_precision("bf16"), "fp16": lambda: precision.set_precision("fp16"),
         "split": lambda: precision.set_split(True), "plan": lambda: precision.set_plan(True)}


def reset_mode():
    precision.set_plan(False)
    precision.set_split(False)
    precision.set_precision("bf16")


def seeded_classifier(seed):
    """random weights that let the input through to the score (default initialisation does not: its biases decide the score)"""
    net = avsync.AVSyncClassifier(avsync.AudioConv2DNet(), avsync.VideoR2Plus1DNet(), avsync.FCHead()).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in net.state_dict().items():
            if name.endswith("num_batches_tracked"):
                continue
            if t.dim() >= 2:
                t.copy_(torch.randn(t.shape, generator=g) * ((1.0 if t.dim() == 2 else 2.0) / t[0].numel()) ** 0.5)
            elif name.endswith(("running_var", "weight")):
                t.copy_(0.5 + (1.0 if name.endswith("running_var") else 0.5) * torch.rand(t.shape, generator=g))
            else:
                t.copy_(0.1 * torch.randn(t.shape, generator=g))
    return net


def waveform(seed):
    """2 s at 16 kHz: a few amplitude-modulated tones (the synthetic clips carry audio encodings, not a waveform)"""
    g = torch.Generator().manual_seed(1000 + seed)
    t = torch.arange(32000, dtype=torch.float32) / 16000.0
    f, m = 200.0 + 2000.0 * torch.rand(4, generator=g), 1.0 + 5.0 * torch.rand(4, generator=g)
    return (0.1 * torch.sin(2 * torch.pi * f[:, None] * t) * (1.0 + torch.sin(2 * torch.pi * m[:, None] * t))).sum(0, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--modes", nargs=2, default=["bf16", "plan"], choices=sorted(MODES))
    ap.add_argument("--model", default=None, help="directory with audio_encoder/ video_encoder/ head/ of a trained AVSync classifier")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--scheduler", choices=("dpmsolver++", "unipc"), default="dpmsolver++")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)

    videos = {}
    for mode in args.modes:
        reset_mode()
        MODES[mode]()
        unet = bench.build_unet(dev, 0, 1)                       # the same seed, so the same weights, in every mode
        with torch.device(dev):
            vae = AutoencoderKL().eval()
        sched = UniPCMultistepScheduler() if args.scheduler == "unipc" else DPMSolverMultistepScheduler()
        pipe = AudioCondAnimationPipeline(unet=unet, scheduler=sched, vae=vae).to(dev)
        pipe.set_progress_bar_config(disable=True)
        out = []
        for s in range(args.clips):
            c = synthetic_clip(args.seed + s, device=dev)
            lat = pipe(texts=[""], text_encodings=[c["text_encodings"][None]], image_latents=c["image_latents"][None], noise=c["noise"][None],
                       audio_encodings=c["audio_encodings"][None], null_audio_encodings=c["null_audio_encodings"][None],
                       audio_masks=audio_segment_mask(12), num_inference_steps=args.steps, audio_guidance_scale=4.0, output_latents=True)
            frames = pipe.decode_latents(lat.permute(0, 2, 1, 3, 4).reshape(12, 4, 32, 32))          # (12, 3, 256, 256) in [0, 1], CPU
            out.append(frames.permute(1, 0, 2, 3))
        videos[mode] = torch.stack(out)                                                                # (clips, 3, 12, 256, 256)
        del pipe, unet, vae
        torch.cuda.empty_cache()
    reset_mode()

    if args.model:
        net = avsync.load_avsync_model(args.model).to(dev)
    else:
        print("WARNING: no --model given: the classifier has seeded random weights and the numbers below mean nothing")
        net = seeded_classifier(args.seed).to(dev)
    audios = torch.stack([waveform_to_melspectrogram(waveform(args.seed + s), device=dev) for s in range(args.clips)])     # (clips, 1, 128, 204)
    a, b = args.modes
    va, vb = videos[a].to(dev), videos[b].to(dev)
    net(audios[:1], avsync.preprocess_videos(va[:1]))                                                   # pack + warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sa = avsync.compute_avsync_scores(audios, va, net)
    sb = avsync.compute_avsync_scores(audios, vb, net)
    rel = avsync.compute_relsync(audios, va, net, ref_videos=vb)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"clip | score {a} | score {b} | RelSync of {a} against {b} (0.5 = the classifier cannot tell them apart)")
    for i in range(args.clips):
        print(f"{i:4d} | {sa[i].item():+.6f} | {sb[i].item():+.6f} | {rel[i].item():.6f}")
    print(f"mean RelSync {rel.mean().item():.6f}; scorer time {1e3 * dt / args.clips:.2f} ms per clip "
          f"(two raw scores + RelSync = four video passes, three audio passes)")


if __name__ == "__main__":
    main()
