"""Animate one still over a whole audio track (AudioCondAnimationPipeline.animate_track through generate_track): chained
12-frame windows on one MI355X, one output file as long as the audio.

    python tools/animate_track.py --image still.png --audio sound.wav --out out/track.mp4 --scheduler unipc --steps 10
    python tools/animate_track.py --seconds 20 --out /tmp/track.mp4            # synthetic still and sound
    python tools/animate_track.py --video clip.avi --out out/track.mp4 --handover pixel

Weights: --unet DIR (a `from_pretrained` directory with an `unet` subfolder) and --sd15 DIR (VAE); without them SD1.5-shaped
networks with seeded random weights are used, which exercises the path and its speed and says nothing about the picture.  No
trained checkpoint has been run through this tool: what many chained windows do to the picture (drift) is unmeasured."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

SCHEDULERS = ("pndm", "ddim", "dpmsolver++", "unipc")


def make_scheduler(name: str):
    from asva_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler, UniPCMultistepScheduler

    return {"pndm": PNDMScheduler, "ddim": DDIMScheduler, "dpmsolver++": DPMSolverMultistepScheduler, "unipc": UniPCMultistepScheduler}[name]()


def seeded_pipeline(dev, scheduler: str, steps: int, audio_encoder: bool = True, unet_dir: str = "", sd15_dir: str = ""):
    """SD1.5-shaped UNet + VAE (+ the ImageBind audio branch) on `dev`: from the given directories, else seeded random weights"""
    import bench
    from asva_amd.audio_encoder import ImageBindSegmaskAudioEncoder
    from asva_amd.pipeline import AudioCondAnimationPipeline
    from asva_amd.unet import AudioUNet3DConditionModel
    from asva_amd.vae import AutoencoderKL

    torch.manual_seed(0)
    unet = AudioUNet3DConditionModel.from_pretrained(unet_dir, subfolder="unet").to(dev) if unet_dir else bench.build_unet(dev, 0, 1)
    if sd15_dir:
        vae = AutoencoderKL.from_pretrained(sd15_dir, subfolder="vae").to(dev)
    else:
        with torch.device(dev):
            vae = AutoencoderKL().eval()
    enc = None
    if audio_encoder:
        ckpt = ImageBindSegmaskAudioEncoder.IMAGEBIND_CKPT
        enc = ImageBindSegmaskAudioEncoder(n_segment=12, imagebind_checkpoint=ckpt if os.path.exists(ckpt) else None).to(dev).eval()
    pipe = AudioCondAnimationPipeline(unet=unet, scheduler=make_scheduler(scheduler), vae=vae, audio_encoder=enc).to(dev)
    pipe.set_progress_bar_config(disable=True)
    pipe.generation_steps = steps
    return pipe


def synthetic_track(seconds: float, seed: int = 0):
    """-> (image (3, 256, 256) in [0, 1], audio (1, T) at 16 kHz: a chirp under decaying clicks, twice a second)"""
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(3, 8, 8, generator=g)
    image = torch.nn.functional.interpolate(image[None], size=(256, 256), mode="bilinear", align_corners=False)[0].clamp(0, 1)
    t = torch.arange(int(seconds * 16000)) / 16000.0
    audio = 0.2 * torch.sin(2 * torch.pi * (220.0 + 40.0 * t) * t) + 0.5 * torch.exp(-30.0 * (t % 0.5)) * torch.randn(t.shape, generator=g)
    return image, audio.clamp(-1, 1)[None]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--image", default="")
    ap.add_argument("--audio", default="", help=".wav (any format with torchaudio)")
    ap.add_argument("--video", default="", help="takes the first frame and / or the audio track from a video")
    ap.add_argument("--seconds", type=float, default=10.0, help="length of the synthetic track when no input file is given")
    ap.add_argument("--out", required=True)
    ap.add_argument("--scheduler", choices=SCHEDULERS, default="unipc")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--handover", choices=("latent", "pixel"), default="latent")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--text-encoding", default="", help=".pt file with a (77, 768) text encoding; default: seeded random")
    ap.add_argument("--unet", default="")
    ap.add_argument("--sd15", default="")
    args = ap.parse_args()

    from asva_amd.pipeline import generate_track

    dev = torch.device("cuda", 0)
    pipe = seeded_pipeline(dev, args.scheduler, args.steps, unet_dir=args.unet, sd15_dir=args.sd15)
    if not (args.unet and args.sd15):
        print("animate_track: seeded random weights - the output shows that the path runs, not what a trained model draws", file=sys.stderr)
    if args.text_encoding:
        text = torch.load(args.text_encoding, map_location="cpu").view(1, 77, 768)
    else:
        text = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(args.seed))
    image_path, audio_path = args.image, args.audio
    if not (image_path or audio_path or args.video):              # synthetic inputs, handed over as files like any others
        import numpy as np
        from PIL import Image
        from scipy.io import wavfile

        image, audio = synthetic_track(args.seconds, args.seed)
        stem = os.path.splitext(args.out)[0]
        os.makedirs(os.path.dirname(stem) or ".", exist_ok=True)
        image_path, audio_path = stem + "_input.png", stem + "_input.wav"
        Image.fromarray((image.permute(1, 2, 0) * 255).byte().numpy()).save(image_path)
        wavfile.write(audio_path, 16000, (audio[0].numpy() * 32767.0).astype(np.int16))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frames, audio = generate_track(pipe, image_path=image_path, audio_path=audio_path, video_path=args.video, category_text_encoding=text,
                                   seed=args.seed, device=dev, handover=args.handover)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    from asva_amd.pipeline import write_video

    path = write_video(args.out, frames, 6, audio, 16000, "aac")
    print(json.dumps({"file": path, "frames": int(frames.shape[0]), "video_s": round(frames.shape[0] / 6, 2), "wall_s": round(dt, 3),
                      "video_s_per_wall_s": round(frames.shape[0] / 6 / dt, 2), "scheduler": args.scheduler, "steps": args.steps,
                      "handover": args.handover, "graph_captures": pipe._engine.captures}))


if __name__ == "__main__":
    main()
