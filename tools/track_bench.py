"""Whole-track animation on one MI355X, measured: a synthetic 20 s track (11 chained windows, 120 frames) through
AudioCondAnimationPipeline.animate_track on SD1.5-shaped networks with seeded random weights, PNDM-50 and UniPC-10, against the
same track made by hand: one `generate_videos` single-clip call per window, each started from the last frame of the one before
(the by-hand cost minus file I/O).  Writes profiles/long_track.md.

    python tools/track_bench.py [--out profiles/long_track.md] [--seconds 20]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from animate_track import make_scheduler, seeded_pipeline, synthetic_track
from asva_amd.data_utils import track_windows
from asva_amd.pipeline import generate_videos

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "long_track.md"))
ap.add_argument("--seconds", type=float, default=20.0)
args = ap.parse_args()

dev = torch.device("cuda", 0)
pipe = seeded_pipeline(dev, "pndm", 50)
image, audio = synthetic_track(args.seconds)
text = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(0))
windows, W, n_frames, padded = track_windows(audio.shape[1])
F, FPS, WIN = 12, 6, 32000


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def chain(steps, handover, marks=None):
    pipe._track_mark = (lambda k, what: marks.append((k, what, sync()))) if marks is not None else None
    gen = torch.Generator(device=dev).manual_seed(0)
    t0 = sync()
    frames = pipe.animate_track(image, audio, texts=[""], text_encodings=[text], num_inference_steps=steps, audio_guidance_scale=4.0,
                                generator=gen, handover=handover, output_type="uint8")
    t1 = sync()
    pipe._track_mark = None
    return frames, t0, t1


def by_hand(steps):
    """W single-clip generate_videos calls: the last frame of a clip is the next clip's image (8-bit, as a file would hold it), the
    audio is the same window the chain hears.  No file is written or read."""
    pipe.generation_steps = steps
    wave = torch.cat([audio, torch.zeros(1, padded - audio.shape[1])], 1)
    img, out = image, []
    t0 = sync()
    for s, _ in windows:
        vids, _ = generate_videos(pipe, category_text_encoding=text, num_clips_per_video=1, seed=0, device=dev,
                                  clips=[dict(image=img, audio=wave[:, s:s + WIN])])
        out.append(vids[0])
        img = vids[0][-1].permute(2, 0, 1).float() / 255.0
    return out, t0, sync()


rows, notes = [], []
for name, steps in (("pndm", 50), ("unipc", 10)):
    pipe.scheduler = make_scheduler(name)
    label = f"{'PNDM' if name == 'pndm' else 'UniPC'}-{steps}"
    chain(steps, "latent")                                             # warm-up: tile table, graph capture, allocator
    by_hand(steps)
    cap0 = pipe._engine.captures
    best = {}
    for handover in ("latent", "pixel"):
        runs = [chain(steps, handover) for _ in range(3)]
        best[handover] = min(t1 - t0 for _, t0, t1 in runs)
        assert runs[0][0].shape == (n_frames, 256, 256, 3)
    marks = []
    _, t0, t1 = chain(steps, "latent", marks)
    caps = pipe._engine.captures
    phase = {"turnover": 0.0, "denoise": 0.0, "decode": 0.0}
    at = {(k, what): t for k, what, t in marks}
    for k in range(1, W):                                               # windows 1.. : the steady state (window 0 has no turnover)
        phase["turnover"] += at[(k, "denoise")] - at[(k, "start")]
        phase["denoise"] += at[(k, "decode")] - at[(k, "denoise")]
        phase["decode"] += at[(k, "end")] - at[(k, "decode")]
    cond_s = at[(0, "start")] - t0                                      # resample + upload + all W audio encodings + text
    hand = min(t1 - t0 for _, t0, t1 in (by_hand(steps) for _ in range(3)))
    per_win, per_clip = best["latent"] / W, hand / W
    rows.append(f"| {label} | {W} | {best['latent']:.3f} | {per_win * 1e3:.1f} | {phase['denoise'] / (W - 1) * 1e3:.1f} | "
                f"{phase['decode'] / (W - 1) * 1e3:.1f} | {phase['turnover'] / (W - 1) * 1e3:.2f} | {cond_s * 1e3:.1f} | "
                f"{n_frames / FPS / best['latent']:.2f} | {best['pixel']:.3f} | {hand:.3f} | {per_clip * 1e3:.1f} | {per_win / per_clip:.3f} | "
                f"{cap0} -> {caps} |")
    print(rows[-1], flush=True)

md = f"""# Whole-track animation: chained windows on the device

`python tools/track_bench.py` on one MI355X.  Synthetic {args.seconds:g} s track at 16 kHz -> {W} windows of 12 frames sharing one
frame each, {n_frames} frames at 6 fps after trimming.  SD1.5-shaped UNet and VAE and the ImageBind-Huge audio branch, all with
**seeded random weights: these are times, not pictures.  No trained checkpoint was available, so nothing here says what the
chain does to image quality, and drift over many windows is unmeasured.**  256 x 256, audio guidance 4.0, bf16 storage.

* chain: `animate_track(image, waveform)`, `handover="latent"`, frames copied to the host window by window (`output_type="uint8"`);
  wall time of the whole call, best of 3 after a warm-up track.  It contains the VAE encode of the still, the one upload of the
  track, all {W} + 1 audio encodings (batches of 16) and the text rows ("conditioning"), then per window: turnover
  (`avsd_window_turnover` + the noise draw + `set_conditioning` in place + `prepare`), denoising, VAE decode + copy of the frames.
  The per-phase columns come from a fourth run that synchronises at every phase boundary, windows 1.. only.
* by hand: {W} `generate_videos` single-clip calls in the same process and session, each with the window's audio and, as its
  image, the last frame of the clip before (8-bit pixels, as a file would hold them) - per clip a VAE encode, an audio
  encoding, the conditioning upload, denoising, decode and copy.  No file is written or read, so this is the by-hand cost minus
  file I/O.  `generate_videos` and everything it calls are the parent commit's code unchanged (the engine lookup moved into a
  helper), which is why the comparison runs in this tree rather than in a second build; best of 3.
* `captures`: `DenoiseEngine.captures` before -> after the timed chains (7 tracks, {7 * W} windows): no window re-captures the graph.

| sampler | windows | chain s | per window ms | denoise ms | decode + copy ms | turnover + conditioning switch ms | conditioning, once ms | video s per wall s | chain, pixel hand-over s | by hand s | per clip ms | per window / per clip | captures |
|---|---|---|---|---|---|---|---|---|---|---|---|---|---|
""" + "\n".join(rows) + """

The claim: the chain's time per window is no larger than the by-hand time per clip - the ratio column.
"""
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(md)
print(md)
