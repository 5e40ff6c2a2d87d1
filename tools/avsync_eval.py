"""The AVSync classifier's own evaluation (the reference's scripts/avsync_eval.py) on the device: shift accuracy.  From every recording
`--num_clips` clips shifted by `--shift_time` seconds are cut; the centre audio is scored against all the videos and all the audios
against the centre video; a prediction is a hit when its argmax lies within `--tolerate_range` of the centre.

    python tools/avsync_eval.py --checkpoint checkpoints/avsync/.../modules --data_root clips/ --example_list_path clips/test.txt
    python tools/avsync_eval.py --synthetic 4                      # seeded weights on generated gratings and tones

Recordings are the project's own .avi files (Motion-JPEG + PCM, asva_amd/video_io.py).  The audio of a clip is cut sample-exact, where
the reference gathers whole container packets (asva_amd.avsync.shifted_pairs).  With --synthetic the classifier has seeded random
weights and the accuracies mean nothing: the run then only shows that the path works and what it costs.  No trained classifier and no
VGGSS data were available when this was written: no accuracy of a real checkpoint has been measured."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from asva_amd import _lib, avsync  # noqa: E402

BATCH = 8                                     # the reference's loader
KERNELS = {"avsd_resize_aa_normalize_f32": 2}   # kernels per entry point where it is not one (avsd_pair_xent_f32: one when P != Q)


class _Counting:
    """the library handle with every launching entry point counted"""

    def __init__(self, handle, counts):
        self._handle, self._counts = handle, counts

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if not name.startswith("avsd_") or name in ("avsd_last_error", "avsd_abi_version", "avsd_precision"):
            return fn

        def call(*args):
            self._counts[name] = self._counts.get(name, 0) + KERNELS.get(name, 1)
            return fn(*args)

        return call


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


def synthetic_recording(seed, seconds=4.0, fps=24, size=112, sample_rate=16000):
    """a moving grating and a few amplitude-modulated tones: (frames (F, 3, H, W) in [0, 1], frame_seconds [F], waveform (1, S), rate)"""
    g = torch.Generator().manual_seed(2000 + seed)
    p = torch.rand(6, generator=g)
    n = int(seconds * fps)
    t = torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1)
    y = torch.arange(size, dtype=torch.float32).view(1, 1, size, 1)
    x = torch.arange(size, dtype=torch.float32).view(1, 1, 1, size)
    c = torch.arange(3, dtype=torch.float32).view(1, 3, 1, 1)
    angle = 3.0 * p[0]
    arg = 2 * torch.pi * ((x * torch.cos(angle) + y * torch.sin(angle)) / (9.0 + 30.0 * p[1]) - (0.05 + 0.3 * p[2]) * t) + 0.9 * c
    frames = (0.5 + 0.45 * torch.sin(arg)).contiguous()
    s = torch.arange(int(seconds * sample_rate), dtype=torch.float32) / sample_rate
    f, m = 200.0 + 2000.0 * p[3:5], 1.0 + 5.0 * p[4:6]
    wave = (0.15 * torch.sin(2 * torch.pi * f[:, None] * s) * (1.0 + torch.sin(2 * torch.pi * m[:, None] * s))).sum(0, keepdim=True)
    return frames, np.arange(n, dtype=np.float64) / fps, wave, sample_rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", type=str, default=None, help="directory with audio_encoder/ video_encoder/ head/")
    ap.add_argument("--data_root", type=str, default="./datasets/VGGSS/videos")
    ap.add_argument("--example_list_path", type=str, default="./datasets/VGGSS/test.txt")
    ap.add_argument("--shift_time", type=float, default=0.04)
    ap.add_argument("--num_clips", type=int, default=31)
    ap.add_argument("--tolerate_range", type=int, default=5)
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N generated recordings and seeded weights instead of files")
    ap.add_argument("--seed", type=int, default=123)
    args = ap.parse_args()
    if not args.synthetic and not args.checkpoint:
        ap.error("--checkpoint is required (or --synthetic N)")
    dev = torch.device("cuda", 0)
    cut = dict(num_clips=args.num_clips, shift_time=args.shift_time, device=dev)

    if args.synthetic:
        print("WARNING: --synthetic: the classifier has seeded random weights and the accuracies below mean nothing")
        net = seeded_classifier(args.seed).to(dev)
        n_examples = args.synthetic
        load = lambda i: avsync.shifted_pairs(*synthetic_recording(args.seed + i), **cut)  # noqa: E731
    else:
        net = avsync.load_avsync_model(args.checkpoint).to(dev)
        with open(args.example_list_path) as f:
            examples = [line.strip() for line in f if line.strip()]
        for e in examples:
            if not e.lower().endswith(".avi"):
                raise SystemExit(f"{e}: only the project's own .avi files (Motion-JPEG + PCM) can be read here")
        n_examples = len(examples)
        load = lambda i: avsync.shifted_pairs_from_avi(os.path.join(args.data_root, examples[i]), **cut)  # noqa: E731

    def batches(counted):
        for lo in range(0, n_examples, BATCH):
            idx = list(range(lo, min(lo + BATCH, n_examples)))
            pairs = [load(i) for i in idx]
            counted.append(len(idx))
            yield {"index": torch.tensor(idx), "audio": torch.stack([a for a, _ in pairs]), "video": torch.stack([v for _, v in pairs])}

    # warm-up: pack the weights, load the code objects
    a, v = load(0)
    avsync.shift_accuracy(net, a[None], v[None], args.tolerate_range)
    torch.cuda.synchronize()

    counts, done = {}, []
    real = _lib.lib
    _lib.lib = lambda: _Counting(real(), counts)
    try:
        t0 = time.perf_counter()
        r = avsync.evaluate_shift_accuracy(net, batches(done), args.tolerate_range)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        _lib.lib = real
    n = sum(done)
    print("#########################################################################")
    print(f"Evaluation result:\ncheckpoint = {args.checkpoint if not args.synthetic else '(seeded weights)'}")
    print("#########################################################################")
    print(f"valid examples = {r['valid_examples']}\nav_acc = {r['av_acc']:.4f}\nva_acc = {r['va_acc']:.4f}")
    head = sum(counts.get(k, 0) for k in ("avsd_pair_head_f32", "avsd_pair_xent_f32"))
    print(f"{sum(counts.values()) / n:.1f} launches and {1e3 * dt / n:.1f} ms per example ({args.num_clips} clips each: cutting, mel spectrograms, resize, "
          f"both encoders; per batch the two pair scorings are four half-layer launches and {head / max(1, len(done)):.0f} of avsd_pair_head_f32 / "
          f"avsd_pair_xent_f32)")


if __name__ == "__main__":
    main()
