"""FVD between two sets of clips, on the device (asva_amd/fvd.py).

    python tools/fvd_score.py A B --weights i3d_torchscript.pt
    python tools/fvd_score.py                       # synthetic clips, seeded random weights: shows that the path runs

A and B are each a folder of pre-decoded .npz clip containers (asva_amd.data_utils: `frames` uint8 (T, H, W, 3); every clip of a folder
must have the same shape, at least 9 frames) or a .pt file holding a tensor (N, 3, T, H, W), uint8 or float in [0, 1].  --weights (or
$AVSD_FVD_I3D) is the StyleGAN-V I3D detector (a TorchScript archive) or a state dict in the layout of the reference's InceptionI3d;
nothing is downloaded.  Without it the network gets seeded random weights and the number means nothing."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from asva_amd import fvd  # noqa: E402


def seeded_state_dict(seed=0):
    """random weights that keep a deep ReLU network alive (He convolutions, BatchNorm near the identity)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in fvd.state_dict_shapes().items():
        if name.endswith("num_batches_tracked"):
            sd[name] = torch.zeros(shape, dtype=torch.int64)
        elif len(shape) >= 2:
            fan_in = int(np.prod(shape[1:]))
            sd[name] = torch.randn(shape, generator=g) * ((1.0 if name.startswith("logits.") else 2.0) / fan_in) ** 0.5
        elif name.endswith("running_var") or name.endswith(".bn.weight"):
            sd[name] = 0.9 + 0.2 * torch.rand(shape, generator=g)
        else:
            sd[name] = 0.1 * torch.randn(shape, generator=g)
    return sd


def synthetic_clips(n, frames, size, seed):
    """(n, 3, frames, size, size) in [0, 1]: smooth random fields that change from frame to frame"""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(n, 3, max(frames // 3, 2), size // 8, size // 8, generator=g)
    return torch.nn.functional.interpolate(base, size=(frames, size, size), mode="trilinear", align_corners=False).clamp(0, 1)


def load_clips(path):
    """-> (N, 3, T, H, W) float32 in [0, 1] on the CPU"""
    if os.path.isfile(path):
        t = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(t, torch.Tensor) or t.dim() != 5 or t.shape[1] != 3:
            raise SystemExit(f"{path}: expected a tensor (N, 3, T, H, W)")
        return t.float() / 255.0 if t.dtype == torch.uint8 else t.float()
    files = sorted(f for f in os.listdir(path) if f.lower().endswith(".npz"))
    if not files:
        raise SystemExit(f"{path}: no .npz clip containers")
    clips = [torch.from_numpy(np.load(os.path.join(path, f))["frames"]).permute(3, 0, 1, 2) for f in files]
    if len({tuple(c.shape) for c in clips}) != 1:
        raise SystemExit(f"{path}: the clips differ in shape")
    return torch.stack(clips).float() / 255.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a", nargs="?", default=None)
    ap.add_argument("b", nargs="?", default=None)
    ap.add_argument("--weights", default=None, help="the I3D detector archive or a state dict (default: $AVSD_FVD_I3D)")
    ap.add_argument("--bn-eps", type=float, default=None, help="BatchNorm epsilon (default: see asva_amd.fvd.load_i3d_pretrained)")
    ap.add_argument("--clips", type=int, default=3, help="synthetic clips per set when no folders are given")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--size", type=int, default=64)
    args = ap.parse_args()
    if (args.a is None) != (args.b is None):
        ap.error("give both sets of clips, or neither")
    dev = torch.device("cuda", 0)
    weights = args.weights or os.environ.get(fvd.ENV_WEIGHTS)
    if weights:
        net = fvd.load_i3d_pretrained(weights=weights, bn_eps=args.bn_eps)
    else:
        print("no --weights: seeded random weights, the number below means nothing")
        net = fvd.InceptionI3d()
        net.load_state_dict(seeded_state_dict())
    net = net.to(dev)
    if args.a is None:
        sets = [synthetic_clips(args.clips, args.frames, args.size, 1), synthetic_clips(args.clips, args.frames, args.size, 2)]
    else:
        sets = [load_clips(args.a), load_clips(args.b)]
    feats = [fvd.compute_fvd_video_features(s.to(dev), net).cpu() for s in sets]
    print(f"clips: {sets[0].shape[0]} of {tuple(sets[0].shape[2:])} and {sets[1].shape[0]} of {tuple(sets[1].shape[2:])}")
    print(f"FVD: {fvd.frechet_distance(feats[0], feats[1]).item():.6f}")


if __name__ == "__main__":
    main()
