"""FID between two sets of frames, on the device (asva_amd/fid.py).

    python tools/fid_score.py A B --weights pt_inception-2015-12-05-6726825d.pth
    python tools/fid_score.py                       # synthetic frames, seeded random weights: shows that the path runs

A and B are each a folder of images (anything PIL opens; every image of a folder must have the same size), a folder of pre-decoded
.npz clip containers (asva_amd.data_utils: `frames` uint8 (T, H, W, 3)), or a .pt file holding a tensor (N, 3, H, W), uint8 or float in
[0, 1].  --weights (or $AVSD_FID_INCEPTION) is pytorch-fid's checkpoint; nothing is downloaded.  Without it the network gets seeded
random weights and the number means nothing."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from asva_amd import fid  # noqa: E402


def seeded_state_dict(seed=0):
    """random weights that keep a deep ReLU network alive (He convolutions, BatchNorm near the identity)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in fid.state_dict_shapes().items():
        if name.endswith("num_batches_tracked"):
            sd[name] = torch.zeros(shape, dtype=torch.int64)
        elif len(shape) >= 2:
            fan_in = int(np.prod(shape[1:]))
            sd[name] = torch.randn(shape, generator=g) * ((1.0 if len(shape) == 2 else 2.0) / fan_in) ** 0.5
        elif name.endswith("running_var") or name.endswith(".bn.weight"):
            sd[name] = 0.9 + 0.2 * torch.rand(shape, generator=g)
        else:
            sd[name] = 0.1 * torch.randn(shape, generator=g)
    return sd


def synthetic_frames(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(n, 3, size // 8, size // 8, generator=g)
    return torch.nn.functional.interpolate(base, size=(size, size), mode="bilinear", align_corners=False).clamp(0, 1)


def load_frames(path):
    """-> (N, 3, H, W) float32 in [0, 1] on the CPU"""
    if os.path.isfile(path):
        t = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3:
            raise SystemExit(f"{path}: expected a tensor (N, 3, H, W)")
        return t.float() / 255.0 if t.dtype == torch.uint8 else t.float()
    files = sorted(os.listdir(path))
    if not files:
        raise SystemExit(f"{path}: empty folder")
    frames = []
    for f in files:
        p = os.path.join(path, f)
        if f.lower().endswith(".npz"):
            frames.append(torch.from_numpy(np.load(p)["frames"]).permute(0, 3, 1, 2))
        else:
            from PIL import Image

            frames.append(torch.from_numpy(np.asarray(Image.open(p).convert("RGB"))).permute(2, 0, 1)[None])
    if len({tuple(f.shape[1:]) for f in frames}) != 1:
        raise SystemExit(f"{path}: the frames differ in size")
    return torch.cat(frames).float() / 255.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a", nargs="?", default=None)
    ap.add_argument("b", nargs="?", default=None)
    ap.add_argument("--weights", default=None, help="pytorch-fid's Inception checkpoint (default: $AVSD_FID_INCEPTION)")
    ap.add_argument("--frames", type=int, default=6, help="synthetic frames per set when no folders are given")
    ap.add_argument("--size", type=int, default=96)
    args = ap.parse_args()
    if (args.a is None) != (args.b is None):
        ap.error("give both sets of frames, or neither")
    dev = torch.device("cuda", 0)
    weights = args.weights or os.environ.get(fid.ENV_WEIGHTS)
    if weights:
        net = fid.load_inceptionv3_pretrained(block_ids=[3], weights=weights)
    else:
        print("no --weights: seeded random weights, the number below means nothing")
        net = fid.InceptionV3((3,))
        net.load_state_dict(seeded_state_dict())
    net = net.to(dev)
    if args.a is None:
        sets = [synthetic_frames(args.frames, args.size, 1), synthetic_frames(args.frames, args.size, 2)]
    else:
        sets = [load_frames(args.a), load_frames(args.b)]
    feats = [fid.compute_fid_image_features(s.to(dev), net).cpu() for s in sets]
    print(f"frames: {sets[0].shape[0]} of {tuple(sets[0].shape[2:])} and {sets[1].shape[0]} of {tuple(sets[1].shape[2:])}")
    print(f"FID: {fid.frechet_distance(feats[0], feats[1]).item():.6f}")


if __name__ == "__main__":
    main()
