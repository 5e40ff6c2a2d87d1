"""Times the FID feature extractor (asva_amd/fid.py) with seeded weights at the real shapes on an MI355X: ms per 12 x 256 x 256 clip for
preprocessing + Inception features at 1 and 8 clips per call, the share of every stage at both batch sizes, the launch count, and — a
yardstick to report, not a gate — the same folded network as plain torch F.conv2d / pooling calls on the same device.
Device events, warm-up, median of repeats.

    python tools/fid_bench.py [--repeats 5] [--clips 1 8] [--no-torch] [--no-stages]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/fid_bench.py --clips 1 --repeats 1 --no-torch --no-stages   # the per-kernel split
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from asva_amd import fid  # noqa: E402
from fid_score import seeded_state_dict  # noqa: E402

FRAMES, SIZE = 12, 256


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


class _Counting(fid._Hip):
    """the device backend, counting launches (every conv / pool / mean / linear call is one kernel launch)"""
    n = 0

    @staticmethod
    def conv(x, layer, out=None):
        _Counting.n += 1
        return fid._Hip.conv(x, layer, out)

    @staticmethod
    def pool(*a, **k):
        _Counting.n += 1
        return fid._Hip.pool(*a, **k)

    @staticmethod
    def mean(x):
        _Counting.n += 1
        return fid._Hip.mean(x)


class _Torch:
    """the folded network as torch-ROCm calls on NCHW f32 (MIOpen convolutions): the yardstick.  Tensors are passed around as
    channels-last 5-d VIEWS of NCHW memory so that fid.run_network drives it unchanged; a slice write is a torch copy."""
    empty = staticmethod(lambda shape, like: torch.empty((shape[0], shape[4], shape[2], shape[3]), dtype=torch.float32,
                                                         device=like.device).permute(0, 2, 3, 1).unsqueeze(1))

    @staticmethod
    def _nchw(x):
        return x[:, 0].permute(0, 3, 1, 2)

    @staticmethod
    def _ret(y, out):
        y = y.permute(0, 2, 3, 1).unsqueeze(1)
        if out is None:
            return y
        out.copy_(y)
        return out

    @staticmethod
    def conv(x, layer, out=None):
        (_, kh, kw), cin = layer.taps, layer.cin
        w = layer.w[:, :kh * kw * cin].view(-1, kh, kw, cin).permute(0, 3, 1, 2)
        y = F.relu(F.conv2d(_Torch._nchw(x).contiguous(), w, layer.bias, layer.stride[1:], layer.pad[1:]))
        return _Torch._ret(y, out)

    @staticmethod
    def pool(x, mode, stride, pad, out=None):
        x = _Torch._nchw(x)
        y = F.max_pool2d(x, 3, stride, pad) if mode == "max" else F.avg_pool2d(x, 3, stride, pad, count_include_pad=False)
        return _Torch._ret(y, out)

    @staticmethod
    def mean(x):
        return _Torch._nchw(x).mean(dim=(2, 3))

    linear = staticmethod(F.linear)


def stage_inputs(pk, n, dev):
    """a random input of the right shape for every stage of the network at 229 x 229, found by running the network once"""
    st = {}
    x = torch.rand(n, 1, fid.INPUT_SIZE, fid.INPUT_SIZE, 3, device=dev) * 2 - 1
    fid.run_network(pk, x, 3, stages=st)
    return x, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clips", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-stages", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    net = fid.InceptionV3((3,))
    net.load_state_dict(seeded_state_dict())
    net = net.to(dev)
    pk = net.pack(dev)
    out = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "frames": FRAMES, "size": SIZE}
    g = torch.Generator().manual_seed(1)
    for clips in args.clips:
        n = clips * FRAMES
        images = torch.rand(n, 3, SIZE, SIZE, generator=g).to(dev)
        ms = timed(lambda: fid.compute_fid_image_features(images, net), args.repeats)
        out[f"ms_per_clip_at_{clips}_clips"] = ms / clips
        out[f"preprocess_ms_per_clip_at_{clips}_clips"] = timed(lambda: fid.preprocess_images(images), args.repeats) / clips
        x = fid.preprocess_images(images).permute(0, 2, 3, 1).contiguous().view(n, 1, fid.INPUT_SIZE, fid.INPUT_SIZE, 3)
        _Counting.n = 0
        fid.run_network(pk, x, 3, be=_Counting)
        out["launches_network"] = _Counting.n                       # + 2 for the preprocessing (horizontal and vertical pass)
        if not args.no_torch:
            feats = fid.run_network(pk, x, 3)[3]
            ref = fid.run_network(pk, x, 3, be=_Torch)[3]
            out[f"torch_vs_device_rel_l2_at_{clips}_clips"] = ((ref - feats).norm() / feats.norm()).item()
            out[f"torch_conv2d_ms_per_clip_at_{clips}_clips"] = timed(lambda: fid.run_network(pk, x, 3, be=_Torch), args.repeats) / clips
            out[f"network_ms_per_clip_at_{clips}_clips"] = timed(lambda: fid.run_network(pk, x, 3), args.repeats) / clips
        if not args.no_stages:
            _, st = stage_inputs(pk, n, dev)
            prev, shares = x, {}
            stem = {"Conv2d_1a_3x3": 0, "Conv2d_2a_3x3": 1, "Conv2d_2b_3x3": 2, "Conv2d_3b_1x1": 3, "Conv2d_4a_3x3": 4}
            blocks = {name: b for (name, _, _), b in zip(fid.BLOCKS, pk.blocks)}
            for name in fid.STAGE_NAMES:
                xin = prev if name != "Conv2d_4a_3x3" else None
                if name in stem:
                    layer = pk.stem[stem[name]]
                    if name == "Conv2d_4a_3x3":                      # reads the 96-wide padded output of Conv2d_3b_1x1
                        xin = fid._Hip.conv(st["maxpool1"], pk.stem[3])
                    fn = lambda xin=xin, layer=layer: fid._Hip.conv(xin, layer)                     # noqa: E731
                elif name.startswith("maxpool"):
                    fn = lambda xin=xin: fid._Hip.pool(xin, "max", 2, 0)                           # noqa: E731
                else:
                    fn = lambda xin=xin, b=blocks[name]: fid._run_block(b, xin, fid._Hip)           # noqa: E731
                shares[name] = timed(fn, args.repeats) / clips
                prev = st[name]
            out[f"stage_ms_per_clip_at_{clips}_clips"] = shares
    print(json.dumps(out))


if __name__ == "__main__":
    main()
