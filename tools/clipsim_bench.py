"""Times the ImageBind towers (asva_amd/imagebind_eval.py) with seeded weights at the real shapes on an MI355X: ms per 12-frame clip for
the vision tower, ms for one text and one audio embedding, and ms per avsd_attention_f32 launch at (12 sequences, 16 heads, 257, 80) beside
torch's fp32 scaled_dot_product_attention on the same device.  Device events, warm-up, median of repeats.

    python tools/clipsim_bench.py [--layers N] [--repeats 5] [--towers vision text audio]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/clipsim_bench.py --towers vision --repeats 1      # the per-kernel split
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from asva_amd import imagebind_eval as E, ops  # noqa: E402


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


def seeded(config, dev):
    m = E.CLIPModel(config)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in m.named_parameters():
            t = torch.randn(p.shape, generator=g)
            if name.endswith((".bias", "in_proj_bias")):
                t *= 0.02
            elif p.dim() >= 2 and "norm" not in name:
                t /= max(1.0, float(t[0].numel())) ** 0.5
            else:
                t = 1.0 + 0.02 * t
            p.copy_(t)
    return m.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=None, help="blocks per tower (default: the real depth)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--towers", nargs="+", default=["vision", "text", "audio"], choices=E.TOWERS)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    g = torch.Generator().manual_seed(1)
    for tower in args.towers:
        cfg = dict(E.DEFAULT_CONFIG[tower])
        if tower == "text":
            cfg["vocab"] = 1024                          # the table is a gather: its size does not enter the time
        if args.layers is not None:
            cfg["layers"] = args.layers
        m = seeded({tower: cfg}, dev)
        if tower == "vision":
            x = torch.randn(12, 3, 224, 224, generator=g).to(dev)
            out["vision_ms_per_12_frames"] = timed(lambda: m.encode_image(x), args.repeats)
        elif tower == "text":
            ids = torch.randint(0, 1023, (1, 77), generator=g)
            out["text_ms"] = timed(lambda: m.encode_text(ids), args.repeats)
        else:
            x = torch.randn(1, 1, 128, 204, generator=g).to(dev)
            out["audio_ms"] = timed(lambda: m.encode_audio(x), args.repeats)
        out[tower + "_layers"] = cfg["layers"]
        del m
        torch.cuda.empty_cache()
    b, heads, seq, d = 12, 16, 257, 80
    qkv = torch.randn(b * seq, 3 * heads * d, generator=g).to(dev)
    c = heads * d
    out["attention_f32_ms"] = timed(lambda: ops.attention_f32(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], b, seq, heads), max(args.repeats, 5))
    q, k, v = (qkv[:, i * c:(i + 1) * c].reshape(b, seq, heads, d).transpose(1, 2).contiguous() for i in range(3))
    out["torch_sdpa_fp32_ms"] = timed(lambda: F.scaled_dot_product_attention(q, k, v), max(args.repeats, 5))
    out["attention_gflop"] = 4.0 * b * heads * seq * seq * d / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
