"""Time per prompt of the CLIP text encoder at the SD1.5 shape (12 layers, C = 768, 12 heads, intermediate 3072; vocabulary cut to
1024, seeded weights), for the device library and for the fp32 torch restatement (tests/clip_text_ref.py) on the same device:

    python tools/clip_text_bench.py [--batches 1 16] [--iters 20]
    rocprofv3 --kernel-trace --stats -d /tmp/clip_kt -o kt -- python tools/clip_text_bench.py --batches 1 --iters 5 --no-torch
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from asva_amd.text_encoder import CLIPTextModel  # noqa: E402
from tests import clip_text_ref as R  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    cfg, dev = R.SD15, torch.device("cuda", 0)
    sd = R.draw_state_dict(cfg)
    m = CLIPTextModel.from_config(cfg)
    m.load_state_dict(sd)
    m = m.to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    out = {}
    for b in args.batches:
        ids = R.make_ids(cfg)["eos10"].expand(b, -1).contiguous()
        dev_ids = ids.to(torch.int32).view(-1).to(dev)
        pk = m.pack(dev)
        row = dict(native_ms=timed(lambda: m.encode_ids(dev_ids, b, 77, pk), args.iters))
        if not args.no_torch:
            ids_dev = ids.to(dev)
            with torch.no_grad():
                row["torch_fp32_ms"] = timed(lambda: R.forward(sd_dev, cfg, ids_dev), args.iters)
                row["torch_fp32_ms_per_prompt"] = row["torch_fp32_ms"] / b
                row["rel_l2_native_vs_torch"] = R.rel_l2(m.encode_ids(dev_ids, b, 77, pk).view(b, 77, -1), R.forward(sd_dev, cfg, ids_dev))
        row["native_ms_per_prompt"] = row["native_ms"] / b
        out[f"B{b}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
