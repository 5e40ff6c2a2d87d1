"""Times the on-device baseline JPEG encoder (asva_amd/video_io.py:encode_jpeg_frames; kernels in csrc/jpeg.hip) against PIL's
encoder on one 12 x 256 x 256 clip, and a whole clip of generate_videos with either encoder, on one MI355X in one session.

  * encode: the clip's uint8 frames are on the device (where avsd_vae_postprocess_u8 leaves them).  "host" = copy the raw frames
    to the host + PIL's encode of each (quality 95, PIL's default 4:2:0, as write_mjpeg_avi does; 4:4:4 as well, the like-for-like
    figure); "device" = encode_jpeg_frames, both of its copies, stuffing and headers included.  Wall time, median / min / max.
    The two entry points alone by device events, and per kernel by a `rocprofv3 --kernel-trace --stats` run of a child
    process (--rocprof).  Stream sizes against the raw frames.
  * clip: generate_videos (UniPC-2, 10 steps, random SD1.5-shaped weights, synthetic conditioning, one clip per call, files
    written to a temporary directory), alternating "host" and "device", wall time per call.

There is no speed gate: the numbers go to profiles/jpeg_encoder.md.

    python tools/jpeg_bench.py [--repeats 9] [--runs 7] [--rocprof] [--out profiles/jpeg_encoder.md]
    python tools/jpeg_bench.py --quick          # the encode part only, one short pass, prints only
    python tools/jpeg_bench.py --kernels-only   # what the rocprofv3 child runs: a few encodes, nothing else
"""
import argparse
import csv
import glob
import io
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from asva_amd import ops, video_io  # noqa: E402


def clip_frames(T=12, H=256, W=256, seed=0):
    """smooth moving colour gradients plus 3 % noise: stands in for decoded frames (random weights decode to noise)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for t in range(T):
        base = np.stack([128 + 90 * np.sin(x / 37.0 + 0.3 * t) * np.cos(y / 53.0), 128 + 80 * np.cos(x / 71.0 - y / 29.0 + 0.2 * t),
                         128 + 70 * np.sin((x + y) / 47.0 - 0.1 * t)], axis=-1)
        out.append(np.clip(np.rint(base + rng.normal(0.0, 0.03 * 255.0, base.shape)), 0, 255).astype(np.uint8))
    return np.stack(out)


def pil_encode(video, quality=95, **kw):
    from PIL import Image

    out = []
    for f in video:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="JPEG", quality=quality, **kw)
        out.append(buf.getvalue())
    return out


def wall(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def events(fn, repeats, calls=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def encode_part(repeats):
    dev = torch.device("cuda", 0)
    frames = torch.from_numpy(clip_frames()).to(dev)
    qy, qc, qy_d, qc_d = video_io._device_tables(95, dev)
    res = {"raw_bytes": frames.numel()}
    res["host_420_ms"] = wall(lambda: pil_encode(frames.cpu().numpy()), repeats)
    res["host_444_ms"] = wall(lambda: pil_encode(frames.cpu().numpy(), subsampling=0), repeats)
    host_frames = frames.cpu().numpy()
    res["host_420_encode_alone_ms"] = wall(lambda: pil_encode(host_frames), repeats)
    res["raw_copy_ms"] = wall(lambda: frames.cpu(), repeats)
    res["device_ms"] = wall(lambda: video_io.encode_jpeg_frames(frames), repeats)
    res["quantize_ms"] = events(lambda: ops.jpeg_quantize(frames, qy_d, qc_d), repeats)
    coef = ops.jpeg_quantize(frames, qy_d, qc_d)
    res["pack_ms"] = events(lambda: ops.jpeg_pack(coef), repeats)
    dev_jpegs = video_io.encode_jpeg_frames(frames)
    res["bytes_device_444"] = sum(len(j) for j in dev_jpegs)
    res["bytes_copied_device"] = 4 * frames.shape[0] + frames.shape[0] * int(ops.jpeg_pack(coef)[1].max())
    res["bytes_pil_444"] = sum(len(j) for j in pil_encode(host_frames, subsampling=0))
    res["bytes_pil_420"] = sum(len(j) for j in pil_encode(host_frames))
    return res


def kernels_only():
    dev = torch.device("cuda", 0)
    frames = torch.from_numpy(clip_frames()).to(dev)
    for _ in range(10):
        video_io.encode_jpeg_frames(frames)
    torch.cuda.synchronize()


def rocprof_part():
    """per-kernel device time of ten encodes, from a rocprofv3 kernel trace of a child process"""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="jpeg_rocprof_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--kernels-only"]
        r = subprocess.run(["timeout", "-k", "10", "240", *cmd], capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            return {"error": f"rocprofv3 exited with {r.returncode}: {r.stderr[-500:]}"}
        rows = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    m = re.search(r"jpeg_\w+", row.get("Name", ""))
                    if m:
                        rows[m.group(0)] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                            "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        return rows or {"error": "no jpeg kernels in the trace"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def clip_part(runs):
    import bench
    from asva_amd.pipeline import AudioCondAnimationPipeline, generate_videos, synthetic_clip
    from asva_amd.schedulers import UniPCMultistepScheduler
    from asva_amd.vae import AutoencoderKL

    dev = torch.device("cuda", 0)
    unet = bench.build_unet(dev, 0, 1)
    with torch.device(dev):
        vae = AutoencoderKL().eval()
    pipe = AudioCondAnimationPipeline(unet=unet, scheduler=UniPCMultistepScheduler(), vae=vae).to(dev)
    pipe.set_progress_bar_config(disable=True)
    pipe.generation_steps = 10
    c = synthetic_clip(1, device=dev)
    clips = [dict(image_latents=c["image_latents"], audio_encodings=c["audio_encodings"], null_audio_encodings=c["null_audio_encodings"])]
    tmp = tempfile.mkdtemp(prefix="jpeg_clip_")
    times, sizes = {"host": [], "device": []}, {}
    try:
        def run(mode, k):
            video_io.set_jpeg_encoder(mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate_videos(pipe, category="", category_text_encoding=c["text_encodings"][None], clips=clips, seed=3, device=dev,
                            save_template=os.path.join(tmp, f"{mode}{k}"))
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for mode in ("host", "device"):                     # autotune, graph capture, first-use costs
                run(mode, "w")
            for k in range(runs):
                for mode in ("host", "device"):
                    times[mode].append(run(mode, k))
        for mode in ("host", "device"):
            path = glob.glob(os.path.join(tmp, f"{mode}0_clip-00.*"))[0]
            sizes[mode] = os.path.getsize(path)
    finally:
        video_io.set_jpeg_encoder("host")
        shutil.rmtree(tmp, ignore_errors=True)
    return {"runs": runs, "host_s": times["host"], "device_s": times["device"], "file_bytes": sizes}


def fmt(d, unit=""):
    return f"{d['median']:.3f}{unit} ({d['min']:.3f} – {d['max']:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encoder.md"))
    args = ap.parse_args()
    if args.kernels_only:
        kernels_only()
        return
    res = {"device": torch.cuda.get_device_name(0), "encode": encode_part(2 if args.quick else args.repeats)}
    e = res["encode"]
    lines = ["", "| one 12 x 256 x 256 clip, quality 95, frames on the device | ms, median (min – max) |", "|---|---|",
             f"| raw copy to the host + PIL 4:2:0 (what `write_mjpeg_avi` does by default) | {fmt(e['host_420_ms'])} |",
             f"| raw copy to the host + PIL 4:4:4 | {fmt(e['host_444_ms'])} |",
             f"| PIL 4:2:0 alone, frames already on the host | {fmt(e['host_420_encode_alone_ms'])} |",
             f"| raw copy alone ({e['raw_bytes']} bytes) | {fmt(e['raw_copy_ms'])} |",
             f"| `encode_jpeg_frames`: both kernels' entry points, both copies, stuffing, headers | {fmt(e['device_ms'])} |",
             f"| `ops.jpeg_quantize` alone (device events, allocation included) | {fmt(e['quantize_ms'])} |",
             f"| `ops.jpeg_pack` alone (device events, three launches and allocations) | {fmt(e['pack_ms'])} |",
             "", "| bytes | |", "|---|---|", f"| raw frames | {e['raw_bytes']} |",
             f"| device streams, 4:4:4, with headers | {e['bytes_device_444']} ({100 * e['bytes_device_444'] / e['raw_bytes']:.1f} % of raw) |",
             f"| copied from the device by `encode_jpeg_frames` (counts + streams cut to the longest) | {e['bytes_copied_device']} ({100 * e['bytes_copied_device'] / e['raw_bytes']:.1f} % of raw) |",
             f"| PIL 4:4:4 | {e['bytes_pil_444']} |", f"| PIL 4:2:0 | {e['bytes_pil_420']} |"]
    if args.rocprof and not args.quick:
        res["rocprof"] = rocprof_part()
        lines += ["", "| kernel (rocprofv3 kernel trace, ten encodes in a child process) | calls | average µs | min – max µs |", "|---|---|---|---|"]
        if "error" in res["rocprof"]:
            lines.append(f"| not collected: {res['rocprof']['error']} | | | |")
        else:
            for name, k in sorted(res["rocprof"].items()):
                lines.append(f"| `{name}` | {k['calls']} | {k['avg_us']:.1f} | {k['min_us']:.1f} – {k['max_us']:.1f} |")
    if not args.quick:
        res["clip"] = clip_part(args.runs)
        c = res["clip"]
        h, d = c["host_s"], c["device_s"]
        lines += ["", f"| `generate_videos`, one clip, UniPC-2 at 10 steps, file written; {c['runs']} alternating runs each | s per call, median (min – max) | file bytes |",
                  "|---|---|---|",
                  f"| `\"host\"` | {statistics.median(h):.4f} ({min(h):.4f} – {max(h):.4f}) | {c['file_bytes']['host']} |",
                  f"| `\"device\"` | {statistics.median(d):.4f} ({min(d):.4f} – {max(d):.4f}) | {c['file_bytes']['device']} |"]
        gain, spread = statistics.median(h) - statistics.median(d), max(max(h) - min(h), max(d) - min(d))
        lines += ["", f"Clip level: the medians differ by {1e3 * gain:.2f} ms ({100 * gain / statistics.median(h):.1f} % of the `\"host\"` clip); the larger "
                  f"of the two min-max spreads is {1e3 * spread:.2f} ms.  " +
                  ("The gain is beyond the run-to-run spread." if gain > spread else
                   "**No gain beyond the run-to-run spread was measured**; the encoder stays, opt-in, for what it removes from the host and "
                   "for the C-ABI callers.") + "  The default stays `\"host\"` either way."]
    print(json.dumps(res))
    table = "\n".join(lines)
    print(table)
    print("device encoder measured against PIL: see the first table")
    if not args.quick:
        with open(args.out, "w") as fh:
            fh.write(HEADER.format(device=res["device"], repeats=args.repeats) + table + "\n" + FOOTER)
        print(f"wrote {args.out}")


HEADER = """# On-device baseline JPEG encoder (asva_amd/video_io.py:encode_jpeg_frames; kernels in csrc/jpeg.hip)

Tables written by `tools/jpeg_bench.py` on an MI355X (the runtime names it "{device}"), one session.  Wall times are
`time.perf_counter` around the call with a device synchronisation on either side, 2 warm-up calls, {repeats} repeats; the two
`ops` rows are device events around 20 back-to-back calls.  The encode inputs are synthetic frames (moving colour gradients plus
3 % noise), because random weights decode to noise; the clip rows encode what the randomly weighted VAE produced.  No test
carries a time threshold.
"""

FOOTER = """
## Reading the tables

The `"device"` files are larger than the `"host"` files because they are 4:4:4 and PIL's are 4:2:0 (the "PIL 4:4:4" row is the
like-for-like size), and the clip rows encode the noise a randomly weighted VAE decodes to, which compresses far worse than a
picture.  The wall time of `encode_jpeg_frames` is mostly host work and two synchronising copies: the four kernels together are the
sum of the kernel table.  The host figures depend on the CPU of the box.

## Not measured

Real decoded frames (no trained weights are available): the size ratios of the second table are for the synthetic frames only.  More than one
clip per forward.  Frame sizes other than 256 x 256.  One session on one box: the spread between sessions has not been measured.
"""

if __name__ == "__main__":
    main()
