"""Times the on-device baseline JPEG decoder (asva_amd/video_io.py:decode_jpeg_frames; kernels in csrc/jpeg.hip) against PIL's
decoder plus the upload, for one 12 x 256 x 256 clip and for eight of them in one call, on one MI355X in one session.

  * files: PIL's own 4:2:0 at quality 95 (what `write_mjpeg_avi` stores by default) and the device encoder's 4:4:4 at quality 95,
    of the synthetic frames of tools/jpeg_bench.py.
  * "host" = PIL's decode of every frame + one upload of the stacked frames; "device" = decode_jpeg_frames: marker parsing,
    stuffing removal, table lookup, the one upload, three launches and the copy of the status words.  Wall time, median / min / max.
    The host-side preparation alone (parsing and stuffing removal) as its own row.
  * the bytes uploaded as a share of the raw frames, and the re-decoding rounds of phase B (ops.jpeg_decode_scan(return_rounds=True)),
    also over every allowed subsequence length.
  * per kernel by a `rocprofv3 --kernel-trace --stats` run of a child process per kind of file (--rocprof).

There is no speed gate: the numbers go to profiles/jpeg_decoder.md.

    python tools/jpeg_decode_bench.py [--repeats 9] [--rocprof] [--out profiles/jpeg_decoder.md]
    python tools/jpeg_decode_bench.py --quick              # one short pass, prints only
    python tools/jpeg_decode_bench.py --kernels-only 420   # what the rocprofv3 child runs: ten decodes of one clip, nothing else
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from jpeg_bench import clip_frames, fmt, pil_encode, wall  # noqa: E402

from asva_amd import ops, video_io  # noqa: E402

KINDS = {"420": "PIL 4:2:0, quality 95", "444": "device encoder 4:4:4, quality 95"}
SUBSEQ = (128, 256, 512, 1024, 2048, 4096)


def files(kind, clips):
    frames = clip_frames(T=12 * clips)
    if kind == "420":
        return pil_encode(frames), frames.nbytes
    return video_io.encode_jpeg_frames(torch.from_numpy(frames).cuda()), frames.nbytes


def pil_decode_upload(jpegs, dev):
    from PIL import Image

    return torch.from_numpy(np.stack([np.array(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs])).to(dev)


def prepare_only(jpegs):
    return [video_io.parse_jpeg(j)["scan"].replace(b"\xff\x00", b"\xff") for j in jpegs]


def decode_part(repeats):
    dev = torch.device("cuda", 0)
    res = {}
    for kind in KINDS:
        for clips in (1, 8):
            jpegs, raw = files(kind, clips)
            want = pil_decode_upload(jpegs, dev)
            counters = {}
            got = video_io.decode_jpeg_frames(jpegs, dev, counters=counters)
            r = {"frames": len(jpegs), "raw_bytes": raw, "file_bytes": sum(len(j) for j in jpegs), "upload_bytes": counters["upload_bytes"],
                 "rounds": counters["rounds"], "equal_to_pil": bool(torch.equal(got, want)),
                 "host_ms": wall(lambda: pil_decode_upload(jpegs, dev), repeats),
                 "device_ms": wall(lambda: video_io.decode_jpeg_frames(jpegs, dev), repeats),
                 "prepare_ms": wall(lambda: prepare_only(jpegs), repeats)}
            if clips == 1:
                r["sweep"] = {}
                for s in SUBSEQ:
                    c = {}
                    video_io.decode_jpeg_frames(jpegs, dev, subseq_bits=s, counters=c)
                    r["sweep"][s] = {"rounds_max": max(c["rounds"]), "ms": wall(lambda: video_io.decode_jpeg_frames(jpegs, dev, subseq_bits=s), repeats)}
            res[f"{kind}x{clips}"] = r
    return res


def kernels_only(kind):
    dev = torch.device("cuda", 0)
    jpegs, _ = files(kind, 1)
    for _ in range(10):
        video_io.decode_jpeg_frames(jpegs, dev)
    torch.cuda.synchronize()


def rocprof_part(kind):
    """per-kernel device time of ten decodes of one clip, from a rocprofv3 kernel trace of a child process"""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="jpeg_dec_rocprof_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--kernels-only", kind]
        r = subprocess.run(["timeout", "-k", "10", "240", *cmd], capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            return {"error": f"rocprofv3 exited with {r.returncode}: {r.stderr[-500:]}"}
        rows = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    m = re.search(r"jpeg_(decode_scan|idct|colour)_kernel", row.get("Name", ""))
                    if m:
                        rows[m.group(0)] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                            "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        return rows or {"error": "no decoder kernels in the trace"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernels-only", choices=tuple(KINDS))
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decoder.md"))
    args = ap.parse_args()
    if args.kernels_only:
        kernels_only(args.kernels_only)
        return
    res = {"device": torch.cuda.get_device_name(0), "default_subseq_bits": ops.JPEG_SUBSEQ_BITS, "decode": decode_part(2 if args.quick else args.repeats)}
    d = res["decode"]
    lines = ["", "| files | frames | PIL decode + upload, ms | `decode_jpeg_frames`, ms | of which parsing and stuffing removal, ms | equal to PIL |",
             "|---|---|---|---|---|---|"]
    for key, r in d.items():
        kind, clips = key.split("x")
        lines.append(f"| {KINDS[kind]}, {clips} clip(s) | {r['frames']} | {fmt(r['host_ms'])} | {fmt(r['device_ms'])} | {fmt(r['prepare_ms'])} | "
                     f"{'yes' if r['equal_to_pil'] else '**no**'} |")
    lines += ["", "| files | raw frame bytes | file bytes | bytes uploaded by `decode_jpeg_frames` | re-decoding rounds per frame: median, max |", "|---|---|---|---|---|"]
    for key, r in d.items():
        kind, clips = key.split("x")
        lines.append(f"| {KINDS[kind]}, {clips} clip(s) | {r['raw_bytes']} | {r['file_bytes']} | {r['upload_bytes']} "
                     f"({100 * r['upload_bytes'] / r['raw_bytes']:.1f} % of raw) | {statistics.median(r['rounds']):g}, {max(r['rounds'])} |")
    lines += ["", "| one clip, subsequence length in bits | " + " | ".join(str(s) for s in SUBSEQ) + " |", "|---|" + "---|" * len(SUBSEQ)]
    for kind in KINDS:
        sw = d[f"{kind}x1"]["sweep"]
        lines.append(f"| {KINDS[kind]}: `decode_jpeg_frames` ms, median | " + " | ".join(f"{sw[s]['ms']['median']:.3f}" for s in SUBSEQ) + " |")
        lines.append(f"| {KINDS[kind]}: most re-decoding rounds of a frame | " + " | ".join(str(sw[s]["rounds_max"]) for s in SUBSEQ) + " |")
    if args.rocprof and not args.quick:
        res["rocprof"] = {kind: rocprof_part(kind) for kind in KINDS}
        lines += ["", "| kernel (rocprofv3 kernel trace, ten decodes of one clip in a child process) | files | calls | average µs | min – max µs |",
                  "|---|---|---|---|---|"]
        for kind, rows in res["rocprof"].items():
            if "error" in rows:
                lines.append(f"| not collected: {rows['error']} | {KINDS[kind]} | | | |")
            else:
                for name, k in sorted(rows.items()):
                    lines.append(f"| `{name}` | {KINDS[kind]} | {k['calls']} | {k['avg_us']:.1f} | {k['min_us']:.1f} – {k['max_us']:.1f} |")
    print(json.dumps(res))
    table = "\n".join(lines)
    print(table)
    if not args.quick:
        with open(args.out, "w") as fh:
            fh.write(HEADER.format(device=res["device"], repeats=args.repeats, default=ops.JPEG_SUBSEQ_BITS) + table + "\n" + FOOTER)
        print(f"wrote {args.out}")


HEADER = """# On-device baseline JPEG decoder (asva_amd/video_io.py:decode_jpeg_frames; kernels in csrc/jpeg.hip)

Tables written by `tools/jpeg_decode_bench.py` on an MI355X (the runtime names it "{device}"), one session.  Wall times are
`time.perf_counter` around the call with a device synchronisation on either side, 2 warm-up calls, {repeats} repeats, median (min – max).
The frames are the synthetic ones of `tools/jpeg_bench.py` (moving colour gradients plus 3 % noise), 256 x 256, 12 per clip; the
default subsequence length is {default} bits.  No test carries a time threshold, and the decoder is off by default.
"""

FOOTER = """
## Reading the tables

`decode_jpeg_frames` is host work (marker parsing, `bytes.replace` for the stuffing, building one buffer), one upload, three launches
and one synchronising copy of the status words; the kernels alone are the last table.  The entropy decoder runs one workgroup per
frame, so one clip occupies 12 of the 256 compute units: its time is the latency of one frame's decode, and more frames in a call
cost little more until the frames outnumber the compute units.  The re-decoding rounds are what the bit position, the block index
inside the MCU and the zigzag index need to agree between neighbouring subsequences; the bit position agrees within a few symbols,
the other two only at the next block both decoders end together, so busy content needs more rounds than the two or three of the
bit position alone.  The host figures depend on the CPU of the box.

## Not measured

Real decoded frames (no trained weights are available).  Frame sizes other than 256 x 256.  The evaluation driver end to end with
either decoder.  One session on one box: the spread between sessions has not been measured.
"""

if __name__ == "__main__":
    main()
