"""Times the on-device sample-rate converter (asva_amd/audio_features.py:resample, kernel avsd_resample_sinc_f32) on an MI355X and
measures how far the host fallback filter (scipy.signal.resample_poly) is from it where it matters: in the normalised log-mel
spectrogram the audio encoder and the AVSync scorer consume.

  * ms per call for one 2 s mono clip at 44.1 -> 16, 48 -> 16 and 22.05 -> 16 kHz, and for one 10 s two-channel file at 44.1 kHz
    (waveform already on the device; device events around a run of back-to-back calls, warm-up, median of repeats);
  * rel-L2 between the waveforms, and between the normalised log-mel spectrograms (waveform_to_melspectrogram), of 2 s of white
    noise at amplitude 0.1 resampled by the device kernel and by resample_poly.

There is no speed gate and nothing to compare the times against: before this kernel there was no device path.

    python tools/resample_bench.py [--repeats 7] [--calls 50] [--out profiles/resample.md]
    python tools/resample_bench.py --quick          # one short pass, prints only
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from asva_amd import ops  # noqa: E402
from asva_amd.audio_features import resample, resample_taps, waveform_to_melspectrogram  # noqa: E402

RATES = (44100, 48000, 22050)


def timed(fn, repeats, calls, warmup=3):
    """median over `repeats` of the device time of `calls` back-to-back calls, per call, in ms"""
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
    return statistics.median(ms), min(ms), max(ms)


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.md"))
    args = ap.parse_args()
    if args.quick:
        args.repeats, args.calls = 2, 5
    from scipy.signal import resample_poly

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "calls_per_repeat": args.calls, "clip_2s": {}, "logmel": {}}
    for sr in RATES:
        x = (0.1 * torch.randn(1, 2 * sr, generator=g)).to(dev)
        taps, width, orig, new = resample_taps(sr, 16000)
        taps = torch.from_numpy(taps).to(dev)
        med, lo, hi = timed(lambda: resample(x, sr, 16000), args.repeats, args.calls)
        kern = timed(lambda: ops.resample_sinc_f32(x, taps, orig, new, width), args.repeats, args.calls)[0]
        res["clip_2s"][sr] = {"orig": orig, "new": new, "taps_per_output": 2 * width + orig, "ms": med, "ms_min": lo, "ms_max": hi,
                              "ms_launch_alone": kern}
    x10 = (0.1 * torch.randn(2, 10 * 44100, generator=g)).to(dev)
    taps, width, orig, new = resample_taps(44100, 16000)
    taps = torch.from_numpy(taps).to(dev)
    med, lo, hi = timed(lambda: resample(x10, 44100, 16000), args.repeats, args.calls)
    res["file_10s_2ch_44100"] = {"ms": med, "ms_min": lo, "ms_max": hi,
                                 "ms_launch_alone": timed(lambda: ops.resample_sinc_f32(x10, taps, orig, new, width), args.repeats, args.calls)[0]}
    for sr in RATES:
        noise = 0.1 * torch.randn(1, 2 * sr, generator=g)
        on_dev = resample(noise, sr, 16000, device=dev)
        k = math.gcd(sr, 16000)
        poly = torch.from_numpy(resample_poly(noise.numpy().astype(np.float64), 16000 // k, sr // k, axis=1).astype(np.float32)).to(dev)
        res["logmel"][sr] = {"waveform_rel_l2": rel_l2(poly, on_dev),
                             "logmel_rel_l2": rel_l2(waveform_to_melspectrogram(poly, device=dev), waveform_to_melspectrogram(on_dev, device=dev))}
    print(json.dumps(res))
    lines = ["", "| conversion | orig : new | taps per output | ms per call (median) | min – max | `ops.resample_sinc_f32` alone |",
             "|---|---|---|---|---|---|"]
    for sr in RATES:
        c = res["clip_2s"][sr]
        lines.append(f"| {sr} -> 16000 Hz, 2 s mono | {c['orig']} : {c['new']} | {c['taps_per_output']} | {c['ms']:.4f} | {c['ms_min']:.4f} – {c['ms_max']:.4f} | {c['ms_launch_alone']:.4f} |")
    f = res["file_10s_2ch_44100"]
    lines.append(f"| 44100 -> 16000 Hz, 10 s, two channels | 441 : 160 | 475 | {f['ms']:.4f} | {f['ms_min']:.4f} – {f['ms_max']:.4f} | {f['ms_launch_alone']:.4f} |")
    lines += ["", "| conversion | waveform rel-L2, resample_poly vs device | normalised log-mel rel-L2 |", "|---|---|---|"]
    for sr in RATES:
        m = res["logmel"][sr]
        lines.append(f"| {sr} -> 16000 Hz | {m['waveform_rel_l2']:.3e} | {m['logmel_rel_l2']:.3e} |")
    table = "\n".join(lines)
    print(table)
    print("log-mel difference between the two resamplers: see the second table")
    if not args.quick:
        with open(args.out, "w") as fh:
            fh.write(HEADER.format(device=res["device"], repeats=args.repeats, calls=args.calls) + table + "\n" + FOOTER)
        print(f"wrote {args.out}")


HEADER = """# On-device sample-rate conversion (asva_amd/audio_features.py:resample; kernel `avsd_resample_sinc_f32` in csrc/audio.hip)

Written by `tools/resample_bench.py` on an MI355X (the runtime names it "{device}"): device events around {calls} back-to-back calls of `resample` on a waveform that is
already on the device, 3 warm-up calls, median / min / max of {repeats} repeats.  One run of the tool: the spread between runs has not been
measured.  **There is nothing to compare these times against: before this kernel the repository had no device path for resampling**
(the host path is `scipy.signal.resample_poly` or torchaudio on the CPU, plus a copy in each direction), so there is no speed gate.

White noise, amplitude 0.1, 2 s, seeded.  The log-mel column is `waveform_to_melspectrogram` (128 x 204, normalised) of the two
16 kHz waveforms: what the ImageBind audio trunk and the AVSync scorer actually see of the difference between the two filters.
"""

FOOTER = """
Each call of `resample` is one launch of the resampling kernel plus the `to` / `contiguous` / `view` calls around it and the allocation
of the result; the last column is the launch with its output allocation alone (`ops.resample_sinc_f32` on prepared taps), same method.

## Not measured

torchaudio is not installed: the device filter is pinned to torchaudio's published definition and to closed-form answers
(tests/test_resample_cpu.py), not to torchaudio's output.  No real clip's conditioning has been compared between the two resamplers;
the white-noise figures above are the only ones.  No `rocprofv3` trace of the kernel has been taken.
"""

if __name__ == "__main__":
    main()
