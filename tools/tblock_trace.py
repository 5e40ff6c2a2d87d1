"""The temporal attention of the 320-channel transformer blocks from rocprofv3 kernel traces (rocpd sqlite) of an EAGER run
(bench.py --no-graph: launches appear in program order):
    python tools/tblock_trace.py <trace of the three-launch form>.db <trace of the fused form>.db > profiles/tblock_kernel_trace.md
Three-launch form: every tattn_kernel<40, 12, false, true> launch (the temporal attention of a 320-channel block at 12 frames), the launch
right before it (the LayerNorm-folded q|k|v projection) and the one right after it (the output projection + h).  Fused form: the
tblock_kernel launches."""
import sys

from qattn_trace import launches, mean


def main():
    sep, fus = launches(sys.argv[1]), launches(sys.argv[2])
    keys = (("qkv", "q|k|v projection"), ("attn", "temporal attention"), ("out", "output projection + h"))
    rows = {k: [] for k, _ in keys}
    names = {k: set() for k, _ in keys}
    for i, (name, us, grid) in enumerate(sep):
        if not name.startswith("tattn_kernel<40, 12, false, true>") or i == 0 or i + 1 >= len(sep):
            continue
        for (key, _), (n, u, g) in zip(keys, sep[i - 1:i + 2]):
            rows[key].append(u)
            names[key].add(f"{n[:48]} grid {g}")
    print("## Three-launch form: the temporal attention at C = 320 and the launches around it\n")
    print("| launch | launches | avg us | min us | kernel |")
    print("|---|---:|---:|---:|---|")
    for key, label in keys:
        v = rows[key]
        print(f"| {label} | {len(v)} | {mean(v):.2f} | {min(v) if v else float('nan'):.2f} | {'; '.join(sorted(names[key]))} |")
    total = [a + b + c for a, b, c in zip(rows["qkv"], rows["attn"], rows["out"])]
    print(f"| sum of the three | {len(total)} | {mean(total):.2f} | {min(total) if total else float('nan'):.2f} | |")
    print("\n## Fused form: tblock_kernel\n")
    print("| kernel | grid | launches | avg us | min us |")
    print("|---|---:|---:|---:|---:|")
    fg = {}
    for name, us, grid in fus:
        if name.startswith("tblock_kernel"):
            fg.setdefault((name, grid), []).append(us)
    for (name, grid), v in sorted(fg.items()):
        print(f"| `{name}` | {grid} | {len(v)} | {mean(v):.2f} | {min(v):.2f} |")
    left = [us for name, us, grid in fus if name.startswith("tattn_kernel<40, 12, false, true>")]
    print(f"\ntattn_kernel<40, 12, false, true> launches left in the fused run: {len(left)}")
    print(f"launches in the traced run: three-launch form {len(sep)}, fused form {len(fus)} (difference {len(sep) - len(fus)})")
    count = {}
    for k, tr in enumerate((sep, fus)):
        for name, us, grid in tr:
            c = count.setdefault(name, [0, 0, 0.0, 0.0])
            c[k] += 1
            c[2 + k] += us
    print("\nkernels whose launch count differs (three-launch form -> fused form, total us):\n")
    for name, c in sorted(count.items()):
        if c[0] != c[1]:
            print(f"* `{name[:80]}`: {c[0]} -> {c[1]} launches, {c[2]:.0f} -> {c[3]:.0f} us")
    print()
    for label, tr in (("three-launch form", sep), ("fused form", fus)):
        print(f"kernel time of the traced run, {label}: {sum(u for _, u, _ in tr) / 1e3:.2f} ms")


if __name__ == "__main__":
    main()
