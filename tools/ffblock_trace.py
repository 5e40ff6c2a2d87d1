"""The tail of the 320-channel transformer blocks from rocprofv3 kernel traces (rocpd sqlite) of an EAGER run (bench.py --no-graph:
launches appear in program order):
    python tools/ffblock_trace.py <trace of the three-launch form>.db <trace of the fused form>.db > profiles/ffblock_kernel_trace.md
Three-launch form: every nstream_kernel<320, 3, true> launch (the GEGLU projection of a 320-channel block) and the two launches right
after it, FF-out and proj_out.  Fused form: the ffblock_kernel launches."""
import re
import sys

from qattn_trace import launches, mean


def main():
    sep, fus = launches(sys.argv[1]), launches(sys.argv[2])
    rows = {"geglu": [], "ffout": [], "proj": []}
    names = {"geglu": set(), "ffout": set(), "proj": set()}
    for i, (name, us, grid) in enumerate(sep):
        if not name.startswith("nstream_kernel<320, 3, true>") or i + 2 >= len(sep):
            continue
        for key, (n, u, g) in zip(("geglu", "ffout", "proj"), sep[i:i + 3]):
            rows[key].append(u)
            names[key].add(f"{n[:48]} grid {g}")
    print("## Three-launch form: GEGLU projection and the two launches after it\n")
    print("| launch | launches | avg us | min us | kernel |")
    print("|---|---:|---:|---:|---|")
    for key, label in (("geglu", "GEGLU projection"), ("ffout", "FF-out + h"), ("proj", "proj_out + x")):
        v = rows[key]
        print(f"| {label} | {len(v)} | {mean(v):.2f} | {min(v) if v else float('nan'):.2f} | {'; '.join(sorted(names[key]))} |")
    total = [a + b + c for a, b, c in zip(rows["geglu"], rows["ffout"], rows["proj"])]
    print(f"| sum of the three | {len(total)} | {mean(total):.2f} | {min(total) if total else float('nan'):.2f} | |")
    print("\n## Fused form: ffblock_kernel<with proj_out>\n")
    print("| kernel | grid | launches | avg us | min us |")
    print("|---|---:|---:|---:|---:|")
    fg = {}
    for name, us, grid in fus:
        if name.startswith("ffblock_kernel<"):
            fg.setdefault((name, grid), []).append(us)
    for (name, grid), v in sorted(fg.items()):
        print(f"| `{name}` | {grid} | {len(v)} | {mean(v):.2f} | {min(v):.2f} |")
    left = [us for name, us, grid in fus if name.startswith("nstream_kernel<320, 3, true>")]
    print(f"\nnstream_kernel<320, 3, true> launches left in the fused run: {len(left)}")
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
