"""Per-group cost of the cross-attentions below 32 x 32 from rocprofv3 kernel traces (rocpd sqlite) of an EAGER run
(bench.py --no-graph: launches appear in program order):
    python tools/qattn_trace.py <trace of the three-launch form>.db <trace of the fused form>.db > profiles/qattn_kernel_trace.md
Three-launch form: every audio / text attn_kernel<80 | 160, 1, gather> launch (a block runs first-frame attention, audio, text in that
order) and the launch right before it, which is its LayerNorm-folded Q projection.  Fused form: the qattn_kernel launches.  Groups are
told apart by head width, key gather (audio) and grid."""
import re
import sqlite3
import sys


def launches(path):
    db = sqlite3.connect(path)
    cur = db.cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    have = all(c in cols for c in ("grid_x", "grid_y", "grid_z", "workgroup_x", "workgroup_y", "workgroup_z"))
    gcol = "grid_x * grid_y * grid_z" if have else None
    wcol = "workgroup_x * workgroup_y * workgroup_z" if have else None
    sel = f"select {name_col}, start, end, {gcol or 0}, {wcol or 1} from kernels order by start"
    out = []
    for name, s, e, g, w in cur.execute(sel):
        name = re.sub(r"\(anonymous namespace\)::", "", name)
        name = re.sub(r"^void ", "", name)
        name = re.sub(r"\(.*", "", name)
        out.append((name, (e - s) / 1e3, int(g) // max(int(w), 1) if gcol else 0))     # grid in workgroups (rocprofv3 reports work items)
    return out


def mean(v):
    return sum(v) / len(v) if v else float("nan")


def main():
    sep, fus = launches(sys.argv[1]), launches(sys.argv[2])
    groups = {}
    after_audio = False        # a block runs first-frame attention, audio, text: an ungathered launch right after a gathered one is the text one
    for i, (name, us, grid) in enumerate(sep):
        m = re.match(r"attn_kernel<(80|160), 1, (true|false)>", name)
        if not m or i == 0:
            continue
        gather = m.group(2) == "true"
        text, after_audio = after_audio and not gather, gather
        if not gather and not text:
            continue           # first-frame attention
        g = groups.setdefault((int(m.group(1)), gather, grid), {"attn": [], "qproj": [], "qname": set()})
        g["attn"].append(us)
        g["qproj"].append(sep[i - 1][1])
        g["qname"].add(f"{sep[i - 1][0][:44]} grid {sep[i - 1][2]}")
    print("## Three-launch form: attention launch and the Q projection before it\n")
    print("| head width | keys | attention grid | launches | attn_kernel avg us | Q projection avg us | sum us | Q projection kernel |")
    print("|---|---|---:|---:|---:|---:|---:|---|")
    for (d, gather, grid), g in sorted(groups.items()):
        a, q = mean(g["attn"]), mean(g["qproj"])
        print(f"| {d} | {'audio (gathered)' if gather else 'text'} | {grid} | {len(g['attn'])} | {a:.2f} | {q:.2f} | {a + q:.2f} | {'; '.join(sorted(g['qname']))} |")
    left = {}
    for name, us, grid in fus:
        if re.match(r"attn_kernel<(80|160), 1, (true|false)>", name):
            left.setdefault((name, grid), []).append(us)
    fg = {}
    for name, us, grid in fus:
        if name.startswith("qattn_kernel<"):
            fg.setdefault((name, grid), []).append(us)
    print("\n## Fused form: qattn_kernel<C, D, BM, key tiles>\n")
    print("| kernel | grid | launches | avg us | min us |")
    print("|---|---:|---:|---:|---:|")
    for (name, grid), v in sorted(fg.items()):
        print(f"| `{name}` | {grid} | {len(v)} | {mean(v):.2f} | {min(v):.2f} |")
    if left:
        print("\nattention launches left in the fused run (first-frame attention, which runs the text template too; audio at 4 x 4):\n")
        for (name, grid), v in sorted(left.items()):
            print(f"* `{name}` grid {grid}: {len(v)} launches, avg {mean(v):.2f} us")
    print(f"\nlaunches in the traced run: three-launch form {len(sep)}, fused form {len(fus)} (difference {len(sep) - len(fus)})")


if __name__ == "__main__":
    main()
