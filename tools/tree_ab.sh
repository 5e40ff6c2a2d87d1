#!/bin/bash
# Whole-tree A/B on ONE box: the previous round's tree (built beside HEAD under _ab/<tag>/, see below) against this tree — step, 4 clips per
# forward, VAE decode, cfg 4 — alternating, so that a regression no switch-level A/B can see (round 4: an allocator change that cost the VAE
# decode 12 %) shows up before the round ends.  Run through gpurun from the repo root:
#     bash tools/tree_ab.sh r4 [reps]
# Prepare the other tree HERE (CPU box) first; _ab/ is git-ignored but travels to the GPU box:
#     mkdir -p _ab/r4 && git archive <previous round's commit> | tar -x -C _ab/r4 && (cd _ab/r4 && python -m asva_amd.build && rm -rf asva_amd/csrc/_obj*)
# Each tree runs its OWN bench.py / tools with its OWN library and tile table.
# STEPS / WARMUP (default 40 / 5) set the length of each bench run; HEADLINE_ONLY=1 times the headline step alone (plain bench.py, no
# 4-clip / VAE / cfg 4 legs) and also prints the mean and the spread (max - min) of each tree's runs.  The first run that fails or runs
# into its time limit ends the script.
TAG=${1:-r4}
REPS=${2:-3}
STEPS=${STEPS:-40}
WARMUP=${WARMUP:-5}
HEADLINE_ONLY=${HEADLINE_ONLY:-0}
cd "$GRAFT_REPO_ROOT" || exit 1
OLD=$GRAFT_REPO_ROOT/_ab/$TAG
[ -f $OLD/asva_amd/libavsd_hip.so ] || { echo "no built tree under _ab/$TAG"; exit 1; }
export TMPDIR=/tmp
ROWS=$(mktemp)
row() { python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
b=d.get('batched',{}); v=d.get('vae_decode',{})
print('$1 step %.2f steps/s (%.3f ms)   4 clips %s clip-steps/s   VAE %s clips/s' % (d['value'], d['ms_per_step'], b.get('value'), v.get('clips_per_s')))"; }
for i in $(seq $REPS); do
  for t in new old; do
    if [ $t = old ]; then D=$OLD; else D=$GRAFT_REPO_ROOT; fi
    if [ $HEADLINE_ONLY = 1 ]; then
      LEGS=""
    else
      F=$(grep -q -- '"--full"' $D/bench.py && echo --full)    # trees older than --full run every leg by default
      LEGS="$F --no-cpu-baseline --no-roofline --no-precise --also-clips 4"
    fi
    J=$(cd $D && timeout -k 10 600 python bench.py --steps $STEPS --warmup $WARMUP $LEGS 2>/dev/null) || { echo "$t: bench.py failed (exit $?)"; exit 1; }
    echo "$J" | row "$t($( [ $t = old ] && echo $TAG || echo HEAD))" | tee -a $ROWS
  done
done
if [ $HEADLINE_ONLY = 1 ]; then
  python - $ROWS <<'EOF'
import re, sys
runs = {}
for line in open(sys.argv[1]):
    m = re.match(r"(\w+)\((.*?)\) step ([\d.]+) steps/s \(([\d.]+) ms\)", line)
    runs.setdefault(m.group(1), []).append((float(m.group(3)), float(m.group(4))))
for t, r in runs.items():
    v, ms = [x[0] for x in r], [x[1] for x in r]
    print("%s: mean %.3f steps/s (%.4f ms per step), spread (max - min) %.3f steps/s over %d runs" % (t, sum(v) / len(v), sum(ms) / len(ms), max(v) - min(v), len(v)))
if "new" in runs and "old" in runs:
    mean = {t: sum(x[0] for x in r) / len(r) for t, r in runs.items()}
    spread = max(max(x[0] for x in r) - min(x[0] for x in r) for r in runs.values())
    gain = mean["new"] - mean["old"]
    print("new - old: %+.3f steps/s (%+.2f %%); 3 x larger spread = %.3f steps/s -> %s" % (gain, 100 * gain / mean["old"], 3 * spread, "counts" if gain > 3 * spread else "does not count"))
EOF
  exit 0
fi
for t in new old; do
  if [ $t = old ]; then D=$OLD; else D=$GRAFT_REPO_ROOT; fi
  (cd $D && timeout -k 10 900 python tools/cfg4_run.py 2>/dev/null | tail -1 | sed "s/^/$t cfg4: /") || exit 1
done
