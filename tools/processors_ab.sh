#!/bin/bash
# Score processors on the device: the parent commit's torch loop against this tree with and without
# --device_processors, alternating processes on one card, each leg twice; then the plain lines without processors and this tree's
# tools/gen_bench.py itself.  usage: tools/processors_ab.sh PARENT_ROOT [OUT]   (PARENT_ROOT: a built checkout of the parent commit)
PARENT=${1:?usage: tools/processors_ab.sh PARENT_ROOT [OUT]}
OUT=${2:-processors_on_device_time.txt}
cd "$(dirname "$0")/.." || exit 1
: > "$OUT"
date -u +"date: %Y-%m-%dT%H:%M:%SZ" >> "$OUT"
rocm-smi --showclocks 2>/dev/null | grep -E "sclk|mclk" | head -2 >> "$OUT"
run() {   # label, command...: one process under its own time limit; nothing more is started after a failure
  label=$1; shift
  echo "# $label" >> "$OUT"
  timeout -k 10 240 "$@" 2> "$OUT.err" | grep '^{' >> "$OUT"
  rc=${PIPESTATUS[0]}
  if [ "$rc" -ne 0 ]; then tail -n 20 "$OUT.err"; echo "stopping after: $label (exit $rc)"; exit "$rc"; fi
}
T="python tools/processors_time.py"
P="--batch 64 --max-length 20 --repetition-penalty 1.2 --no-repeat-ngram 3"
S="--do-sample --num-gen 5 --top-k 50 --top-p 0.9"
for mode in "" "$S"; do
  kind=greedy; [ -n "$mode" ] && kind=sampling
  for round in 1 2; do
    run "$kind + processors, parent (torch loop), run $round" $T --root "$PARENT" --tag parent $P $mode
    run "$kind + processors, this tree, default (torch loop), run $round" $T --root . --tag this $P $mode
    run "$kind + processors, this tree, --device_processors, run $round" $T --root . --tag this $P $mode --device_processors
  done
done
for round in 1 2; do
  run "plain greedy, parent, run $round" $T --root "$PARENT" --tag parent --batch 64 --max-length 20
  run "plain greedy, this tree, run $round" $T --root . --tag this --batch 64 --max-length 20
  run "plain sampling, parent, run $round" $T --root "$PARENT" --tag parent --batch 64 --max-length 20 $S
  run "plain sampling, this tree, run $round" $T --root . --tag this --batch 64 --max-length 20 $S
done
run "tools/gen_bench.py --beams 1 + processors, this tree, default" python tools/gen_bench.py --beams 1 $P
run "tools/gen_bench.py --beams 1 + processors, this tree, --device_processors" python tools/gen_bench.py --beams 1 $P --device_processors
run "tools/gen_bench.py sampling + processors, this tree, --device_processors" python tools/gen_bench.py --beams 1 $P $S --no-host --device_processors
rm -f "$OUT.err"
cat "$OUT"
