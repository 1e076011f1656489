#!/bin/bash
# Score processors on the device: the parent commit's torch loop against this tree with and without
# --device_processors, alternating processes on one card, each leg twice; then the plain lines without processors and this tree's
# tools/gen_bench.py itself.  usage: tools/processors_ab.sh PARENT_ROOT [OUT] [beams]   (PARENT_ROOT: a built checkout of the parent commit)
# With `beams` as the third word: greedy beam search, 64 items x 5 beams, three trees -- the parent's host beam
# loop, this tree's default and this tree with --device_beam_processors -- each leg twice; then plain beam search without processors on
# both trees, as it runs and with KMB_GEN_HEAD_STATS=0 (the two-launch beam step the processed step is built on).
PARENT=${1:?usage: tools/processors_ab.sh PARENT_ROOT [OUT] [beams]}
OUT=${2:-processors_on_device_time.txt}
WHAT=${3:-one_beam}
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
if [ "$WHAT" = beams ]; then
  for round in 1 2; do
    run "beam search 64 x 5 + processors, parent (host beam loop), run $round" $T --root "$PARENT" --tag parent $P --num-beams 5
    run "beam search 64 x 5 + processors, this tree, default (host beam loop), run $round" $T --root . --tag this $P --num-beams 5
    run "beam search 64 x 5 + processors, this tree, --device_beam_processors, run $round" $T --root . --tag this $P --num-beams 5 --device_beam_processors
  done
  for round in 1 2; do
    run "plain beam search 64 x 5, parent, run $round" $T --root "$PARENT" --tag parent --batch 64 --max-length 20 --num-beams 5
    run "plain beam search 64 x 5, this tree, run $round" $T --root . --tag this --batch 64 --max-length 20 --num-beams 5
    run "plain beam search 64 x 5, KMB_GEN_HEAD_STATS=0, parent, run $round" env KMB_GEN_HEAD_STATS=0 $T --root "$PARENT" --tag parent --batch 64 --max-length 20 --num-beams 5
    run "plain beam search 64 x 5, KMB_GEN_HEAD_STATS=0, this tree, run $round" env KMB_GEN_HEAD_STATS=0 $T --root . --tag this --batch 64 --max-length 20 --num-beams 5
  done
  rm -f "$OUT.err"
  cat "$OUT"
  exit 0
fi
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
