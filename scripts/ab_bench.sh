#!/bin/bash
# A/B on ONE box (box-to-box variation is +-2 %, and on one box back-to-back runs of one binary still differ by a few % in a stage): every librtx_hip.so
# variant under rustracer_amd/csrc/_build/ab/ is copied over the library in turn and benched on the scenes given (default: all four), 2 timed frames each;
# REPS=n repeats the whole round n times (variants interleaved: a b c a b c ...) and scripts/ab_summary.py prints the medians.
# A variant NAME.so may come with NAME.env: KEY=VALUE lines, the environment of its runs (knobs read per scene, e.g. RTX_LDS_SPEC=0).
# Every run has a time limit (LIMIT seconds); the first run that fails or runs out of time ends the script - nothing more is started on that GPU.
# Usage (GPU box, repo root): [REPS=3] [STEPS=2] [LIMIT=300] bash scripts/ab_bench.sh [scene ...]
RESULTS=${RESULTS:-results}  # where the runs' outputs go
SCENES=${@:-cornell blob mis room}
REPS=${REPS:-1}
STEPS=${STEPS:-2}
LIMIT=${LIMIT:-300}
LIB=rustracer_amd/csrc/_build/librtx_hip.so
cp $LIB /tmp/orig_librtx_hip.so
mkdir -p $RESULTS/ab
rc=0
for rep in $(seq 1 $REPS); do
for v in rustracer_amd/csrc/_build/ab/*.so; do
  name=$(basename $v .so)
  cp $v $LIB
  vars=""; [ -f ${v%.so}.env ] && vars=$(grep -v '^#' ${v%.so}.env | xargs)
  for sc in $SCENES; do
    env $vars timeout -k 10 $LIMIT python bench.py --full --scene $sc --steps $STEPS --warmup 1 --no-cpu-baseline --headline-only --detail $RESULTS/ab/${name}_${sc}_$rep.json > $RESULTS/ab/${name}_${sc}_$rep.line 2> $RESULTS/ab/${name}_${sc}_$rep.err
    rc=$?
    if [ $rc -ne 0 ]; then echo "$name $sc rep $rep: exit $rc - stopping"; tail -5 $RESULTS/ab/${name}_${sc}_$rep.err; break 3; fi
    python scripts/ab_line.py $name $sc $RESULTS/ab/${name}_${sc}_$rep.json
  done
done
done
cp /tmp/orig_librtx_hip.so $LIB
python scripts/ab_summary.py
exit $rc
