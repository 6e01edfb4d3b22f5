#!/bin/bash
# A/B of an environment knob on ONE box: bash scripts/ab_env.sh "VAR=value" scene... (first the default, then with the assignment), 2 timed frames each
RESULTS=${RESULTS:-results}  # where the runs' outputs go
KNOB=$1; shift
SCENES=${@:-cornell blob mis room}
mkdir -p $RESULTS/ab
for sc in $SCENES; do
  python bench.py --full --scene $sc --steps 2 --warmup 1 --no-cpu-baseline --headline-only --detail $RESULTS/ab/default_${sc}.json > $RESULTS/ab/default_${sc}.line 2> $RESULTS/ab/default_${sc}.err
  python scripts/ab_line.py default $sc $RESULTS/ab/default_${sc}.json
  env $KNOB python bench.py --full --scene $sc --steps 2 --warmup 1 --no-cpu-baseline --headline-only --detail $RESULTS/ab/knob_${sc}.json > $RESULTS/ab/knob_${sc}.line 2> $RESULTS/ab/knob_${sc}.err
  python scripts/ab_line.py "$KNOB" $sc $RESULTS/ab/knob_${sc}.json
done
