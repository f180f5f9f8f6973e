#!/bin/bash
# usage: ab_env.sh "<bench arguments>" ...   one bench line per setting, e.g.
#   bash tools/ab_env.sh "" "--variant side_blur=3" "--variant desc=separate --variant side_blur=2"
cd $GRAFT_REPO_ROOT
O=${AB_OUT:-/tmp/ab}   # one bench line (.json) and its stderr (.err) per setting
mkdir -p "$O"
i=0
for e in "$@"; do
  i=$((i+1))
  python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-end-to-end --no-density-sweep --no-extra-configs $e $AB_ARGS > "$O/env$i.json" 2> "$O/env$i.err"
  python -c "
import json
d=json.load(open('$O/env$i.json')); print('[$e]', d['value'], d['ms_per_step'], d['stages_ms'], d.get('stages_ms_in_step'))"
done
