#!/bin/bash
# as ab_train_size.sh with the batch scaled to 131072 / points.   tools/ab_train_size_b.sh <points> <variant> ...
PTS=$1; shift
for round in 1 2; do
for v in "$@"; do
  if [ "$v" = base ]; then unset SHW_LIB_PATH; else export SHW_LIB_PATH=$PWD/build/variants/libshw_hip_$v.so; fi
  python bench.py --mode train --steps 50 --warmup 20 --points $PTS --batch $((131072/PTS)) 2>/dev/null | python -c "import json,sys;d=json.loads(sys.stdin.read());print('$v', 'N=$PTS train ms/step %.4f' % d['ms_per_step'])"
done; done
