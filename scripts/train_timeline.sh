#!/bin/bash
# kernel timeline of one training step at cfg-5's per-GPU size (bf16 operands) -> build/train_timeline/
cd "$(dirname "$0")/.."
R=$PWD; O=$R/build/train_timeline; mkdir -p $O; export PYTHONUNBUFFERED=1 TMPDIR=/tmp
(cd /tmp && timeout 500 rocprofv3 --kernel-trace --output-format csv -d $O/prof -o kt -- python $R/scripts/train_bench.py 1 250 256 3 16 > $O/run.log 2>&1 < /dev/null)
f=$(find $O/prof -name "*kernel_trace.csv" | head -1)
tail -2 $O/run.log
python scripts/train_timeline.py "$f" list > $O/timeline.txt 2>&1
head -45 $O/timeline.txt
rm -rf $O/prof
