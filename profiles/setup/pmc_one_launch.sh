#!/bin/bash
# One rocprofv3 counter pass (counters only, no tracing) over one C2 launch at a time
# (profiles/profile_kernel.py --kernel tile --iters 3, orders learned): the mean of the last three
# tile-pass dispatches per counter.
#   bash profiles/setup/pmc_one_launch.sh <name> <library> <out dir> COUNTER [COUNTER ...]
set -u
NAME=$1; LIB=$2; OUT=$3; shift 3
CFG=${PMC_CONFIG:-C2}
mkdir -p "$OUT"
export TMPDIR=/tmp
VR_LIBRARY=$(realpath "$LIB") timeout -s KILL 120 rocprofv3 --pmc "$@" -f csv -d "$OUT/$NAME" -o run -- \
    python3 profiles/profile_kernel.py --config "$CFG" --kernel tile --iters 3 > "$OUT/$NAME.log" 2>&1
rc=$?
if [ $rc -ne 0 ]; then echo "$NAME: counter pass failed rc=$rc"; tail -5 "$OUT/$NAME.log"; exit $rc; fi
python3 - "$OUT/$NAME" "$NAME" <<'PY'
import collections
import csv
import glob
import sys
agg = collections.defaultdict(list)
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "march_kernel" in r["Kernel_Name"]:
            agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
for k in sorted(agg):
    v = agg[k][-3:]
    print(f"{sys.argv[2]:14s} {k:28s} {sum(v) / len(v):.6g}   ({len(agg[k])} dispatches, mean of the last {len(v)})")
PY
