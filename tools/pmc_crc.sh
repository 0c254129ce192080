#!/bin/bash
# PMC counters of k_crc32 on the C2 workload (1 M x 4 KiB), which the bench runs
# with --full; PMC="..." selects the counters.  Results go to $OUT/pmcc (default
# prof_out/pmcc).
set -e
O=${OUT:-prof_out}/pmcc
mkdir -p $O
export TMPDIR=/tmp
timeout -s KILL 120 rocprofv3 --pmc ${PMC} --kernel-include-regex k_crc32 --output-format csv -d $O/r -o run -- \
   python3 bench.py --full --buffers 64 --no-cpu --no-inflate --verify 1 --steps 2 --warmup 1 > $O/r.json 2> $O/r.err
python3 - "$O" <<'PY'
import csv, glob, collections, sys
f = glob.glob(sys.argv[1] + "/r/**/*counter_collection.csv", recursive=True)[0]
d = collections.defaultdict(list)
for r in csv.DictReader(open(f)):
    d[r["Counter_Name"]].append(float(r["Counter_Value"]))
print({k: f"{sum(v)/len(v):.4g}" for k, v in sorted(d.items())})
PY
