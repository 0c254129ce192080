# C3-shaped level-1 leg: rocprofv3 kernel stats of the full per-GPU shard
# (65536 x 1 MiB enwik-style) with the bench's --full legs (CRC-32, verification,
# CPU baseline), then FETCH_SIZE / WRITE_SIZE passes of one 16384 x 1 MiB launch
# (file names carry the launch shape bench.py looks up).  Results go to $OUT/c3
# (default prof_out/c3).
set -e
O=${OUT:-prof_out}/c3
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o run -- python3 bench.py --full --level 1 --kind enwik --buffers 65536 --steps 2 --warmup 1 --no-inflate --adler-buffers 0 > $O/bench_stats.json 2> $O/bench_stats.err
timeout -k 10 150 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/fetch -o run -- python3 bench.py --steps 1 --warmup 0 --level 1 --kind enwik --buffers 16384 > $O/f.json 2> $O/f.err
timeout -k 10 150 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/write -o run -- python3 bench.py --steps 1 --warmup 0 --level 1 --kind enwik --buffers 16384 > $O/w.json 2> $O/w.err
find $O -name "*.csv"
cat $O/bench_stats.json
