# rocprofv3 collection recipe for profiles/: kernel stats of the default bench
# with all its legs (--full), then FETCH_SIZE and WRITE_SIZE in separate passes
# on one 4 GiB sub-batch.  Results go to $OUT/p (default prof_out/p).
set -e
O=${OUT:-prof_out}/p
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o run -- python3 bench.py --full --steps 1 --warmup 1 --cpu-seconds 6 > $O/bench_stats.json 2> $O/bench_stats.err
timeout -k 10 150 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/fetch -o run -- python3 bench.py --full --steps 1 --warmup 0 --buffers 4096 --no-cpu --verify 1 > $O/f.json 2> $O/f.err
timeout -k 10 150 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/write -o run -- python3 bench.py --full --steps 1 --warmup 0 --buffers 4096 --no-cpu --verify 1 > $O/w.json 2> $O/w.err
find $O -name "*.csv" | head -20
