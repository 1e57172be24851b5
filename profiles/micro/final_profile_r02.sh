#!/bin/bash
# round-2 measurement set (run through gpurun from the repo root): the default bench line, its rocprofv3 kernel stats (the exact
# driver command), the PMC traffic passes, the navigator-loop lines
R=$GRAFT_REPO_ROOT
O=${PROFILE_OUT:-$R/profile_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
python3 $R/bench.py --full > $O/r02_bench.json 2> $O/r02_bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/r02_prof -- python3 $R/bench.py --no-cpu-baseline --no-parity --no-secondary --no-profile > $O/r02_bench_under_rocprof.json 2> $O/r02_prof.err
find $O/r02_prof -name "*kernel_stats.csv" -exec cp {} $O/r02_kernel_stats.csv \;
find $O/r02_prof -name "*kernel_trace.csv" -delete
rm -f $O/r02_prof/*/*.db $O/r02_prof/*.db
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py --mode eager --steps 6 --warmup 3 --no-cpu-baseline --no-profile --no-parity --no-secondary > /dev/null 2> $O/r02_pmc_fetch.err
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 $R/bench.py --mode eager --steps 6 --warmup 3 --no-cpu-baseline --no-profile --no-parity --no-secondary > /dev/null 2> $O/r02_pmc_write.err
python3 $R/profiles/pmc_traffic.py $O/pmc_fetch $O/pmc_write 9 > $O/r02_pmc_traffic.json
rm -rf $O/pmc_fetch $O/pmc_write
tail -c 400 $O/r02_bench.json; echo; head -12 $O/r02_pmc_traffic.json
python3 $R/bench_nav.py --steps 6 --warmup 2 > $O/r02_bench_nav.json 2> $O/r02_bench_nav.err
python3 $R/bench_nav.py --icod --hidden 128 --teacher-hidden 768 --instr-min 20 --instr-max 80 --hops-min 4 --hops-max 7 --max-action-len 15 --no-cpu-baseline --no-host-loop > $O/r02_bench_nav_icod.json 2> $O/r02_bench_nav_icod.err
tail -c 300 $O/r02_bench_nav.json; echo; tail -c 300 $O/r02_bench_nav_icod.json; echo
