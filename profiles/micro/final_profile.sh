#!/bin/bash
# final measurement set of the round (run through gpurun from the repo root)
R=$GRAFT_REPO_ROOT
O=${PROFILE_OUT:-$R/profile_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
python3 $R/bench.py --full > $O/bench_final.json 2> $O/bench_final.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_final -- python3 $R/bench.py --full --steps 30 --warmup 6 --no-cpu-baseline --no-profile > $O/bench_under_rocprof.json 2> $O/prof_final.err
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py --mode eager --steps 6 --warmup 3 --no-cpu-baseline --no-profile > /dev/null 2> $O/pmc_fetch.err
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 $R/bench.py --mode eager --steps 6 --warmup 3 --no-cpu-baseline --no-profile > /dev/null 2> $O/pmc_write.err
python3 $R/profiles/pmc_traffic.py $O/pmc_fetch $O/pmc_write 9 > $O/pmc_traffic.json
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_mfma -- python3 $R/bench.py --mode eager --steps 6 --warmup 3 --no-cpu-baseline --no-profile > /dev/null 2> $O/pmc_mfma.err
python3 $R/profiles/pmc_mfma.py $O/pmc_mfma > $O/pmc_mfma.json; rm -rf $O/pmc_mfma
find $O/prof_final -name "*kernel_stats.csv" -exec cp {} $O/kernel_stats_final.csv \;
# keep the merge-back small: drop the raw traces
rm -rf $O/pmc_fetch $O/pmc_write
find $O/prof_final -name "*kernel_trace.csv" -delete
tail -c 600 $O/bench_final.json; echo; cat $O/pmc_traffic.json | head -12
# navigator loop (SURVEY f-1): bench line + kernel stats
cd /tmp
python3 $R/bench_nav.py --steps 6 --warmup 2 > $O/bench_nav_final.json 2> $O/bench_nav_final.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_nav -- python3 $R/bench_nav.py --steps 3 --warmup 1 --no-cpu-baseline --no-host-loop --no-profile > $O/bench_nav_under_rocprof.json 2> $O/prof_nav.err
find $O/prof_nav -name "*kernel_stats.csv" -exec cp {} $O/kernel_stats_nav.csv \;
find $O/prof_nav -name "*kernel_trace.csv" -delete
rm -f $O/prof_nav/*.db
tail -c 300 $O/bench_nav_final.json; echo
