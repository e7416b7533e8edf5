#!/usr/bin/env bash
# Collects the round profiles on a GPU box (from the repo root):
#   full bench line, rocprofv3 kernel stats of the same command, and the two PMC passes (FETCH_SIZE / WRITE_SIZE in
#   separate runs).  Outputs land in $O (default out/); copy the summaries into profiles/ (see DESIGN.md section 7).
set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${O:-out}; mkdir -p $O
rm -rf $O/prof $O/pmc_fetch $O/pmc_write
timeout -k 10 400 python bench.py --full > $O/bench_full.json 2> $O/bench_full.err
echo full done
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o p -- python3 bench.py --no-cpu-baseline --steps 20 --warmup 5 > $O/bench_rocprof.json 2> $O/bench_rocprof.err
echo stats done
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_fetch -o f -- python3 bench.py --full --no-cpu-baseline --steps 5 --warmup 3 > /dev/null 2> $O/pmc_f.err
echo fetch done
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_write -o w -- python3 bench.py --full --no-cpu-baseline --steps 5 --warmup 3 > /dev/null 2> $O/pmc_w.err
echo write done
python tools/summarize_profile.py $O/prof $O/kernel_stats.md "rocprofv3 --kernel-trace --stats -- python3 bench.py --no-cpu-baseline --steps 20 --warmup 5"
python tools/pmc_traffic.py $O/pmc_fetch $O/pmc_write $O/pmc_traffic
rm -rf $O/prof $O/pmc_fetch $O/pmc_write
ls $O
