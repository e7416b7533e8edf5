#!/usr/bin/env bash
# Round-2 extra measurements (GPU box, from the repo root): slab sweep of the headline gradient step, the tag
# workload, the C3 PPO workload and its kernel stats.  Outputs land in $O (default out/; copy into profiles/).
set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${O:-out}; mkdir -p $O
timeout -k 10 200 python tools/sweep_slab.py > $O/r02_sweep_slab.txt 2> $O/sweep_slab.err
echo sweep done
timeout -k 10 200 python bench.py --workload tag > $O/r02_bench_tag.json 2> $O/tag.err
echo tag done
timeout -k 10 200 python bench.py --full --workload c3ppo --steps 10 --warmup 4 > $O/r02_bench_c3ppo.json 2> $O/c3ppo.err
echo c3ppo done
rm -rf $O/prof_c3
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_c3 -o p -- python3 bench.py --workload c3ppo --steps 5 --warmup 3 > $O/c3_rocprof.json 2> $O/c3_rocprof.err
python tools/summarize_profile.py $O/prof_c3 $O/r02_c3ppo_kernel_stats.md "rocprofv3 --kernel-trace --stats -- python3 bench.py --workload c3ppo --steps 5 --warmup 3"
rm -rf $O/prof_c3
cat $O/r02_sweep_slab.txt
