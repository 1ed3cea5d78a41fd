cd /root/repo
out=${1:?usage: tools/run_r6_final.sh OUTDIR}; mkdir -p "$out"
timeout 1500 python -m pytest tests -m gpu -q > $out/r06_gputest.txt 2>&1; tail -3 $out/r06_gputest.txt
timeout 1500 python -m pytest tests -m gpu -q --conv-bf16x3 > $out/r06_gputest_conv_bf16x3.txt 2>&1; tail -3 $out/r06_gputest_conv_bf16x3.txt
bash tools/profile_r06.sh > $out/r06_profile.log 2>&1; tail -5 $out/r06_profile.log
python bench.py --full > $out/r06_bench_line.json 2> $out/r06_bench_line.err; tail -2 $out/r06_bench_line.err
python tools/bench_pose_solve.py > $out/r06_pose_solve_ab.txt 2>&1
python tools/bench_lookup_conv.py > $out/r06_lookup_conv_ab.txt 2>&1
