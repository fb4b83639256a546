#!/bin/bash
# Round-6 final call (after the dense pre-pass): the tree's GPU suite and smoke, its bench lines (the
# driver's default command and --steps 20 --warmup 5, twice), the NUTS
# iteration profiles (measurement build abrun/nprof) and the rocprofv3 passes
# of the bench command (tools/profile_r06.sh).
source tools/gpu_check.sh
run gpu_tests 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread || exit $?
run smoke 120 python -c "import __graft_entry__ as g; g.smoke()" || exit $?
run bench_default 400 python bench.py --full || exit $?
grep '^{' gpurun_out/bench_default.log | tail -n 1 > gpurun_out/bench_default_line.json
for r in 1 2; do
  run bench20 400 python bench.py --full --steps 20 --warmup 5 || exit $?
  grep '^{' gpurun_out/bench20.log | tail -n 1 >> gpurun_out/bench20_lines.jsonl
done
run nprof_cfg3 120 env GMCMC_LIB=abrun/nprof/libgmcmc.so python tools/probe_nuts_prof.py || exit $?
run nprof_dense 200 env MASS=dense GMCMC_LIB=abrun/nprof/libgmcmc.so python tools/probe_nuts_prof.py || exit $?
PMC_OUT=gpurun_out/pmc_r06b K=20 bash tools/profile_r06.sh
