#!/bin/bash
# on the GPU box: gradient-kernel timing (and optionally the bench) for every built variant, interleaved twice
cd "$(dirname "$0")/.."
V=pantheonrl_amd/csrc/variants
for rep in 1 2; do
  for so in "$@"; do
    PANTHEON_HIP_LIB=$PWD/$V/$so.so python scripts/gradbench.py 2>&1 | tail -1 | sed "s/^/$so: /"
  done
done
if [ -n "$AB_BENCH" ]; then
  for so in "$@"; do
    PANTHEON_HIP_LIB=$PWD/$V/$so.so python bench.py --steps 20 --warmup 3 --full --no-cpu-baseline 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$so bench: %.2f M agent-steps/s, %.3f ms/iter, grad %.1f us' % (d['value']/1e6, d['ms_per_step'], d['roofline']['launch_ms']*1e3))"
  done
fi
if [ -n "$AB_TEST" ]; then
  for so in $AB_TEST; do
    PANTHEON_HIP_LIB=$PWD/$V/$so.so python -m pytest tests/test_gpu_parity.py -x -q -k "minibatch_gradient or train_matches or mfma_and_valu or train_full_size or train_single_row or early_stop or golden or joint_update or forward_matches" 2>&1 | tail -2 | sed "s/^/$so: /"
  done
fi
