#!/bin/bash
# GPU box: run the GPU parity suite and the exact-reference tests against the MUTANT builds (make -C gym_cloth_amd/csrc mutants: 1-5 one ordering rule of
# the reference broken in each, 6-9 one value of the metrics wrong in each, 10-12 one value of both rasterisers wrong in each, 13-16 one value of both grabs wrong in each) and record which tests
# reject which mutant -> $OUT/summary.txt (copied to profiles/r06_mutation.txt; mutants 6-9 on the two metrics files: profiles/metrics_mutation.txt;
# mutants 10-12 on the two exact-render files: profiles/render_mutation.txt; mutants 13-16 on the gripper files: profiles/gripper_mutation.txt).
#   bash tools/run_mutants.sh            every mutant must fail at least one test; a surviving mutant means a missing test
#   MUTANTS="6 7 8 9" SEL="tests/test_gpu_metrics_exact.py tests/test_metrics_exact_host.py" bash tools/run_mutants.sh     some mutants, some files
#   MUTANTS="10 11 12" SEL="tests/test_gpu_render_exact.py tests/test_render_exact_host.py" bash tools/run_mutants.sh
#   MUTANTS="13 14 15 16" SEL="tests/test_gpu_gripper_exact.py tests/test_gpu_gripper.py tests/test_gripper_exact_host.py" bash tools/run_mutants.sh
# A run that ends in a time limit (124, 137), an abort (134) or a segmentation fault (139) ends the loop: nothing more is started on that GPU.
OUT=gpurun_out/mutants; mkdir -p $OUT
SEL=${SEL:-'tests/test_gpu_parity.py tests/test_gpu_fullsize.py tests/test_gpu_lean.py tests/test_gpu_large2.py tests/test_gpu_soak.py tests/test_gpu_env.py tests/test_gpu_fused.py tests/test_gpu_refpins.py tests/test_gpu_early_walk.py tests/test_gpu_window_flags.py tests/test_gpu_metrics_exact.py tests/test_metrics_exact_host.py tests/test_gpu_render_exact.py tests/test_render_exact_host.py tests/test_gpu_gripper_exact.py tests/test_gpu_gripper.py tests/test_gripper_exact_host.py'}
MUTANTS=${MUTANTS:-'1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16'}
DESC=("" "1: ONE particle adds two of its incident springs in swapped list order (Hooke, cloth.pyx:221-237)"
         "2: the first two visits of a collision cell swapped (cloth.pyx:324-343)"
         "3: the second over-stretched spring of a pass committed with the first whether or not it depends on it (cloth.pyx:265-296)"
         "4: the both-pinned skip of the strain limit dropped (cloth.pyx:268)"
         "5: the early walk (eight-wave fp32 LEAN build) jumps over a tested window without looking at its flag bit (cloth.pyx:265-296)"
         "6: metrics: the sort of the clipped points drops its y tie-break (cloth_metrics.hpp)"
         "7: metrics: the upper x / y out-of-bounds test is > instead of >= (cloth_env.py:1031, :1033)"
         "8: metrics: the height count tests z <= thickness/2 instead of < (cloth_env.py:606)"
         "9: metrics: y is not clipped to [0, 1] before the hull (cloth_env.py:629)"
         "10: render: edge e0 owns the centres on it when it is a right or a bottom edge (both rasterisers; the rule is top-left)"
         "11: render: depth mixed from the vertices' d instead of their 1 / d (both rasterisers)"
         "12: render: the pixel centre taken at + 0.0 instead of + 0.5 (both rasterisers)"
         "13: gripper: the cylinder test dx^2 + dy^2 < radius is <= (both grabs; gripper.pyx:35)"
         "14: gripper: the band test |z - level| < 2 thickness is <= (both grabs; gripper.pyx:36)"
         "15: gripper: the level search keeps the LAST level that hits, not the first (both grabs; gripper.pyx:33-41)"
         "16: gripper: the force_grab radius is accumulated in the handle's type, not in double (the launch's grab; cloth_env.py:439)")
: > $OUT/summary.txt
echo "# pytest -m gpu ($SEL) against libclothhip_mut{$MUTANTS}.so: tests that FAIL = tests that reject the mutant. f32-only = the failing tests whose id carries f32 / lean." >> $OUT/summary.txt
echo "# control: the production library passes all of them (GPUTEST)." >> $OUT/summary.txt
for k in $MUTANTS; do
  lib=$PWD/gym_cloth_amd/libclothhip_mut$k.so
  [ -f $lib ] || { echo "mutant $k: library missing" >> $OUT/summary.txt; continue; }
  CLOTHHIP_LIB=$lib timeout -k 10 900 python -m pytest $SEL -m gpu -q -p no:cacheprovider -o addopts="" --timeout 600 > $OUT/mut$k.log 2>&1
  rc=$?
  nf=$(grep -c "^FAILED" $OUT/mut$k.log); np=$(tail -1 $OUT/mut$k.log)
  echo "== mutant ${DESC[$k]}" >> $OUT/summary.txt
  echo "   $np" >> $OUT/summary.txt
  echo "   failing tests: $nf, of them fp32: $(grep "^FAILED" $OUT/mut$k.log | grep -ci "f32\|lean\|float")" >> $OUT/summary.txt
  grep "^FAILED" $OUT/mut$k.log | sed 's/ - .*//' | sed 's/^/     /' >> $OUT/summary.txt
  case $rc in
    124|137|134|139) echo "   pytest ended with status $rc (time limit / abort / segmentation fault): stopping here, no further library is run" >> $OUT/summary.txt
                     cat $OUT/summary.txt; exit $rc;;
  esac
done
cat $OUT/summary.txt
