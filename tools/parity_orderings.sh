#!/bin/bash
# the model-level parity tests under other arithmetic orderings -- the default build, and alternative libraries where they were built: the sigmoid-form GELU
# instead of the polynomials (bash tools/build_alt.sh sigm gemm_nt_dma.hip,gemm_nt_p8.hip,mlp_fused.hip,mlp_pipe.hip,mlp_wgrad.hip -DMVLT_GELU_POLY=0 -- the GEMM files whose epilogues
# carry GELU / GELU'): the tightest margins of each run.
#   bash tools/parity_orderings.sh > rNN_parity_orderings.txt
cd "${GRAFT_REPO_ROOT:-.}"
run() {
  echo "=== $1"
  env $2 python -m pytest tests/test_model_gpu.py tests/test_engine_gpu.py -m gpu -q 2>&1 | tail -1
  python tools/parity_report.py "$1" 2>/dev/null | sed -n '/# tightest margins/,$p' | head -7
}
run "default build" "MVLT_DUMMY=1"
for lib in ab/libmvlt_*.so; do
  [ -f "$lib" ] && run "alternative build ($lib)" "MVLT_HIP_LIB=$lib"
done
