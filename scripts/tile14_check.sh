# GPU: GEMM tile tests incl. the 64x32 gemm_mid tile, then the full bench (Llama-2-7B + the GPT-2-XL secondary)
O=${OUT_DIR:-${TMPDIR:-/tmp}/llmss_t14}
mkdir -p $O
T="--timeout 120 --timeout-method thread"
timeout -k 10 900 python -u -m pytest -x -q $T tests/test_kernels_gpu.py -k "tiled_variants or combine_in_launch or norm_fold or w8a8_mid or test_native_loaded" > $O/kernels.log 2>&1 &&
timeout -k 10 400 python bench.py --full --steps 5 --warmup 2 > $O/bench.log 2>&1
rc=$?; for f in $O/*.log; do echo "== $f"; tail -n 2 $f | cut -c1-300; done; exit $rc
