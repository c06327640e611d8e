#!/bin/bash
# usage: tools/gpu_call.sh <tag> [what...]   (runs on the GPU machine from the repo root; everything lands in $TD_OUT_DIR/<tag>_*, default out/)
tag=$1; shift
R=$(pwd)
mkdir -p "${TD_OUT_DIR:-out}"
O=$(cd "${TD_OUT_DIR:-out}" && pwd)
for what in "$@"; do
  case $what in
    tests) timeout 1500 python -m pytest tests -m gpu -q --timeout 900 -p no:cacheprovider > $O/${tag}_pytest.log 2>&1; echo "pytest rc=$?" >> $O/${tag}_pytest.log ;;
    newtests) timeout 1200 python -m pytest tests/test_bench_shapes_gpu.py tests/test_fullsize_gpu.py tests/test_model_gpu.py tests/test_input_pipeline_gpu.py tests/test_optim_gpu.py -m gpu -q --timeout 900 -p no:cacheprovider > $O/${tag}_newtests.log 2>&1; echo "pytest rc=$?" >> $O/${tag}_newtests.log ;;
    sel) timeout 1500 python -m pytest $TD_PYTEST_SEL -m gpu -q --timeout 900 -p no:cacheprovider > $O/${tag}_sel.log 2>&1; echo "pytest rc=$?" >> $O/${tag}_sel.log ;;
    bench) timeout 600 python bench.py --full > $O/${tag}_bench.json 2> $O/${tag}_bench.err; echo "bench rc=$?" >> $O/${tag}_bench.err ;;
    benchfast) timeout 600 python bench.py --full --cpu-frames 0 > $O/${tag}_bench.json 2> $O/${tag}_bench.err; echo "bench rc=$?" >> $O/${tag}_bench.err ;;
    stats) (cd /tmp && export TMPDIR=/tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${tag}_stats -- python $R/bench.py --no-graph --steps 3 --warmup 2 --cpu-frames 0 --roofline-steps 1 --dedupe-steps 0 > $O/${tag}_stats.log 2>&1) ;;
    *) echo "unknown step $what" ;;
  esac
done
ls $O | grep "^${tag}_" > /dev/null && echo done
