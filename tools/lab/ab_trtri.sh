# A/B of NMGP_TRTRI on the 128-chain value+gradient step: bash tools/lab/ab_trtri.sh <output dir>
set -e
O=${1:?output dir}
mkdir -p "$O"
python -m pytest tests/test_gpu_variants.py -q -m gpu -x -k "blocked_triangular" > "$O/trtri_test.log" 2>&1 || { tail -40 "$O/trtri_test.log"; exit 1; }
tail -3 "$O/trtri_test.log"
for v in 0 1 0 1; do
  NMGP_TRTRI=$v python bench.py --full --chains 128 --grad --steps 4 --warmup 1 --hmc-samples 0 --no-cpu-baseline > "$O/g128_trtri$v.json" 2>"$O/err.log"
  python -c "import json;r=json.load(open('$O/g128_trtri$v.json'));print('TRTRI=$v', r['value'], r['config']['stage_ms'])"
done
