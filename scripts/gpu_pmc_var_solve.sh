# FETCH_SIZE / WRITE_SIZE passes (one eager step, validation solve and solve timing included) of
# library variants: scripts/gpu_pmc_var_solve.sh DIR ...   (DIR = a variant tree of build_variants.sh)
#   -> $OUT/pmcs_NAME.json (scripts/pmc_summary.py), NAME = basename of DIR; one summary line for
#      the CB SYRK each
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}
mkdir -p "$OUT"; export TMPDIR=/tmp
for d in "$@"; do
  v=$(basename "$d")
  for c in FETCH_SIZE WRITE_SIZE; do
    timeout -k 10 300 rocprofv3 --pmc $c --kernel-trace -f csv -d "$OUT/pmcs_${v}_$c" -o pmc -- \
      python3 "$d/bench.py" --full --graph 0 --steps 1 --warmup 0 --no-cpu-baseline > "$OUT/pmcs_${v}_$c.log" 2>&1 || exit 1
  done
  python3 scripts/pmc_summary.py "$OUT/pmcs_${v}_FETCH_SIZE" "$OUT/pmcs_${v}_WRITE_SIZE" > "$OUT/pmcs_$v.json" || exit 1
  python3 -c "
import json
d = json.load(open('$OUT/pmcs_$v.json'))['kernels']
for k, x in d.items():
    if 'syrk_mfma_kernel<128, 2, 4, 1, 0' in k: print('$v', k[:48], x['launches'], round(x['fetch_bytes_per_launch'] / 1e9, 3), round(x['write_bytes_per_launch'] / 1e9, 3))"
done
