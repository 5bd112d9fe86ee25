# Runs the render MLP's stamp diagnostic (scripts/microbench/mlp16s_stamps.hip: per-phase cycles and the
# in-kernel clock of mlp16s_kernel), built beforehand as scripts/microbench/mlp16s_stamps.  The log goes
# to $OUT (default prof_out/).
set -o pipefail
OUT=${OUT:-prof_out}
mkdir -p "$OUT"
timeout -k 10 200 ./scripts/microbench/mlp16s_stamps > "$OUT/stamps16s.log" 2>&1 || { echo "rc=$?"; cat "$OUT/stamps16s.log"; exit 1; }
cat "$OUT/stamps16s.log"
