# the flow kernel with 16 and 32 columns per workgroup side by side on one box; usage (GPU box):
# bash scripts/flow_matrix.sh "64 64" "128 64" "128 128"
for sz in "$@"; do
  for cw in 16 32; do
    echo -n "cw $cw  "
    TSX_PCS_CFG=4,16,$cw SHARD_MODES=wrap timeout 300 python scripts/shard_study.py $sz 64 2>&1 | grep -v amdgpu.ids
  done
done
