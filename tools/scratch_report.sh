#!/bin/bash
# Kernels of one HIP source (at a git revision, default: the working tree) that use scratch memory or spill registers.
# --all: one row for EVERY kernel instead -- VGPRs, AGPRs, SGPRs, scratch bytes per lane, spill counts, LDS bytes, occupancy (waves per
# SIMD), name -- the table to compare before and after a change to a kernel file (sort both, then diff).
# usage: tools/scratch_report.sh [--all] conv_igemm_ring.hip [rev]
set -e
ALL=0; if [ "$1" = --all ]; then ALL=1; shift; fi
R="$(cd "$(dirname "$0")/.." && pwd)"; S="$R/unsupervised_detection_amd/csrc"; T=$(mktemp -d)
if [ -n "$2" ]; then git -C "$R" archive "$2" unsupervised_detection_amd/csrc include | tar -x -C "$T"; S="$T/unsupervised_detection_amd/csrc"; fi
X=""; [ "$1" = conv_wino.hip ] && X="-fno-slp-vectorize"  # (the per-file flags of csrc/Makefile)
[ "$1" = conv_igemm_staged.hip ] && X="-mllvm -instcombine-max-copied-from-constant-users=4096"
if [ $ALL = 1 ]; then
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 $X --cuda-device-only --no-gpu-bundle-output -Rpass-analysis=kernel-resource-usage \
    -c "$S/$1" -o "$T/k.co" 2>&1 | grep "remark:" | sed -e 's/^.*remark: *//' -e 's/ *\[-Rpass.*$//' |
    awk -F': ' 'BEGIN { K["VGPRs"]="vgprs"; K["AGPRs"]="agprs"; K["TotalSGPRs"]="sgprs"; K["ScratchSize [bytes/lane]"]="scratch"; K["VGPRs Spill"]="vgpr_spill"
                        K["SGPRs Spill"]="sgpr_spill"; K["LDS Size [bytes/block]"]="lds"; K["Occupancy [waves/SIMD]"]="occupancy" }
                $1=="Function Name" { if (n != "") print r n; n=$2; r="" }
                ($1 in K) { r = r K[$1] " " $2 " " }
                END { if (n != "") print r n }' | c++filt | cut -c1-260
else
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 $X --cuda-device-only --no-gpu-bundle-output -c "$S/$1" -o "$T/k.co" 2> /dev/null
  /opt/rocm/lib/llvm/bin/llvm-readelf --notes "$T/k.co" | grep -E "^\s+\.name:|\.private_segment_fixed_size|\.vgpr_spill_count|\.sgpr_spill_count|\.vgpr_count" | paste - - - - - |
    awk '{ n=""; for (i=1;i<=NF;i++) { if ($i==".name:") n=$(i+1); if ($i==".private_segment_fixed_size:") p=$(i+1); if ($i==".vgpr_spill_count:") v=$(i+1); if ($i==".sgpr_spill_count:") s=$(i+1); if ($i==".vgpr_count:") c=$(i+1) } if (p+v+s > 0) print "scratch", p, "vgpr_spill", v, "sgpr_spill", s, "vgprs", c, n }' | c++filt | cut -c1-200
fi
rm -rf "$T"
