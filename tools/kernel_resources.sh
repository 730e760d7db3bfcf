#!/bin/bash
# Registers, spills, LDS and occupancy of the kernels of one translation unit (compiler remarks; no GPU needed):
#   tools/kernel_resources.sh block|table|ray|raytrans|raydepth|raygrad|raytgrad|raygndiag|raytangent|rayttangent|gradord|raysort|rayplan|dense|assembly|query|main [name filter]     (main: vrt_kernels.hip, the frame set-up)
# raygrad, raytgrad and raygndiag list the ORDERED instantiations (units of their own) behind the others; gradord: the count pass, the sort and the reduction around them.
cd "$(dirname "$0")/../simd-gaussian-ray-tracing_amd/csrc" || exit 1
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-pass-failed -fno-slp-vectorize --cuda-device-only -Rpass-analysis=kernel-resource-usage"
case "$1" in
  block) SRC=vrt_block_kernel.hip; EXTRA="-DVRT_RENDER_ECMAX=6 -DVRT_RENDER_WPE=3 -mllvm -amdgpu-sched-strategy=max-ilp" ;;
  table) SRC=vrt_table_kernel.hip; EXTRA="" ;;
  ray) SRC=vrt_ray_kernel.hip; EXTRA="-mllvm -amdgpu-sched-strategy=max-ilp" ;;
  raytrans) SRC=vrt_ray_trans_kernel.hip; EXTRA="" ;;
  raydepth) SRC=vrt_ray_depth_kernel.hip; EXTRA="" ;;
  raygrad) SRC="vrt_ray_grad_kernel.hip vrt_ray_grad_ordered_kernel.hip"; EXTRA="" ;;
  raytgrad) SRC="vrt_ray_trans_grad_kernel.hip vrt_ray_trans_grad_ordered_kernel.hip"; EXTRA="" ;;
  raygndiag) SRC="vrt_ray_gn_diag_kernel.hip vrt_ray_gn_diag_ordered_kernel.hip"; EXTRA="" ;;
  raytangent) SRC=vrt_ray_tangent_kernel.hip; EXTRA="" ;;
  rayttangent) SRC=vrt_ray_trans_tangent_kernel.hip; EXTRA="" ;;
  gradord) SRC=vrt_grad_ordered_kernel.hip; EXTRA="" ;;
  raysort) SRC=vrt_ray_sort_kernel.hip; EXTRA="" ;;
  rayplan) SRC=vrt_ray_plan_kernel.hip; EXTRA="" ;;
  dense|assembly|query) SRC=vrt_$1_kernel.hip; EXTRA="" ;;
  *) SRC=vrt_kernels.hip; EXTRA="" ;;
esac
for src in $SRC; do
/opt/rocm/bin/hipcc $FLAGS $EXTRA -c $src -o /dev/null 2>&1 | grep -E "Function Name|VGPRs:|SGPRs:|Spill|ScratchSize|Occupancy|LDS Size" | sed 's/^.*remark: //' | paste - - - - - - - - | grep -E "${2:-.}" | sed 's/\[-Rpass-analysis=kernel-resource-usage\]//g' | cut -c1-400
done
