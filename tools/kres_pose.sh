#!/bin/bash
# The compiler's resource table of the pose-stream (POSE) step kernels next to their twins without poses, with the flags of
# csrc/Makefile (CPU only: hipcc cross-compiles).
#   bash tools/kres_pose.sh > profiles/r05_pose_kernel_resources.txt
cd "$(dirname "$0")/../target_estimation_amd/csrc"
echo "# hipcc -Rpass-analysis=kernel-resource-usage (tools/kres_pose.sh, tools/kres.py; flags of csrc/Makefile): every POSE instantiation and its twin."
echo "# kf_step_sep_kernel<model,T,layout,INDEXED,FUSED,QUERY,PERQR,LIVE,AB,POSE>; kf_step_population_kernel<T,QUERY,AB,POSE>"
echo "# (0/1 = false/true; layout 2 = axis-separable, 3 = axis-separable with packed groups; a name without the POSE argument is the twin)"
tmp=$(mktemp -d)
for f in kf_model_uv kf_model_ua kf_model_ar kf_model_av kf_population_f64 kf_population_f32 kf_population_f64_pose kf_population_f32_pose; do
  extra=""
  case $f in kf_model_ar|kf_model_av) extra="-mllvm -disable-machine-licm";; esac
  ( /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $extra -c $f.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 \
      | python3 ../../tools/kres.py kf_step > "$tmp/$f.txt" ) &
done
wait
for f in kf_model_uv kf_model_ua kf_model_ar kf_model_av kf_population_f64 kf_population_f32 kf_population_f64_pose kf_population_f32_pose; do
  # the separable kernels that have a POSE variant (dense single ticks, FUSED, QUERY, AB), then the POSE variants themselves
  grep -E "^kf_step_sep_kernel<[A-Z]+,[a-z]+,[23],0,[01],[01],0,0,[01],[01]>|^kf_step_population_kernel" "$tmp/$f.txt"
done
rm -rf "$tmp"
