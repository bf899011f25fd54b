#!/bin/bash
# The compiler's resource table of the innovation-stream (INNOV) step kernels next to their twins without the stream, with the
# flags of csrc/Makefile (CPU only: hipcc cross-compiles).
#   bash tools/kres_innov.sh > profiles/r09_innov_kernel_resources.txt
cd "$(dirname "$0")/../target_estimation_amd/csrc"
echo "# hipcc -Rpass-analysis=kernel-resource-usage (tools/kres_innov.sh, tools/kres.py; flags of csrc/Makefile): every INNOV instantiation and its twin."
echo "# kf_step_sep_kernel<model,T,layout,INDEXED,FUSED,QUERY,PERQR,LIVE,AB,POSE,INNOV>; kf_step_population_kernel<T,QUERY,AB,POSE,SHARED,INNOV>"
echo "# (0/1 = false/true; layout 2 = axis-separable, 3 = axis-separable with packed groups, 4 = its shared-axes form; INNOV 0 is the twin)"
tmp=$(mktemp -d)
srcs="kf_model_uv kf_model_ua kf_model_ar kf_model_av kf_shared_uv kf_shared_ua kf_shared_ar kf_shared_av kf_innov_uv kf_innov_ua kf_innov_ar kf_innov_av \
kf_population_f64 kf_population_f32 kf_population_f64_shared kf_population_f64_innov kf_population_f32_innov kf_population_f64_shared_innov"
for f in $srcs; do
  extra=""
  case $f in kf_model_ar|kf_model_av|kf_innov_ar|kf_innov_av) extra="-mllvm -disable-machine-licm";; esac
  echo "/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $extra -c $f.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 | python3 ../../tools/kres.py kf_step > $tmp/$f.txt"
done | xargs -P 4 -I{} bash -c '{}'
# the dense single tick in place of every separable layout and the plain population tick, INNOV 0 (twin) and 1, side by side
cat "$tmp"/*.txt | grep -E "^kf_step_sep_kernel<[A-Z]+,[a-z]+,[234],0,0,0,0,0,0,0,[01]>|^kf_step_population_kernel<[a-z]+,0,0,0,[01],[01]>" | sort
rm -rf "$tmp"
