#!/bin/bash
# The compiler's resource table of every step kernel of the library (CPU only: hipcc cross-compiles): the `listings` target of
# csrc/Makefile over every kernel unit, each with its own flags, summarised by tools/kres.py.
#   bash tools/kres_all.sh [name filter, default kf_step] > profiles/<round>_kernel_resources.txt
# A feature's kernels next to their twins: filter the table, e.g.  | grep -E ",(0|POSE|FUSED|FUSED\|POSE)>"
set -e -o pipefail
here="$(cd "$(dirname "$0")" && pwd)"
lst="$(mktemp -d)"
trap 'rm -rf "$lst"' EXIT
make -C "$here/../target_estimation_amd/csrc" -j"${JOBS:-8}" listings LST="$lst" >&2
echo "# hipcc -Rpass-analysis=kernel-resource-usage, every ${1:-kf_step}* instantiation of the library (tools/kres_all.sh, tools/kres.py; flags of csrc/Makefile)."
echo "# kf_step_sep_kernel<model,T,layout,variant>; kf_step_kernel<model,T,G,layout,variant>; kf_step_population_kernel<T,shared-axes form,variant>;"
echo "# variant: tools/step_variant.py, 0 = the plain tick  (lds = static LDS per workgroup: resident kernels are one wavefront per workgroup)"
for f in "$lst"/*.kres; do
  python3 "$here/kres.py" "${1:-kf_step}" < "$f"
done
