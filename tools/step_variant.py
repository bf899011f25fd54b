"""The step kernels' variant word (target_estimation_amd/csrc/step_variant.hpp) as names, for the tools that print or build
kernel names: kf_step_sep_kernel<model, T, layout, VAR>, kf_step_kernel<model, T, lanes per target, layout, VAR>,
kf_step_population_kernel<T, shared, VAR>.  tests/test_step_variant_host.py holds this table to the header."""
import re

BITS = {"INDEXED": 1 << 0, "FUSED": 1 << 1, "QUERY": 1 << 2, "PERQR": 1 << 3, "AB": 1 << 4, "POSE": 1 << 5, "INNOV": 1 << 6}
LIVE_SHIFT = 7   # a two-bit field: LIVE1 resident, LIVE2 resident with the per-tick query / pose output


def variant_name(v):
    """258 -> 'FUSED|LIVE2'; 0 -> '0'"""
    names = [n for n, b in BITS.items() if v & b]
    live = (v >> LIVE_SHIFT) & 3
    if live:
        names.append("LIVE%d" % live)
    return "|".join(names) if names else "0"


def variant_word(*names):
    """('FUSED', 'LIVE2') -> 258"""
    return sum((int(n[4:]) << LIVE_SHIFT) if n.startswith("LIVE") else BITS[n] for n in names)


def name_variants(kernel):
    """'kf_step_sep_kernel<te::ModelUV, double, 3, 258u>' -> '...<te::ModelUV, double, 3, FUSED|LIVE2>' (other names pass).
    c++filt and rocprofv3 print an unsigned template argument as `258u`; a bare `258` is taken too.  The gated kernels
    (kf_step_sep_gate_kernel<model, T, layout>, kf_step_population_gate_kernel<T, shared>) and the fused kernels with a time-step
    table (kf_step_sep_fused_dt_kernel<model, T, layout>) carry no variant word and pass."""
    return re.sub(r"(kf_step(?!\w*_gate_)(?!\w*_fused_dt_)\w*kernel<[^>]*?,\s*)(\d+)u?>", lambda m: m.group(1) + variant_name(int(m.group(2))) + ">", kernel)
