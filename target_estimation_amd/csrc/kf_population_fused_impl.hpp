// kf_population_fused_impl.hpp -- included by the kf_population_fused*.hip translation units: the host side of
// kf_step_population_fused_kernel (kf_step_sep.hpp), one launch for a temporally fused replay of a whole population.  Every
// instantiation <T, GATE, DTTAB> holds the multi-tick loops of all four motion models and lives in a unit of its own
// (kf_population_fused_f{64,32}{,_gate}{,_dt}.hip) so that the build stays parallel; kf_population_fused.hip holds the launcher.
#pragma once
#include "dt_schedule.hpp"
#include "kf_ops_impl.hpp"
#include "kf_population.hpp"

namespace te {

// one launch of kf_step_population_fused_kernel<T, GATE, DTTAB>: defined (as an explicit specialisation) in that instantiation's unit
template <typename T, bool GATE, bool DTTAB>
void launch_population_fused_grid(const PopulationFusedArgs<T>& p, unsigned blocks, unsigned wpb, hipStream_t s);

#define TE_POPULATION_FUSED_DECL_(T_)                                                                                       \
  template <> void launch_population_fused_grid<T_, false, false>(const PopulationFusedArgs<T_>&, unsigned, unsigned, hipStream_t); \
  template <> void launch_population_fused_grid<T_, false, true>(const PopulationFusedArgs<T_>&, unsigned, unsigned, hipStream_t);  \
  template <> void launch_population_fused_grid<T_, true, false>(const PopulationFusedArgs<T_>&, unsigned, unsigned, hipStream_t);  \
  template <> void launch_population_fused_grid<T_, true, true>(const PopulationFusedArgs<T_>&, unsigned, unsigned, hipStream_t);
TE_POPULATION_FUSED_DECL_(double)
TE_POPULATION_FUSED_DECL_(float)
#undef TE_POPULATION_FUSED_DECL_

#define TE_POPULATION_FUSED_UNIT(T_, GATE_, DTTAB_)                                                                                    \
  template <>                                                                                                                          \
  void launch_population_fused_grid<T_, GATE_, DTTAB_>(const PopulationFusedArgs<T_>& p, unsigned blocks, unsigned wpb, hipStream_t s) { \
    static_assert(population_fused_ok(sizeof(T_) == 8, GATE_, DTTAB_), "not a shipped instantiation (step_variant.hpp)");              \
    hipLaunchKernelGGL((kf_step_population_fused_kernel<T_, GATE_, DTTAB_>), dim3(blocks), dim3(64 * wpb), 0, s, p);                   \
  }

}  // namespace te
