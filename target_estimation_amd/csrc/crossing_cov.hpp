// crossing_cov.hpp -- host side of crossing_cov_kernel (crossing_cov.hip): the position covariance Sigma = (A(tau) P A(tau)^T + Q)[0:3, 0:3]
// of a target at its sphere crossing, tau = delta + dq, and from it the radial spread sigma_r and the first-order spread sigma_t of
// the crossing time (target_batch_c.h, target_batch_crossing_cov_dev).  One launch, a thread per row, records
// read-only through the layout's accessors; a row whose delta is no candidate costs its delta (and, in the rows form, its slot).
#pragma once
#include <hip/hip_runtime.h>

#include "crossing_cov_plan.hpp"
#include "te_clock.hpp"

namespace te {

struct CrossingCovArgs {
  char* rec;                 // the records as stored (read, never written)
  const void* qr;            // the batch's [Q | R] row in its precision, or (cls != null) its table of rows
  const int* cls;            // per-slot parameter class, or null
  const double* tile_blk;    // the batch's uniform tiles, honoured read-only (null: none)
  const int* tile_uni;
  long size;                 // targets of the batch: a slot outside 0..size-1 is no candidate
  long n;                    // rows
  const int* slots;          // [n] slot of row i (-1: none), or null: dense, row i is slot i
  const int* batch;          // [n] or null: with it the launch serves only the rows whose entry is batch_index
  int batch_index;
  const double* delta;       // [n], by row
  double t1;                 // absolute query time; NaN = each target's own time
  TClock t_acc;
  const TClock* t_base;
  int have_origin;
  double origin[3];
  double sigma_r_max, sigma_t_max;
  double* cov;               // [n][6]
  double* sigma;             // [n][2] or null
  unsigned char* ok;         // [n] or null
};

// the launcher of a (model, precision, lanes per target, layout as LayoutInfo reports it, shared-axes form), or null
using CrossingCovLaunch = void (*)(const CrossingCovArgs&, hipStream_t);
CrossingCovLaunch crossing_cov_launcher(int type, int dtype, int g, int layout, bool shared_axes);
// the filler into the rows of a manager-level list that belong to no batch (entry outside 0..n_batches-1)
void launch_crossing_cov_orphans(const int* batch, long n, int n_batches, double* cov, double* sigma, unsigned char* ok, hipStream_t st);

}  // namespace te
