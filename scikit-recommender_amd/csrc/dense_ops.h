// dense_ops.h -- the two dense products over rows that mgcn.hip owns (its kernels mg_xty_kernel, mg_colsum_kernel,
// mg_reduce_kernel and mg_rows_w_kernel), for the other models' steps: host functions of the library, not exported.
// Operands are fp32, the sums run on v_mfma_f64_16x16x4_f64 and are rounded once; no floating-point atomic, fixed order.
#pragma once
#include "skr_common.h"

namespace skr {

// floats of `part` for one dense_xty over n rows with ld columns
int64_t dense_xty_floats(int64_t n, int ld);
// out = Dm^T Y [64][ld] | the column sums of Dm [64], over the n rows of Dm [n][64] and Y [n][ld]: per-row-block partial sums
// in `part`, added in block order.  Y == NULL: the column sums alone, out [64]
int dense_xty(const float* Dm, const float* Y, int64_t n, int ld, float* part, float* out, hipStream_t st);
// out[b][f] (+)= sum_o Dm[b][o] W[o][f] for Dm [n][64], W [64][ld], out [n][ld]
int dense_rows_w(const float* Dm, int64_t n, int ld, const float* W, float* out, int accumulate, hipStream_t st);

}  // namespace skr
