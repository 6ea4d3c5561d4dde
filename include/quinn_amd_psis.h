/* quinn_amd -- the PSIS-LOO extension of the C ABI (include/quinn_amd.h holds the rest, the error codes and QN_F64 / QN_F32).
 * Same library, same conventions: every call returns QN_OK or a negative code, qn_last_error() says why. */
#ifndef QUINN_AMD_PSIS_H
#define QUINN_AMD_PSIS_H
#include "quinn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pareto-smoothed importance-sampling leave-one-out scores of the ensemble that qn_pred_score scores (Vehtari, Gelman & Gabry 2017; Vehtari et al.
 * 2024; quinn_amd/psis.py states the contract in numpy and forms the summaries; the reference has no counterpart).  F, V,
 * dtype, Y and sigma are those of that call (include/quinn_amd.h), ll_mk its log density, bit for bit.  Per entry k:
 *   lr_m = -ll_mk - max_m(-ll_mk), the log importance ratios of leaving y_k out;  T = ceil(min(M / 5, 3 sqrt(M))).
 *   The tail is the T largest members in the total order (lr_m, m) -- ties never change its size -- and the cutoff c the
 *   (T+1)-th largest lr.  x_j = exp(lr_(j)) - exp(c), j = 1 .. T ascending, n = T, q = floor(T / 4 + 0.5).
 *   Generalised Pareto fit (Zhang & Stephens 2009): m = 30 + floor(sqrt(n)); b_i = 1 / x_n + (1 - sqrt(m / (i - 0.5))) / (3 x_q),
 *   k_i = mean_j log1p(-b_i x_j), L_i = n (log(-b_i / k_i) - k_i - 1), w_i = 1 / sum_l exp(L_l - L_i) for i = 1 .. m (no
 *   weight is dropped); b = sum_i w_i b_i, k' = mean_j log1p(-b x_j), sigma_gpd = -k' / b, khat = (n k' + 5) / (n + 10).
 *   The j-th smallest tail member gets lw = log(exp(c) + sigma_gpd expm1(-khat log1p(-p_j)) / khat), p_j = (j - 0.5) / T
 *   (khat == 0: the quantile is -sigma_gpd log1p(-p_j)); the other members keep lw_m = lr_m; every lw is cut at 0.
 *   With T < 5 (M < 21), x_q <= 0 (a tied or underflowed tail) or a non-finite khat or sigma_gpd, the tail keeps lw_m = lr_m
 *   too (truncated importance sampling) and khat is +Inf.
 * out [QN_LOO_NOUT, K] float64 holds per entry, with w = softmax_m(lw_m):
 *   row 0  elpd_loo  logsumexp_m(ll_mk + lw_m) - logsumexp_m(lw_m)
 *   row 1  khat      the shape of the fitted tail: the estimate is reliable below min(1 - 1 / log10(M), 0.7)
 *   row 2  ess       1 / sum_m w_m^2
 *   row 3  pit_loo   sum_m w_m Phi((y_k - f_mk) / s_mk)
 * All arithmetic is float64 whatever the input type, without atomics, and every sum runs in an order fixed by M alone (a tail
 * member is summed at its rank): an entry's four numbers do not depend on K, on the other entries of the call or on the launch
 * geometry, and two calls give the same bits.  A non-finite f, V or y, sigma^2 + V_mk < 0 or s_mk = 0 makes the four rows of
 * THAT entry NaN and changes no other entry.
 * QN_EINVAL with a message, before any pointer is touched: M < 2 or M > QN_PSIS_MAX_M, K < 1 (or K > 2^31), a bad dtype,
 * sigma < 0 or not finite, sigma == 0 with V == NULL, a NULL F, Y, out or workspace; a workspace that is too small is
 * QN_EWORKSPACE.  qn_psis_loo_workspace_bytes returns 0 for (M, K) the call would refuse (qn_last_error() says why) and needs
 * no device.  The workspace ([10, K] float64: the ratio maximum, the cutoff and the tail's partial sums of each entry) needs no
 * initialisation and keeps no state. */
#define QN_LOO_NOUT 4
#define QN_PSIS_MAX_M 16384
size_t qn_psis_loo_workspace_bytes(int64_t M, int64_t K);
int qn_psis_loo(const void* F, const void* V, int dtype, const double* Y, int64_t M, int64_t K, double sigma,
                double* out /* [QN_LOO_NOUT, K] float64 */, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QUINN_AMD_PSIS_H */
