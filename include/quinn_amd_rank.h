/* quinn_amd -- the rank-diagnostics extension of the C ABI (include/quinn_amd.h holds the rest, the error codes and QN_F64 / QN_F32).
 * Same library, same conventions: every call returns QN_OK or a negative code, qn_last_error() says why. */
#ifndef QUINN_AMD_RANK_H
#define QUINN_AMD_RANK_H
#include "quinn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rank-normalised split-R-hat, folded split-R-hat, bulk- and tail-ESS, the ESS and the MCSE of the mean (Vehtari, Gelman,
 * Simpson, Carpenter & Buerkner 2021) of every entry of a stack of chains; quinn_amd/mcmc/rankdiag.py states the contract in
 * numpy float64, step by step, and the reference has no counterpart.
 * chain [C, T, K] contiguous, QN_F64 or QN_F32.  The window of a chain is its rows t0 + j * stride, j < 2 nh; j / nh is the
 * half: m = 2 C split sequences of nh draws, sequence 2 c + h, pooled size S = 2 C nh.  Per entry k, x the S window values:
 *   average ranks with ties r_i = (#{x_j < x_i} + #{x_j <= x_i} + 1) / 2,  z_i = Phi^-1((r_i - 3/8) / (S + 1/4));
 *   the folded series is |x_i - med|, med = (s[(S-1)/2] + s[S/2]) / 2 of the sorted values s, ranked and normalised alike;
 *   the tail indicators are 1[x_i <= q], q the pooled quantile at position q (S - 1) of s, linearly interpolated.
 * out [QN_RANK_NOUT, K] float64 holds per entry
 *   row 0  rhat_bulk  split-R-hat of z over the m sequences
 *   row 1  rhat_tail  split-R-hat of the rank-normalised folded series
 *   row 2  ess_bulk   autocorrelation ESS of z (Geyer's initial positive, then monotone, sequence of pair sums)
 *   row 3  ess_tail   the smaller of the ESS of the indicators at q = 0.05 and q = 0.95
 *   row 4  ess_mean   ESS of x
 *   row 5  mcse_mean  sqrt(pooled variance of x (ddof = 1) / ess_mean)
 * With stride > 1 these are the figures of the thinned draws.  All arithmetic is float64 whatever the input type, without
 * atomics, one writer per word, and every sum runs in an order fixed by (C, nh) alone: an entry's six numbers do not depend on
 * K, on the other entries of the call, on t0 or T beyond the rows selected, or on the launch geometry, and two calls give the
 * same bits.  Rows outside the window are never read.  A non-finite value in the window of an entry makes the six rows of
 * THAT entry NaN and changes no other entry; a series without within-sequence variance (W = 0) gives NaN for its figures.
 * QN_EINVAL with a message, before any pointer is touched: C < 1, nh < 4, stride < 1, t0 < 0, K < 1 (or K > 2^31),
 * 2 C nh > QN_RANK_MAX_S, t0 + (2 nh - 1) stride >= T, a bad dtype, a NULL chain, out or workspace; a workspace that is too
 * small is QN_EWORKSPACE.  qn_rank_diag_workspace_bytes returns 0 for arguments the call would refuse (qn_last_error() says
 * why) and needs no device.  The workspace (the windows of at most 1024 entries at a time, entry-major float64) needs no
 * initialisation and keeps no state. */
#define QN_RANK_MAX_S 16384
enum { QN_RANK_RHAT_BULK = 0, QN_RANK_RHAT_TAIL = 1, QN_RANK_ESS_BULK = 2,
       QN_RANK_ESS_TAIL = 3, QN_RANK_ESS_MEAN = 4, QN_RANK_MCSE_MEAN = 5, QN_RANK_NOUT = 6 };
size_t qn_rank_diag_workspace_bytes(int C, int64_t T, int64_t K, int64_t nh, int64_t stride);
int qn_rank_diag(const void* chain, int dtype, int C, int64_t T, int64_t K, int64_t t0, int64_t nh, int64_t stride,
                 double* out /* [QN_RANK_NOUT, K] float64 */, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QUINN_AMD_RANK_H */
