/* quinn_amd -- the stacking extension of the C ABI (include/quinn_amd.h holds the rest, the error codes, QN_F64 / QN_F32 and the
 * QN_SCORE_ bits).  Same library, same conventions: every call returns QN_OK or a negative code, qn_last_error() says why. */
#ifndef QUINN_AMD_STACK_H
#define QUINN_AMD_STACK_H
#include "quinn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Stacking of the chains of a fit that did not mix, or of the members of a deep ensemble (Yao, Vehtari, Simpson & Gelman 2018;
 * Yao, Vehtari & Gelman 2022; quinn_amd/stacking.py states the contract in numpy; the reference has no counterpart): every
 * group g gets a weight w_g on the simplex that maximises the log predictive density of the weighted mixture.
 * All arithmetic below is float64 whatever the input type, without atomics, and every sum runs in an order fixed by the
 * shape of the problem alone: two calls give the same bits and nothing depends on the launch geometry.  Argument errors are
 * QN_EINVAL with a message before any pointer is touched; a workspace that is too small is QN_EWORKSPACE.  Every
 * _workspace_bytes query needs no device and returns 0 for arguments the call would refuse (qn_last_error() says why).
 * The workspaces need no initialisation. */
#define QN_STACK_MAX_G 1024
#define QN_STACK_NSTATUS 8

/* L [G, K] float64: L_gk = logsumexp_{m in g} ll_mk - log M_g, the log density of entry k under group g alone, in one streaming
 * pass over F.  F, V, dtype, Y, sigma and ll_mk are those of qn_pred_score, bit for bit; group g holds the members
 * offsets[g] .. offsets[g + 1] - 1 (offsets: G + 1 values in HOST memory rising strictly from 0 to M; it is read before the call
 * returns).  M_g = 1 is legal.  A non-finite f or V, sigma^2 + V_mk <= 0 in a member of the group or a non-finite y makes
 * L_gk NaN and touches no other group or entry.  QN_EINVAL: M < 1, K < 1, G < 1 or G > M, a bad dtype, sigma < 0 or not finite,
 * sigma == 0 with V == NULL, a NULL F, Y, offsets, L or workspace, offsets that do not rise from 0 to M. */
size_t qn_group_lpd_workspace_bytes(int64_t M, int64_t K, int64_t G);
int qn_group_lpd(const void* F, const void* V, int dtype, const double* Y, int64_t M, int64_t K, double sigma,
                 const int64_t* offsets /* host, [G + 1] */, int64_t G, double* L /* [G, K] float64 */, void* workspace,
                 size_t workspace_bytes, void* stream);

/* The stacking weights of L [G, K] (-Inf: density 0) by EM for mixture weights.
 *   m_k = max_g L_gk over the elements that are neither NaN nor +Inf, E_gk = exp(L_gk - m_k); a NaN or +Inf element counts as
 *   E = 0 and in n_nonfinite; an entry whose m_k is -Inf (or that has no other element) is dropped from every sum and counted
 *   in n_dropped; K' entries are kept.  E lives in the workspace and is computed once.
 *   From w = 1 / G:  mix_k = sum_g w_g E_gk (g ascending),  grad_g = (1 / K') sum_k E_gk / mix_k,  obj = sum_k (log mix_k + m_k),
 *   gap = K' (max_g grad_g - 1) >= obj(w*) - obj(w) (obj is concave): the stopping certificate in nats.  Stop at the first
 *   iterate with gap <= tol or at iterate max_iter; else w_g <- w_g grad_g, renormalised by its sum (a fixed tree over g).
 *   The sums over k: block b of nb = min(ceil(K / 256), 256) owns the tiles b, b + nb, ... of 256 entries, a thread adds its
 *   entries in tile order, a wave its lanes by a fixed butterfly, the block its 4 waves in order; the partial sums of the nb
 *   blocks are added in block order by the NEXT launch, which every workgroup does for itself.  K' = 0: w = 1 / G, obj = gap = 0.
 * One call with t0 = 0 prepares E and enqueues launches 0 .. nlaunch - 1; a call with t0 > 0 continues with launches t0 ..
 * t0 + nlaunch - 1 on the same workspace, w and status.  Launch t evaluates iterate t after launch t - 1's sums have decided
 * that iterate t - 1 does not stop; once an iterate has stopped, `done` is set and every later launch is a no-op, so the host may
 * enqueue launches in blocks of any size and read the status late: w and iters do not depend on nlaunch.  max_iter + 2
 * launches always finish.  w [G] and status are written by the launch that stops and are undefined before `done` is 1:
 *   status[0] obj   [1] gap   [2] iters (the index of the iterate w, obj and gap belong to)   [3] K'   [4] n_nonfinite
 *   status[5] n_dropped   [6] obj at w = 1 / G   [7] done (0 or 1; valid after any launch)
 * QN_EINVAL: G < 1 or G > QN_STACK_MAX_G, K < 1 (or K > 2^31), tol < 0 or not finite, max_iter < 0, t0 < 0, nlaunch < 1, a NULL
 * pointer.  Workspace: [G + 3, K] float64 (E, m, the entries' non-finite counts, r) and 2 nb (G + 3) + 2 G more (the double-buffered
 * partial sums and iterates). */
size_t qn_stack_weights_workspace_bytes(int64_t G, int64_t K);
int qn_stack_weights(const double* L, int64_t G, int64_t K, double tol, int64_t max_iter, int64_t t0, int64_t nlaunch,
                     double* w /* [G] */, double* status /* [QN_STACK_NSTATUS] */, void* workspace, size_t workspace_bytes,
                     void* stream);

/* The scores of qn_pred_score, include/quinn_amd.h, for the mixture sum_m wm_m N(f_mk, sigma^2 + V_mk), wm [M] float64 on the device, wm_m >= 0,
 * sum wm = 1: the same `what` bits, row numbers and QN_SCORE_NOUT.  With s_m^2 = sigma^2 + V_mk and A as in qn_pred_score:
 *   row 0  lppd    logsumexp_m(ll_mk + log wm_m)
 *   row 1  p_waic  sum wm (ll - mean_w)^2 / (1 - sum wm^2)
 *   row 2  pit     sum wm Phi((y_k - f_mk) / s_m)
 *   row 3  crps    sum_i wm_i A(y - f_i, s_i^2) - 0.5 sum_i sum_j wm_i wm_j A(f_i - f_j, s_i^2 + s_j^2)   (j <= i evaluated)
 *   row 4  mean    sum wm f
 *   row 5  var     sum wm (f - mean)^2 / (1 - sum wm^2)
 * The 1 - sum wm^2 forms make every row that of qn_pred_score at wm = 1 / M.  A member with wm_m == 0 is skipped entirely: its
 * f and V may be anything.  1 - sum wm^2 == 0 (one member carries everything): rows 1 and 5 are 0.  The host cannot see wm: a
 * negative or non-finite weight makes every requested row NaN; the weights are not renormalised.  M >= 1; Y may be NULL when
 * what == QN_SCORE_MOMENTS.  Otherwise the refusals and the NaN rules of qn_pred_score. */
size_t qn_pred_score_w_workspace_bytes(int64_t M, int64_t K, int what);
int qn_pred_score_w(const void* F, const void* V, int dtype, const double* Y, const double* wm, int64_t M, int64_t K, double sigma,
                    int what, double* out /* [QN_SCORE_NOUT, K] float64 */, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QUINN_AMD_STACK_H */
