/* quinn_amd -- the Laplace-evidence extension of the C ABI (include/quinn_amd.h holds the rest and the error codes).  Same
 * library, same conventions: every call returns QN_OK or a negative code, qn_last_error() says why. */
#ifndef QUINN_AMD_EVIDENCE_H
#define QUINN_AMD_EVIDENCE_H
#include "quinn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The Laplace approximation of the log marginal likelihood of a member at its MAP weights (MacKay 1992; Immer et al. 2021;
 * quinn_amd/evidence.py states the contract in numpy; the reference has no counterpart).  Per member: c [p] >= 0 the curvature
 * spectrum in units of G (H = G / s2 + diag(tau)), w [p] the MAP weights, sse the sum of squared errors over its n entries of y,
 * and G groups of contiguous elements bounds[g] .. bounds[g + 1] - 1 (bounds: G + 1 values in HOST memory rising strictly from 0
 * to p; read before the call returns), n_g elements each.  With the noise variance s2 and the group precisions tau_g:
 *   lambda_j = c_j / s2 + tau_g(j)       logdet_g = sum_{j in g} log lambda_j       gamma_g = sum_{j in g} (c_j / s2) / lambda_j
 *   S_g = sum_{j in g} w_j^2             logdet = sum_g logdet_g                    gamma = sum_g gamma_g        (g ascending)
 *   loglik = -n/2 log(2 pi s2) - sse / (2 s2)
 *   logZ   = loglik + sum_g (n_g/2 log tau_g - tau_g S_g / 2) - logdet / 2
 * All arithmetic is float64, without atomics, fences or any exchange between workgroups, and every sum runs in an order fixed by
 * p, G and the bounds alone: a thread of the workgroup of 256 adds its elements bounds[g] + tid, + 256, ... of a group in index
 * order, a wave adds its lanes by a fixed butterfly, the workgroup adds its 4 waves in order.  Two calls give the same bits, and
 * nothing depends on B or Hc.  c_j / s2 is formed as c_j (1 / s2).  Argument errors are QN_EINVAL with a message before any
 * pointer is touched; a workspace that is too small is QN_EWORKSPACE.  Every _workspace_bytes query needs no device and returns 0
 * for arguments the call would refuse.  The workspace (the bounds on the device) needs no initialisation. */
#define QN_EV_MAX_G 32
#define QN_EV_NOUT 4          /* rows logZ, loglik, logdet, gamma; then gamma_g [G] and S_g [G] */
#define QN_EV_NSTATUS 6
#define QN_EV_MAX_ITER 100000
/* the bits of status[5] */
#define QN_EV_CLAMP_S2_MIN 1
#define QN_EV_CLAMP_S2_MAX 2
#define QN_EV_CLAMP_TAU_MIN 4
#define QN_EV_CLAMP_TAU_MAX 8

/* out [B, Hc, QN_EV_NOUT + 2 G]: the rows above for every member b and every candidate h of its grid, s2 [B, Hc] and
 * tau [B, Hc, G] on the device.  One workgroup per (member, candidate).  The host cannot see the device values: an s2 or tau_g
 * that is not finite and > 0, a c_j that is negative or not finite, a w_j or sse that is not finite makes all rows of THAT
 * candidate NaN and touches no other.
 * QN_EINVAL: B, p, Hc or n < 1, G < 1 or G > QN_EV_MAX_G or G > p, B Hc >= 2^31, p > 2^40, a NULL pointer, bounds that do not
 * rise strictly from 0 to p. */
size_t qn_la_evidence_workspace_bytes(int64_t B, int64_t p, int64_t G, int64_t Hc);
int qn_la_evidence(const double* c /* [B, p] */, const double* W /* [B, p] */, const double* sse /* [B] */, int64_t n, int64_t B,
                   int64_t p, const int64_t* bounds /* host, [G + 1] */, int64_t G, int64_t Hc, const double* s2 /* [B, Hc] */,
                   const double* tau /* [B, Hc, G] */, double* out /* [B, Hc, QN_EV_NOUT + 2 G] */, void* workspace,
                   size_t workspace_bytes, void* stream);

/* The maximisation of logZ over s2 (tune_noise) and the tau_g (tune_prior) at fixed w by MacKay's fixed point, one workgroup per
 * member and the whole iteration inside ONE launch.  From theta_0 = (s2_0 [B], tau_0 [B, G]), iterate t = 0, 1, ... evaluates the
 * rows at theta_t and
 *   resid = max( max_g |log(gamma_g / (tau_g S_g))|  (tune_prior only),  |log(sse / ((n - gamma) s2))|  (tune_noise only) ),
 * 0 if nothing is tuned; an argument of a log that is not finite and > 0 makes resid +Inf.  resid <= tol: stop, converged = 1,
 * theta_t is the answer.  t == max_iter: stop, converged = 0, the answer is the evaluated iterate with the largest finite logZ
 * (the first on a tie; iterate 0 if no logZ was finite), so logZ >= the logZ of the start.  Otherwise
 *   s2   <- sse / (n - gamma) clamped to [s2_min, s2_max]; s2_max if n - gamma <= 0                         (tune_noise only)
 *   tau_g <- gamma_g / S_g clamped to [tau_min, tau_max]; tau_min if gamma_g <= 0, else tau_max if S_g == 0   (tune_prior only)
 * and every clamp that acted in any update sets its QN_EV_CLAMP_ bit.  A component that is not tuned keeps its bits.
 * Outputs: s2 [B], tau [B, G], rows [B, QN_EV_NOUT + 2 G] of the returned iterate, status [B, QN_EV_NSTATUS]:
 *   [0] iters (the index of the last iterate evaluated)   [1] the index of the returned iterate   [2] converged (0 or 1)
 *   [3] resid of the returned iterate   [4] logZ of iterate 0   [5] the OR of the clamp bits
 * and, where not NULL, Dinv [B, p] = 1 / (cov_scale lambda_j) and Dih [B, p] = sqrt(Dinv) at the returned iterate (each within
 * 1 ulp), in c's order.  A member whose inputs are bad by the rules of qn_la_evidence gets NaN rows, Dinv and Dih, its start
 * back, iters = converged = 0 and resid = +Inf.
 * QN_EINVAL: the refusals of qn_la_evidence (Hc = 1), tol < 0 or not finite, max_iter < 0 or > QN_EV_MAX_ITER, clamps that are
 * not finite with 0 < min <= max, cov_scale not finite and > 0, tune_noise or tune_prior not 0 or 1. */
size_t qn_la_tune_workspace_bytes(int64_t B, int64_t p, int64_t G);
int qn_la_tune(const double* c /* [B, p] */, const double* W /* [B, p] */, const double* sse /* [B] */, int64_t n, int64_t B,
               int64_t p, const int64_t* bounds /* host, [G + 1] */, int64_t G, const double* s2_0 /* [B] */,
               const double* tau_0 /* [B, G] */, double tol, int64_t max_iter, double s2_min, double s2_max, double tau_min,
               double tau_max, int tune_noise, int tune_prior, double cov_scale, double* s2 /* [B] */, double* tau /* [B, G] */,
               double* rows /* [B, QN_EV_NOUT + 2 G] */, double* status /* [B, QN_EV_NSTATUS] */, double* Dinv /* [B, p] or NULL */,
               double* Dih /* [B, p] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QUINN_AMD_EVIDENCE_H */
