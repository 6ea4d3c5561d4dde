/* quinn_amd -- the NUTS warm-up extension of the C ABI (include/quinn_amd.h holds the rest, the error codes and the contract of
 * the No-U-Turn entry points whose state this call reads and amends).
 * Same library, same conventions: every call returns QN_OK or a negative code, qn_last_error() says why. */
#ifndef QUINN_AMD_NUTS_ADAPT_H
#define QUINN_AMD_NUTS_ADAPT_H
#include "quinn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The windowed warm-up of the No-U-Turn sampler: per-chain step size by dual averaging and per-chain diagonal mass by Welford
 * moments over Stan's slow windows, for chains that each run on their own step counter (quinn_amd/mcmc/nuts_adapt.py states the
 * contract and restates it in numpy; quinn_amd/mcmc/adapt.py has the schedule).  One launch BEHIND each call of the iteration
 * entry point of include/quinn_amd.h, with the `parity` that call was given and with that call's adapt = 0 (its own dual
 * averaging counts m = t + 1 and cannot restart at a window end).
 *
 * es [2, C, 12], ei [2, C, 8], cur, ql, ul, gl, q, u [C, p], alphas [C, nmcmc + 1]: the arrays of the iteration call.
 * plan: int32 [adapt, 4] on the device, row k - 1 for warm-up step k = 1 .. adapt: m (the index of the step in the current
 *   dual-averaging run, >= 1), n (the states collected in the current window, this one included), flags (QN_NUTS_PLAN_*), 0.
 * ws [2, C, 4] float64: (mu, hbar, logbar, eps) of dual averaging, double-buffered like es: slot `parity` is read, slot
 *   1 - parity written.  Slot 0 starts as (log(10 eps0), 0, 0, eps0).
 * mean, m2, scale [C, p]: the window's moments (0 at the start) and the scale the leapfrogs read (1, or a given one).
 *
 * A chain ENDED A STEP in the iteration iff t of slot 1 - parity of ei (written) is t + 1 of slot parity (read); k is the new
 * value.  For such a chain with 1 <= k <= adapt and the row (m, n, flags) of step k:
 *   a = alphas[c, k], NaN counted as 0, capped at 1
 *   hbar = (1 - 1 / (m + 10)) hbar + (target_accept - a) / (m + 10);  logeps = mu - (sqrt(m) / 0.05) hbar
 *   logbar = m^-0.75 logeps + (1 - m^-0.75) logbar;  eps = exp(logeps), or exp(logbar) with QN_NUTS_PLAN_FREEZE
 *   QN_NUTS_PLAN_COLLECT:  d = cur - mean;  mean += d / n;  m2 += d (cur - mean)
 *   QN_NUTS_PLAN_FINISH:   scale = sqrt((n / (n + 5)) m2 / (n - 1) + 0.005 / (n + 5));  mean = m2 = 0;  mu = log(10 eps);
 *                          hbar = logbar = 0
 *   k < nmcmc (the next step has started; its first half kick and drift used the old eps and scale):
 *                          u = ul + (hk scale) gl;  q = ql + (dr scale) u     hk = v ((eps / 2) gs), dr = v eps, gs = -0.5 /
 *                          sigma^2, v of slot 1 - parity; ul, rho, the parts of |z|^2 and H0 stay (the momenta are whitened)
 *   ws[1 - parity] = (mu, hbar, logbar, eps) and eps of es[1 - parity] = eps.
 * Every other chain -- no step ended, k > adapt, done, or a plan row with m < 1, a collecting n < 1 or a finishing n < 2 -- keeps
 * every bit of es, ei and the vectors in both slots; its ws[parity] is copied to ws[1 - parity].
 *
 * Geometry of the No-U-Turn kernels (the same workgroups per chain, the same pair of elements per thread: mean, m2, scale, q, u
 * are updated in place by the thread that owns the element).  Every workgroup of a chain reads both slots of ei, the chain's
 * alphas entry and ws[parity] and computes the same eps; workgroup 0 alone writes ws[1 - parity] and es.eps, which no workgroup
 * reads here.  No atomics, no fences, nothing is read back; every elementwise operation is rounded once (no contraction), so
 * mean, m2, scale, q and u are those of the numpy restatement bit for bit given the same eps.  Equal inputs give equal bits; a
 * chain does not depend on C, on its place in the launch or on the other chains.  HBM traffic per element of a chain that
 * ended a warm-up step: 6 x 8 B for the redo (scale, ql, ul, gl read; q, u written), 5 more when collecting, 1 more at a window
 * end; any other chain moves nothing but its scalars.
 * QN_EINVAL with a message, before any pointer is touched: C < 1 or C > 65535, p < 1, nmcmc < 1, sigma not > 0 and finite,
 * adapt outside 1 .. nmcmc, target_accept outside (0, 1), parity other than 0 / 1, a NULL pointer (only stream may be NULL). */
#define QN_NUTS_PLAN_COLLECT 1
#define QN_NUTS_PLAN_FINISH  2
#define QN_NUTS_PLAN_FREEZE  4
int qn_nuts_adapt(const double* cur, const double* alphas, int nmcmc, int adapt, double target_accept,
                  const int32_t* plan /* device int32 [adapt, 4]: m, n, flags, 0 */, double* es, const int64_t* ei, int parity,
                  int C, int64_t p, double sigma, const double* ql, const double* ul, const double* gl, double* q, double* u,
                  double* ws /* [2, C, 4] */, double* mean, double* m2, double* scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QUINN_AMD_NUTS_ADAPT_H */
