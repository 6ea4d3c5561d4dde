// Laplace evidence and its maximisation (include/quinn_amd_evidence.h; quinn_amd/evidence.py is the contract in numpy).
//
//   k_la_evidence    one workgroup of 256 per (member, candidate): one pass over the member's c and w, group by group, gives
//                    logdet_g, gamma_g and S_g; thread g finishes group g, every thread then adds the G numbers in order.
//   k_la_tune        one workgroup per member: the same pass per iterate of MacKay's fixed point (S_g only in the first), the
//                    stopping rule, the clamped update and the best-iterate fallback, all inside the launch; the loop is bounded
//                    by max_iter.  A last pass writes Dinv and Dih at the returned iterate.
//
// Every thread of a workgroup takes every decision from the same LDS values, so control flow is uniform.  No atomics, no fences,
// nothing shared between workgroups, one writer per output.  The wave butterfly is qn_stack.hip's, restated: lifting it into a
// header would change that file.
#include <cmath>

#include "qn_common.h"
#include "../../include/quinn_amd_evidence.h"

namespace {

constexpr int EB = 256;                  // threads per workgroup: the stride of a thread's elements
constexpr int EW = EB / 64;              // its waves
constexpr int GMAX = QN_EV_MAX_G;
constexpr double LOG_2PI = 1.8378770664093453;

struct EvShared {
    int64_t bnd[GMAX + 1];
    double tau[GMAX];
    double red[EW][3][GMAX];             // per wave: logdet_g, gamma_g, S_g
    double ld[GMAX], gm[GMAX], S[GMAX];  // the workgroup's sums
    double pri[GMAX];                    // n_g/2 log tau_g - tau_g S_g / 2
    double best_tau[GMAX], best_gm[GMAX];
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ bool pos_finite(double v) { return v > 0.0 && isfinite(v); }

// logdet_g, gamma_g (and with FIRST: S_g and the check of c and w) of every group at (1 / s2, sh.tau) into sh.ld, sh.gm, sh.S,
// then sh.pri.  Ends with a barrier.
template <bool FIRST>
__device__ __forceinline__ void ev_pass(const double* __restrict__ c, const double* __restrict__ w, int G, double inv_s2,
                                        EvShared& sh, bool& bad) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int g = 0; g < G; ++g) {
        const int64_t hi = sh.bnd[g + 1];
        const double tau = sh.tau[g];
        double ld = 0.0, gm = 0.0, ss = 0.0;
#pragma unroll 4
        for (int64_t j = sh.bnd[g] + tid; j < hi; j += EB) {
            const double cj = c[j];
            if (FIRST) {
                const double wj = w[j];
                bad = bad || !(cj >= 0.0) || !isfinite(cj) || !isfinite(wj);
                ss += wj * wj;
            }
            const double a = cj * inv_s2, lam = a + tau;
            ld += log(lam);
            gm += a / lam;
        }
        ld = wave_sum(ld);
        gm = wave_sum(gm);
        if (FIRST) ss = wave_sum(ss);
        if (lane == 0) {
            sh.red[wv][0][g] = ld;
            sh.red[wv][1][g] = gm;
            if (FIRST) sh.red[wv][2][g] = ss;
        }
    }
    __syncthreads();
    if (tid < G) {
        double ld = sh.red[0][0][tid], gm = sh.red[0][1][tid], ss = FIRST ? sh.red[0][2][tid] : sh.S[tid];
#pragma unroll
        for (int q = 1; q < EW; ++q) {
            ld += sh.red[q][0][tid];
            gm += sh.red[q][1][tid];
            if (FIRST) ss += sh.red[q][2][tid];
        }
        sh.ld[tid] = ld;
        sh.gm[tid] = gm;
        if (FIRST) sh.S[tid] = ss;
        const double tau = sh.tau[tid];
        sh.pri[tid] = 0.5 * (double)(sh.bnd[tid + 1] - sh.bnd[tid]) * log(tau) - 0.5 * tau * ss;
    }
    __syncthreads();
}

struct EvRows {
    double logZ, loglik, logdet, gamma;
};

// the four scalar rows from the group sums (every thread, the same bits)
__device__ __forceinline__ EvRows ev_rows(const EvShared& sh, int G, double n, double sse, double s2, double inv_s2) {
    EvRows r;
    double ld = 0.0, gm = 0.0, pri = 0.0;
    for (int g = 0; g < G; ++g) {
        ld += sh.ld[g];
        gm += sh.gm[g];
        pri += sh.pri[g];
    }
    r.logdet = ld;
    r.gamma = gm;
    r.loglik = -0.5 * n * (LOG_2PI + log(s2)) - 0.5 * sse * inv_s2;
    r.logZ = r.loglik + pri - 0.5 * ld;
    return r;
}

__device__ __forceinline__ void ev_load(EvShared& sh, const int64_t* __restrict__ bnd, const double* __restrict__ tau, int G,
                                        bool& bad) {
    const int tid = threadIdx.x;
    if (tid <= G) sh.bnd[tid] = bnd[tid];
    if (tid < G) {
        const double t = tau[tid];
        sh.tau[tid] = t;
        bad = bad || !pos_finite(t);
    }
    __syncthreads();
}

__global__ __launch_bounds__(EB) void k_la_evidence(const double* __restrict__ c, const double* __restrict__ W,
                                                    const double* __restrict__ sse, double n, int64_t p,
                                                    const int64_t* __restrict__ bnd, int G, int64_t Hc,
                                                    const double* __restrict__ s2, const double* __restrict__ tau,
                                                    double* __restrict__ out) {
    __shared__ EvShared sh;
    const int tid = threadIdx.x;
    const int64_t blk = blockIdx.x, b = blk / Hc;
    const double s2v = s2[blk], ssev = sse[b];
    bool bad = !pos_finite(s2v) || !isfinite(ssev);
    ev_load(sh, bnd, tau + blk * G, G, bad);
    const double inv_s2 = 1.0 / s2v;
    ev_pass<true>(c + b * p, W + b * p, G, inv_s2, sh, bad);
    const bool anybad = __syncthreads_or(bad);
    const EvRows r = ev_rows(sh, G, n, ssev, s2v, inv_s2);
    const double nan = __builtin_nan("");
    double* o = out + blk * (QN_EV_NOUT + 2 * G);
    if (tid == 0) {
        o[0] = anybad ? nan : r.logZ;
        o[1] = anybad ? nan : r.loglik;
        o[2] = anybad ? nan : r.logdet;
        o[3] = anybad ? nan : r.gamma;
    }
    if (tid < G) {
        o[QN_EV_NOUT + tid] = anybad ? nan : sh.gm[tid];
        o[QN_EV_NOUT + G + tid] = anybad ? nan : sh.S[tid];
    }
}

// |log(num / den)| of the stopping rule; +Inf when the argument is not finite and > 0
__device__ __forceinline__ double ev_abslog(double num, double den) {
    const double a = num / den;
    return pos_finite(a) ? fabs(log(a)) : __builtin_inf();
}

// 1 / (cs (c / s2 + tau)) with the roundings of the quotient, the sum and the product carried along: within 1 ulp
__device__ __forceinline__ double ev_dinv(double c, double s2, double tau, double cs) {
    const double q = c / s2, lam = q + tau, x = cs * lam, d = 1.0 / x;
    if (!isfinite(x) || !isfinite(d)) return d;
    const double ql = fma(-q, s2, c) / s2;
    const double bb = lam - q, le = (q - (lam - bb)) + (tau - bb);
    const double xl = fma(cs, lam, -x) + cs * (le + ql);
    return fma(d, fma(-xl, d, fma(-d, x, 1.0)), d);
}

struct TuneArgs {
    double n, tol, s2_min, s2_max, tau_min, tau_max, cov_scale;
    int64_t p, max_iter;
    int G, tune_noise, tune_prior;
};

__global__ __launch_bounds__(EB) void k_la_tune(const double* __restrict__ c, const double* __restrict__ W,
                                                const double* __restrict__ sse, const int64_t* __restrict__ bnd,
                                                const double* __restrict__ s2_0, const double* __restrict__ tau_0, TuneArgs a,
                                                double* __restrict__ s2_out, double* __restrict__ tau_out,
                                                double* __restrict__ rows, double* __restrict__ status,
                                                double* __restrict__ Dinv, double* __restrict__ Dih) {
    __shared__ EvShared sh;
    const int tid = threadIdx.x, G = a.G;
    const int64_t b = blockIdx.x;
    const double* cb = c + b * a.p;
    const double ssev = sse[b], nan = __builtin_nan(""), inf = __builtin_inf();
    double s2v = s2_0[b];
    bool bad = !pos_finite(s2v) || !isfinite(ssev);
    ev_load(sh, bnd, tau_0 + b * G, G, bad);
    ev_pass<true>(cb, W + b * a.p, G, 1.0 / s2v, sh, bad);
    double* ro = rows + b * (QN_EV_NOUT + 2 * G);
    double* so = status + b * QN_EV_NSTATUS;
    if (__syncthreads_or(bad)) {
        if (tid == 0) {
            s2_out[b] = s2v;
            ro[0] = ro[1] = ro[2] = ro[3] = nan;
            so[0] = so[1] = so[2] = so[5] = 0.0;
            so[3] = inf;
            so[4] = nan;
        }
        if (tid < G) {
            tau_out[b * G + tid] = tau_0[b * G + tid];
            ro[QN_EV_NOUT + tid] = ro[QN_EV_NOUT + G + tid] = nan;
        }
        for (int64_t j = tid; j < a.p; j += EB) {
            if (Dinv) Dinv[b * a.p + j] = nan;
            if (Dih) Dih[b * a.p + j] = nan;
        }
        return;
    }
    EvRows r, best;
    double resid = 0.0, best_resid = 0.0, best_s2 = s2v, logZ0 = 0.0;
    int64_t t = 0, best_t = 0;
    int flags = 0;
    bool conv = false;
    for (;; ++t) {                                               // at most max_iter + 1 rounds
        const double inv_s2 = 1.0 / s2v;
        if (t > 0) ev_pass<false>(cb, nullptr, G, inv_s2, sh, bad);
        r = ev_rows(sh, G, a.n, ssev, s2v, inv_s2);
        resid = 0.0;
        if (a.tune_prior)
            for (int g = 0; g < G; ++g) resid = fmax(resid, ev_abslog(sh.gm[g], sh.tau[g] * sh.S[g]));
        if (a.tune_noise) resid = fmax(resid, ev_abslog(ssev, (a.n - r.gamma) * s2v));
        if (t == 0) logZ0 = r.logZ;
        if (t == 0 || (isfinite(r.logZ) && !(best.logZ >= r.logZ))) {
            best = r;
            best_resid = resid;
            best_s2 = s2v;
            best_t = t;
            if (tid < G) {
                sh.best_tau[tid] = sh.tau[tid];
                sh.best_gm[tid] = sh.gm[tid];
            }
        }
        conv = resid <= a.tol;
        if (conv || t >= a.max_iter) break;
        if (a.tune_noise) {
            const double den = a.n - r.gamma;
            double v = den > 0.0 ? ssev / den : a.s2_max;
            if (!(den > 0.0) || v > a.s2_max) {
                v = a.s2_max;
                flags |= QN_EV_CLAMP_S2_MAX;
            } else if (v < a.s2_min) {
                v = a.s2_min;
                flags |= QN_EV_CLAMP_S2_MIN;
            }
            s2v = v;
        }
        __syncthreads();                                         // every thread has read this iterate's tau
        if (a.tune_prior)
            for (int g = 0; g < G; ++g) {
                const double gg = sh.gm[g], sg = sh.S[g];
                double v;
                if (!(gg > 0.0)) {
                    v = a.tau_min;
                    flags |= QN_EV_CLAMP_TAU_MIN;
                } else if (sg == 0.0 || gg / sg > a.tau_max) {
                    v = a.tau_max;
                    flags |= QN_EV_CLAMP_TAU_MAX;
                } else if (gg / sg < a.tau_min) {
                    v = a.tau_min;
                    flags |= QN_EV_CLAMP_TAU_MIN;
                } else {
                    v = gg / sg;
                }
                if (tid == g) sh.tau[g] = v;
            }
        __syncthreads();
    }
    __syncthreads();
    if (!conv && best_t != t) {                                  // the fallback: the best iterate seen
        r = best;
        resid = best_resid;
        s2v = best_s2;
        if (tid < G) {
            sh.tau[tid] = sh.best_tau[tid];
            sh.gm[tid] = sh.best_gm[tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        s2_out[b] = s2v;
        ro[0] = r.logZ;
        ro[1] = r.loglik;
        ro[2] = r.logdet;
        ro[3] = r.gamma;
        so[0] = (double)t;
        so[1] = (double)(conv ? t : best_t);
        so[2] = conv ? 1.0 : 0.0;
        so[3] = resid;
        so[4] = logZ0;
        so[5] = (double)flags;
    }
    if (tid < G) {
        tau_out[b * G + tid] = sh.tau[tid];
        ro[QN_EV_NOUT + tid] = sh.gm[tid];
        ro[QN_EV_NOUT + G + tid] = sh.S[tid];
    }
    if (!Dinv && !Dih) return;
    for (int g = 0; g < G; ++g) {
        const int64_t hi = sh.bnd[g + 1];
        const double tau = sh.tau[g];
        for (int64_t j = sh.bnd[g] + tid; j < hi; j += EB) {
            const double d = ev_dinv(cb[j], s2v, tau, a.cov_scale);
            if (Dinv) Dinv[b * a.p + j] = d;
            if (Dih) Dih[b * a.p + j] = sqrt(d);
        }
    }
}

size_t ev_workspace(const char* who, int64_t B, int64_t p, int64_t G, int64_t Hc, int64_t n) {
    if (B < 1 || p < 1 || Hc < 1 || n < 1) {
        qn_set_error("%s: need B >= 1 members, p >= 1 elements, Hc >= 1 candidates and n >= 1 entries (B=%lld p=%lld Hc=%lld n=%lld)",
                     who, (long long)B, (long long)p, (long long)Hc, (long long)n);
        return 0;
    }
    if (G < 1 || G > GMAX || G > p) {
        qn_set_error("%s: need 1 <= G <= min(%d, p) groups (G=%lld p=%lld)", who, GMAX, (long long)G, (long long)p);
        return 0;
    }
    if (p > (int64_t(1) << 40) || Hc >= (int64_t(1) << 31) || B >= (int64_t(1) << 31) / Hc) {
        qn_set_error("%s: shape too large (B=%lld p=%lld Hc=%lld)", who, (long long)B, (long long)p, (long long)Hc);
        return 0;
    }
    return qn_align((size_t)(G + 1) * sizeof(int64_t));
}

// the checks both entry points share, after the shape: pointers, workspace, bounds.  QN_OK or the code to return.
int ev_check(const char* who, bool ptrs_ok, const char* ptr_names, const int64_t* bounds, int64_t G, int64_t p, size_t need,
             size_t workspace_bytes) {
    if (!ptrs_ok) {
        qn_set_error("%s: %s must not be NULL", who, ptr_names);
        return QN_EINVAL;
    }
    if (workspace_bytes < need) {
        qn_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
        return QN_EWORKSPACE;
    }
    bool rising = bounds[0] == 0 && bounds[G] == p;
    for (int64_t g = 0; g < G && rising; ++g) rising = bounds[g + 1] > bounds[g];
    if (!rising) {
        qn_set_error("%s: bounds must rise strictly from 0 to p = %lld", who, (long long)p);
        return QN_EINVAL;
    }
    return QN_OK;
}

}  // namespace

extern "C" size_t qn_la_evidence_workspace_bytes(int64_t B, int64_t p, int64_t G, int64_t Hc) {
    return ev_workspace("qn_la_evidence_workspace_bytes", B, p, G, Hc, 1);
}

extern "C" int qn_la_evidence(const double* c, const double* W, const double* sse, int64_t n, int64_t B, int64_t p,
                              const int64_t* bounds, int64_t G, int64_t Hc, const double* s2, const double* tau, double* out,
                              void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = ev_workspace("qn_la_evidence", B, p, G, Hc, n);
    if (need == 0) return QN_EINVAL;
    const int rc = ev_check("qn_la_evidence", c && W && sse && bounds && s2 && tau && out && workspace,
                            "c, W, sse, bounds, s2, tau, out and workspace", bounds, G, p, need, workspace_bytes);
    if (rc != QN_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    int64_t* bnd = static_cast<int64_t*>(workspace);
    QN_HIP_CHECK(hipMemcpyAsync(bnd, bounds, (size_t)(G + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_la_evidence, dim3((unsigned)(B * Hc)), dim3(EB), 0, st, c, W, sse, (double)n, p, bnd, (int)G, Hc, s2, tau,
                       out);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}

extern "C" size_t qn_la_tune_workspace_bytes(int64_t B, int64_t p, int64_t G) {
    return ev_workspace("qn_la_tune_workspace_bytes", B, p, G, 1, 1);
}

extern "C" int qn_la_tune(const double* c, const double* W, const double* sse, int64_t n, int64_t B, int64_t p,
                          const int64_t* bounds, int64_t G, const double* s2_0, const double* tau_0, double tol, int64_t max_iter,
                          double s2_min, double s2_max, double tau_min, double tau_max, int tune_noise, int tune_prior,
                          double cov_scale, double* s2, double* tau, double* rows, double* status, double* Dinv, double* Dih,
                          void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = ev_workspace("qn_la_tune", B, p, G, 1, n);
    if (need == 0) return QN_EINVAL;
    if (!(tol >= 0.0) || !std::isfinite(tol) || max_iter < 0 || max_iter > QN_EV_MAX_ITER) {
        qn_set_error("qn_la_tune: need tol >= 0 and finite and 0 <= max_iter <= %d (tol=%g max_iter=%lld)", QN_EV_MAX_ITER, tol,
                     (long long)max_iter);
        return QN_EINVAL;
    }
    if (!(s2_min > 0.0) || !(s2_max >= s2_min) || !std::isfinite(s2_max) || !(tau_min > 0.0) || !(tau_max >= tau_min) ||
        !std::isfinite(tau_max)) {
        qn_set_error("qn_la_tune: the clamps must be finite with 0 < min <= max (s2: %g, %g; tau: %g, %g)", s2_min, s2_max, tau_min,
                     tau_max);
        return QN_EINVAL;
    }
    if (!(cov_scale > 0.0) || !std::isfinite(cov_scale) || (tune_noise != 0 && tune_noise != 1) ||
        (tune_prior != 0 && tune_prior != 1)) {
        qn_set_error("qn_la_tune: need cov_scale > 0 and finite, tune_noise and tune_prior 0 or 1 (cov_scale=%g tune_noise=%d "
                     "tune_prior=%d)", cov_scale, tune_noise, tune_prior);
        return QN_EINVAL;
    }
    const int rc = ev_check("qn_la_tune", c && W && sse && bounds && s2_0 && tau_0 && s2 && tau && rows && status && workspace,
                            "c, W, sse, bounds, s2_0, tau_0, s2, tau, rows, status and workspace", bounds, G, p, need,
                            workspace_bytes);
    if (rc != QN_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    int64_t* bnd = static_cast<int64_t*>(workspace);
    QN_HIP_CHECK(hipMemcpyAsync(bnd, bounds, (size_t)(G + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    TuneArgs a;
    a.n = (double)n;
    a.tol = tol;
    a.s2_min = s2_min;
    a.s2_max = s2_max;
    a.tau_min = tau_min;
    a.tau_max = tau_max;
    a.cov_scale = cov_scale;
    a.p = p;
    a.max_iter = max_iter;
    a.G = (int)G;
    a.tune_noise = tune_noise;
    a.tune_prior = tune_prior;
    hipLaunchKernelGGL(k_la_tune, dim3((unsigned)B), dim3(EB), 0, st, c, W, sse, bnd, s2_0, tau_0, a, s2, tau, rows, status, Dinv,
                       Dih);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
