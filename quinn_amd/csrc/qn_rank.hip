// Rank-normalised convergence diagnostics of a stack of chains: chain [C, T, K] -> out [QN_RANK_NOUT, K] (rhat_bulk, rhat_tail,
// ess_bulk, ess_tail, ess_mean, mcse_mean per entry; the definitions are in include/quinn_amd_rank.h at qn_rank_diag, written out
// step by step in numpy by quinn_amd/mcmc/rankdiag.py).  The entries are walked in chunks of RK_CHUNK, two launches per chunk:
//
//   k_rank_gather  reads the window rows of the chunk coalesced across entries (the chain's layout) and writes them entry-major
//                  into the workspace, ws[e][p], p = (2 c + h) nh + i the pooled index, through a 32 x 32 LDS tile; float64.
//   k_rank_entry   one workgroup of RK_T threads per entry.  Thread t owns the draws p = t, t + RK_T, ... and reads them from the
//                  workspace whenever a series is formed; LDS holds ONE series of S doubles at a time (padded to a power of
//                  two while it is sorted) and RK_SCR doubles of scratch.  Sort (bitonic network, +Inf sentinels), then every draw finds
//                  lo = #less and hi = #less-or-equal by binary search, so tied draws get their average rank exactly; the
//                  median and the two quantiles are read off the sorted values.  z overwrites the buffer in chain order;
//                  `series` turns the buffer into W, B and, when asked, the ESS.  The same for |x - med|, the two
//                  indicators and x itself.
//
// `series`: d = v - v[0] (the figures are shift-invariant; a common offset of 1e8 would otherwise cost the sums 8 digits), the
// sequence means (chunks of 64 draws summed in order, then the chunk sums in order), the draws centred in place, then the lagged
// products RK_L lags at a time: thread (lag, slot) sums units (sequence, chunk of 64 draws) slot, slot + 64, ... each in draw
// order, slots are joined by a butterfly and across waves in wave order.  Geyer's rule is evaluated by every thread alike on the
// block's lags, and the next block is computed only if the rule has not stopped: the figures do not depend on that.
//
// No atomics, one writer per word, every order a function of (C, nh) alone.
#include <cmath>

#include "qn_common.h"
#include "../../include/quinn_amd_rank.h"

namespace {

constexpr int RK_T = 1024;                        // threads of k_rank_entry
constexpr int RK_CH = 64;                         // draws per unit of a sequence sum
constexpr int RK_L = 16;                          // lags per block (a power of two <= 64, even: whole pairs)
constexpr int RK_SLOTS = RK_T / RK_L;
constexpr int RK_WAVES = RK_T / 64;
constexpr int RK_CHUNK = 512;                     // entries per pair of launches
// scratch (doubles): chunk sums of the sequences with more than one chunk, their means, the per-wave partials
constexpr int SC_PART = 0, SC_PART_N = QN_RANK_MAX_S / RK_CH + QN_RANK_MAX_S / (RK_CH + 1);      // m * ceil(nh / 64) when nh > 64
constexpr int SC_MEAN = SC_PART + SC_PART_N, SC_MEAN_N = QN_RANK_MAX_S / (RK_CH + 1) + 1;        // m when nh > 64
constexpr int SC_RED = SC_MEAN + SC_MEAN_N, SC_RED_N = RK_WAVES * RK_L + RK_L;
constexpr int RK_SCR = (SC_RED + SC_RED_N + 1) / 2 * 2;
constexpr int RK_MSEQ = QN_RANK_MAX_S / 4 / RK_T; // sequences whose mean a thread keeps: m <= MAX_S / 4 (nh >= 4)

static_assert(RK_MSEQ * RK_T * 4 == QN_RANK_MAX_S, "sequences per thread");
static_assert((size_t)(QN_RANK_MAX_S + RK_SCR) * sizeof(double) <= 160 * 1024 - 1024, "series + scratch fit the CU's LDS");
static_assert(RK_L % 2 == 0 && 64 % RK_L == 0, "a block of lags is whole pairs and divides a wave");

template <typename T>
__global__ __launch_bounds__(256) void k_rank_gather(const T* __restrict__ chain, int64_t Tn, int64_t K, int64_t t0, int64_t nh,
                                                     int64_t stride, int S, int64_t k0, int kc, double* __restrict__ ws) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int e = blockIdx.x * 32 + tx;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = blockIdx.y * 32 + ty + 8 * r;
        if (e < kc && p < S) {
            const int64_t c = p / (2 * nh), j = p % (2 * nh);
            tile[ty + 8 * r][tx] = (double)chain[(c * Tn + t0 + j * stride) * K + k0 + e];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e2 = blockIdx.x * 32 + ty + 8 * r, p2 = blockIdx.y * 32 + tx;
        if (e2 < kc && p2 < S) ws[(int64_t)e2 * S + p2] = tile[tx][ty + 8 * r];
    }
}

// Phi^-1 by Wichura's AS241 (PPND16, Appl. Statist. 37, 1988), the algorithm of Python's statistics.NormalDist.inv_cdf.  Its
// third branch (sqrt(-log p) > 5) cannot be reached: p >= 0.625 / (QN_RANK_MAX_S + 0.25) gives sqrt(-log p) < 3.2.
__device__ double inv_normal_cdf(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                              1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                                2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                              4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    double r = sqrt(-log(q <= 0.0 ? p : 1.0 - p)) - 1.6;
    const double num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                            1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                          4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    const double den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                            1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                          2.05319162663775882187e+0) * r + 1.0);
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

// the pooled quantile at position q (S - 1) of the sorted values; no contraction: q decides the indicator series, and the
// contract forms it with a product and a sum
__device__ double sorted_quantile(const double* s, int S, double q) {
#pragma clang fp contract(off)
    const double pos = q * (double)(S - 1);
    const int i0 = (int)pos, i1 = i0 + 1 < S ? i0 + 1 : S - 1;
    const double frac = pos - (double)i0, a = s[i0], d = s[i1] - a, fd = frac * d;
    return a + fd;
}

// the bitonic network on buf[0 .. P), ascending; P a power of two >= 2.  Ends behind a barrier.
__device__ void sort_lds(double* buf, int P) {
    const int t = threadIdx.x;
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int p = t; p < (P >> 1); p += RK_T) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const double a = buf[i], b = buf[l];
                if ((a > b) == ((i & k2) == 0)) {
                    buf[i] = b;
                    buf[l] = a;
                }
            }
            __syncthreads();
        }
}

// lo + hi + 1 = twice the average rank of x among the sorted s[0 .. S)
__device__ __forceinline__ int twice_rank(const double* s, int S, double x) {
    int lo = 0, n = S;
    while (n > 0) {                      // first index with s[i] >= x
        const int h = n >> 1;
        if (s[lo + h] < x) {
            lo += h + 1;
            n -= h + 1;
        } else
            n = h;
    }
    int hi = lo;
    n = S - lo;
    while (n > 0) {                      // first index with s[i] > x
        const int h = n >> 1;
        if (s[hi + h] <= x) {
            hi += h + 1;
            n -= h + 1;
        } else
            n = h;
    }
    return lo + hi + 1;
}

// the sum of one value per thread, the same bits in every thread: a butterfly inside each wave, then the waves in order.
// red: RK_WAVES doubles of scratch.  Ends behind a barrier that also frees red.
__device__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < RK_WAVES; ++w) s += red[w];
    __syncthreads();
    return s;
}

struct SeriesStats {
    double W, B, ess;      // within- and between-sequence variance (NaN unless W > 0), S / tau (only with want_ess)
};

// The statistics of the series in buf[0 .. S), sequence j = draws j nh .. j nh + nh - 1; buf is left centred.  Called by the
// whole workgroup, and every thread returns the same bits.
__device__ SeriesStats series(double* buf, double* sc, int m, int nh, bool want_ess) {
    const int t = threadIdx.x, S = m * nh;
    const int nc = (nh + RK_CH - 1) / RK_CH;
    const double dn = (double)nh, dm = (double)m;
    const double c0 = buf[0];
    __syncthreads();                     // everyone has c0 before buf[0] changes
    double mean[RK_MSEQ];                // of d = v - c0, sequences t + RK_T q
#pragma unroll
    for (int q = 0; q < RK_MSEQ; ++q) mean[q] = 0.0;
    if (nc == 1) {                       // a thread owns whole sequences
#pragma unroll
        for (int q = 0; q < RK_MSEQ; ++q) {
            const int j = t + RK_T * q;
            if (j < m) {
                double* v = buf + j * nh;
                double s = 0.0;
                for (int i = 0; i < nh; ++i) s += v[i] - c0;
                mean[q] = s / dn;
                for (int i = 0; i < nh; ++i) v[i] = (v[i] - c0) - mean[q];
            }
        }
    } else {                             // m nc <= SC_PART_N units, m <= SC_MEAN_N
        for (int u = t; u < m * nc; u += RK_T) {
            const int j = u / nc, c = u % nc, i1 = (c + 1) * RK_CH < nh ? (c + 1) * RK_CH : nh;
            const double* v = buf + j * nh;
            double s = 0.0;
            for (int i = c * RK_CH; i < i1; ++i) s += v[i] - c0;
            sc[SC_PART + u] = s;
        }
        __syncthreads();
        if (t < m) {
            double s = 0.0;
            for (int c = 0; c < nc; ++c) s += sc[SC_PART + t * nc + c];
            mean[0] = s / dn;
            sc[SC_MEAN + t] = mean[0];
        }
        __syncthreads();
        for (int p = t; p < S; p += RK_T) buf[p] = (buf[p] - c0) - sc[SC_MEAN + p / nh];
    }
    __syncthreads();
    double* red = sc + SC_RED;
    double ms = 0.0;
#pragma unroll
    for (int q = 0; q < RK_MSEQ; ++q) ms += (t + RK_T * q < m) ? mean[q] : 0.0;
    const double gm = block_sum(ms, red) / dm;
    double bs = 0.0;
#pragma unroll
    for (int q = 0; q < RK_MSEQ; ++q) bs += (t + RK_T * q < m) ? (mean[q] - gm) * (mean[q] - gm) : 0.0;
    const double B = dn * block_sum(bs, red) / (dm - 1.0);

    // ---- lagged products, RK_L lags at a time; Geyer's rule on the pairs (rankdiag.ess_from_acov is this loop)
    const int lag = t & (RK_L - 1), slot = t / RK_L, wave = t >> 6;
    const int npair = nh / 2, U = m * nc;
    double W = 0.0, varp = 0.0, sumP = 0.0, prev = 0.0, trail = 0.0;
    bool stopped = false;
    for (int l0 = 0; !stopped && l0 < (want_ess ? 2 * npair : 1); l0 += RK_L) {
        const int tl = l0 + lag;
        double acc = 0.0;
        if (tl < nh && (want_ess || tl == 0))
            for (int u = slot; u < U; u += RK_SLOTS) {
                const int j = u / nc, c = u % nc;
                const int e1 = (c + 1) * RK_CH < nh ? (c + 1) * RK_CH : nh, i1 = e1 < nh - tl ? e1 : nh - tl;
                const double* v = buf + j * nh;
                double s = 0.0;
                for (int i = c * RK_CH; i < i1; ++i) s += v[i] * v[i + tl];
                acc += s;
            }
#pragma unroll
        for (int o = 32; o >= RK_L; o >>= 1) acc += __shfl_xor(acc, o);
        if ((t & 63) < RK_L) red[wave * RK_L + lag] = acc;
        __syncthreads();
        if (t < RK_L) {                  // the waves in order
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < RK_WAVES; ++w) s += red[w * RK_L + t];
            red[RK_WAVES * RK_L + t] = s / dn / dm;
        }
        __syncthreads();
        double A[RK_L];                  // mean over the sequences of the biased autocovariance at lag l0 + i
#pragma unroll
        for (int i = 0; i < RK_L; ++i) A[i] = red[RK_WAVES * RK_L + i];
        __syncthreads();
        if (l0 == 0) {
            W = A[0] * dn / (dn - 1.0);
            varp = (dn - 1.0) / dn * W + B / dn;
            if (!(W > 0.0) || !want_ess) break;
        }
#pragma unroll
        for (int i = 0; i < RK_L; i += 2) {
            const int k = (l0 + i) >> 1;
            if (stopped || k >= npair) continue;
            const double re = k == 0 ? 1.0 : 1.0 - (W - A[i]) / varp, ro = 1.0 - (W - A[i + 1]) / varp, P = re + ro;
            if (k == 0) {
                sumP = prev = P;
            } else if (P > 0.0) {
                prev = P < prev ? P : prev;
                sumP += prev;
            } else {
                stopped = true;
                trail = re > 0.0 ? re : 0.0;
            }
        }
    }
    SeriesStats r;
    const double qnan = __builtin_nan("");
    const bool ok = W > 0.0;
    r.W = ok ? W : qnan;
    r.B = ok ? B : qnan;
    double tau = -1.0 + 2.0 * sumP + trail;
    const double tmin = 1.0 / log10((double)S);
    tau = tau > tmin ? tau : tmin;       // (a NaN tau cannot occur with W > 0: varp >= (n - 1) / n W > 0)
    r.ess = ok && want_ess ? (double)S / tau : qnan;
    return r;
}

__device__ __forceinline__ double split_rhat(const SeriesStats& s, int nh) {
    const double dn = (double)nh;
    return sqrt(((dn - 1.0) / dn * s.W + s.B / dn) / s.W);
}

__global__ __launch_bounds__(RK_T) void k_rank_entry(const double* __restrict__ ws, double* __restrict__ zs, int m, int nh, int P,
                                                     int64_t K, int64_t k0, double* __restrict__ out) {
    extern __shared__ __align__(16) double lds[];
    const int t = threadIdx.x, S = m * nh;
    double* buf = lds;                                   // P >= S doubles
    double* sc = lds + P;                                // RK_SCR doubles
    const double* x = ws + (int64_t)blockIdx.x * S;      // the entry's window, pooled order
    double* zt = zs + (int64_t)blockIdx.x * S;           // draw p's z between its search and the barrier: written and read by thread p % RK_T
    const int64_t k = k0 + blockIdx.x;
    int bad = 0;
    for (int p = t; p < S; p += RK_T) bad |= !isfinite(x[p]);
    if (block_sum((double)bad, sc + SC_RED) > 0.0) {      // the whole workgroup leaves (no static LDS: the dynamic part is all of it)
        if (t < QN_RANK_NOUT) out[(int64_t)t * K + k] = __builtin_nan("");
        return;
    }
    const double sp = (double)S + 0.25;
    double med = 0.0, q05 = 0.0, q95 = 0.0;
    SeriesStats bulk, fold, lo, hi, raw;
    // the five series, one after the other in the one buffer: z of x, z of |x - med| (R-hat only), the two tail indicators, x
#pragma unroll 1
    for (int pass = 0; pass < 5; ++pass) {
        if (pass < 2) {                                  // sorted -> (median, quantiles,) ranks -> z in chain order
            for (int p = t; p < P; p += RK_T) buf[p] = p < S ? (pass == 0 ? x[p] : fabs(x[p] - med)) : INFINITY;
            __syncthreads();
            sort_lds(buf, P);
            if (pass == 0) {
                med = 0.5 * (buf[(S - 1) / 2] + buf[S / 2]);
                q05 = sorted_quantile(buf, S, 0.05);
                q95 = sorted_quantile(buf, S, 0.95);
            }
#pragma unroll 1
            for (int p = t; p < S; p += RK_T) {
                const int r2 = twice_rank(buf, S, pass == 0 ? x[p] : fabs(x[p] - med));
                zt[p] = inv_normal_cdf(((double)r2 * 0.5 - 0.375) / sp);
            }
            __syncthreads();
            for (int p = t; p < S; p += RK_T) buf[p] = zt[p];
        } else {
            for (int p = t; p < S; p += RK_T) buf[p] = pass == 4 ? x[p] : (x[p] <= (pass == 2 ? q05 : q95) ? 1.0 : 0.0);
        }
        __syncthreads();
        const SeriesStats st = series(buf, sc, m, nh, pass != 1);
        __syncthreads();
        if (pass == 0) bulk = st;
        else if (pass == 1) fold = st;
        else if (pass == 2) lo = st;
        else if (pass == 3) hi = st;
        else raw = st;
    }

    if (t == 0) {
        const double dn = (double)nh, dm = (double)m;
        // the pooled sum of squares: within the sequences (n - 1) m W, between them (m - 1) B
        const double pvar = ((dn - 1.0) * dm * raw.W + (dm - 1.0) * raw.B) / ((double)S - 1.0);
        out[(int64_t)QN_RANK_RHAT_BULK * K + k] = split_rhat(bulk, nh);
        out[(int64_t)QN_RANK_RHAT_TAIL * K + k] = split_rhat(fold, nh);
        out[(int64_t)QN_RANK_ESS_BULK * K + k] = bulk.ess;
        out[(int64_t)QN_RANK_ESS_TAIL * K + k] = (isnan(lo.ess) || isnan(hi.ess)) ? __builtin_nan("") : fmin(lo.ess, hi.ess);
        out[(int64_t)QN_RANK_ESS_MEAN * K + k] = raw.ess;
        out[(int64_t)QN_RANK_MCSE_MEAN * K + k] = sqrt(pvar / raw.ess);
    }
}

// the argument checks shared by the workspace query and the call (t0 = 0 for the query); 0 = refused (message set)
size_t checked_workspace(const char* who, int C, int64_t T, int64_t K, int64_t t0, int64_t nh, int64_t stride) {
    if (C < 1 || K < 1 || nh < 4 || stride < 1 || t0 < 0) {
        qn_set_error("%s: need C >= 1 chains, K >= 1 entries, nh >= 4 draws per half, stride >= 1 and t0 >= 0 (C=%d K=%lld nh=%lld "
                     "stride=%lld t0=%lld)", who, C, (long long)K, (long long)nh, (long long)stride, (long long)t0);
        return 0;
    }
    if (nh > QN_RANK_MAX_S || 2 * (int64_t)C * nh > QN_RANK_MAX_S) {
        qn_set_error("%s: 2 C nh = %lld pooled draws, at most %d (thin with stride)", who, (long long)(2 * (int64_t)C * nh),
                     QN_RANK_MAX_S);
        return 0;
    }
    if (T < 1 || stride > T || t0 >= T || t0 + (2 * nh - 1) * stride >= T) {
        qn_set_error("%s: the window t0 + j stride, j < 2 nh, runs past T (T=%lld t0=%lld nh=%lld stride=%lld)", who, (long long)T,
                     (long long)t0, (long long)nh, (long long)stride);
        return 0;
    }
    if (K > (int64_t(1) << 31) || (double)C * (double)T * (double)K > 9.0e18) {
        qn_set_error("%s: shape too large (C=%d T=%lld K=%lld)", who, C, (long long)T, (long long)K);
        return 0;
    }
    const int64_t kc = K < RK_CHUNK ? K : RK_CHUNK;
    return 2 * qn_align((size_t)kc * (size_t)(2 * C * nh) * sizeof(double));      // the windows, and a z per draw
}

int pow2_at_least(int S) {
    int P = 2;
    while (P < S) P <<= 1;
    return P;
}

template <typename T>
int launch(const T* chain, int C, int64_t Tn, int64_t K, int64_t t0, int64_t nh, int64_t stride, double* out, double* ws,
           hipStream_t st) {
    const int m = 2 * C, S = m * (int)nh, P = pow2_at_least(S);
    const size_t lds = (size_t)(P + RK_SCR) * sizeof(double);
    if (int rc = qn_arm_lds(reinterpret_cast<const void*>(k_rank_entry), lds)) return rc;
    double* zs = ws + qn_align((size_t)(K < RK_CHUNK ? K : RK_CHUNK) * (size_t)S * sizeof(double)) / sizeof(double);
    for (int64_t k0 = 0; k0 < K; k0 += RK_CHUNK) {
        const int kc = (int)(K - k0 < RK_CHUNK ? K - k0 : RK_CHUNK);
        hipLaunchKernelGGL((k_rank_gather<T>), dim3((kc + 31) / 32, (S + 31) / 32), dim3(32, 8), 0, st, chain, Tn, K, t0, nh, stride,
                           S, k0, kc, ws);
        hipLaunchKernelGGL(k_rank_entry, dim3(kc), dim3(RK_T), lds, st, (const double*)ws, zs, m, (int)nh, P, K, k0, out);
    }
    return QN_OK;
}

}  // namespace

extern "C" size_t qn_rank_diag_workspace_bytes(int C, int64_t T, int64_t K, int64_t nh, int64_t stride) {
    return checked_workspace("qn_rank_diag_workspace_bytes", C, T, K, 0, nh, stride);
}

extern "C" int qn_rank_diag(const void* chain, int dtype, int C, int64_t T, int64_t K, int64_t t0, int64_t nh, int64_t stride,
                            double* out, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = checked_workspace("qn_rank_diag", C, T, K, t0, nh, stride);
    if (need == 0) return QN_EINVAL;
    if (dtype != QN_F64 && dtype != QN_F32) {
        qn_set_error("qn_rank_diag: dtype %d (QN_F64 or QN_F32)", dtype);
        return QN_EINVAL;
    }
    if (!chain || !out || !workspace) {
        qn_set_error("qn_rank_diag: chain, out and workspace must not be NULL");
        return QN_EINVAL;
    }
    if (workspace_bytes < need) {
        qn_set_error("qn_rank_diag: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return QN_EWORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    int rc;
    if (dtype == QN_F32)
        rc = launch(static_cast<const float*>(chain), C, T, K, t0, nh, stride, out, static_cast<double*>(workspace), st);
    else
        rc = launch(static_cast<const double*>(chain), C, T, K, t0, nh, stride, out, static_cast<double*>(workspace), st);
    if (rc) return rc;
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
