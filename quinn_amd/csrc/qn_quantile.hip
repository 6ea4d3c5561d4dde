// Quantiles of the predictive mixture that qn_pred_score scores: F [M, K] member means, optional V [M, K] member variances,
// optional wm [M] member weights, Q levels -> out [Q, K] (the definitions are in include/quinn_amd_quantile.h at qn_pred_quantile,
// written out step by step in numpy by quinn_amd/predquant.py).
//
//   k_quant_mix   mixture mode.  One thread per entry k, members walked in member order, coalesced across entries: the layout of
//                 k_score_stream (qn_score.hip), whose `pit` this inverts.  F is [M, K] with K contiguous, so lane = entry
//                 makes every load a full line, needs no cross-lane reduction and adds in member order whatever the launch; a
//                 wave per entry would read one member per lane at a stride of K.  Up to QL levels live in registers: a pass over
//                 the members forms s = sqrt(sigma^2 + v) and 1 / s once and evaluates G and the density at the iterates of all
//                 levels.  Pass 0 is the bracket and the first iterate (min, max and weighted mean of f + s z); then at most
//                 QN_QUANT_MAX_ITER passes.  A level that has stopped keeps its state; the pass itself is the same for all.
//                 More than QL levels are further launches: an entry's level never sees another level's numbers.
//   k_quant_emp   empirical mode.  One workgroup per entry sorts the members of positive weight in LDS by the bitonic network of
//                 qn_rank.hip, +Inf standing in for padding and for members without weight.  Without wm the keys alone are
//                 sorted and a thread per level reads its two order statistics.  With wm the network carries the member index
//                 as a 16-bit word beside each key and compares (f, m), so tied members keep their member order; the indices
//                 live in LDS up to 8192 padded members and in the workspace above (128 KiB of keys leave no room).  Thread t owns
//                 the sorted members t c .. t c + c - 1, c = P / threads: it adds their weights in order, the chunk sums
//                 before it in thread order, forms the positions p_i, and keeps per level the last member with p_i <= q; the
//                 largest over the workgroup is j, and the thread that owns it writes the level.
//
// No atomics, one writer per word, every order a function of M alone.
#include <cmath>

#include "qn_common.h"
#include "../../include/quinn_amd_quantile.h"

namespace {

constexpr int QL = 8;                    // levels per k_quant_mix launch
constexpr int MBLK = 64;                 // one wave per block, as k_score_stream
constexpr int ET = 1024;                 // most threads of k_quant_emp
constexpr int EW = ET / 64;
constexpr int EMP_SCR = 2 * ET + EW * QN_QUANT_MAX_Q / 2;      // doubles: chunk sums, chunk-first positions, [wave][level] ints
constexpr int EMP_LDS_IDX = 8192;        // padded members up to which the indices fit LDS beside the keys
constexpr int EMP_CHUNK = 512;           // entries per launch when the indices live in the workspace
constexpr double INV_SQRT_2PI = 0.39894228040143267794;

static_assert((size_t)(QN_QUANT_MAX_M + EMP_SCR) * sizeof(double) <= 160 * 1024 - 1024, "keys + scratch fit the CU's LDS");
static_assert((size_t)(EMP_LDS_IDX + EMP_SCR) * sizeof(double) + EMP_LDS_IDX * sizeof(uint16_t) <= 160 * 1024 - 1024, "with indices");
static_assert(QN_QUANT_MAX_M <= 65536 && QN_QUANT_MAX_M / ET <= 16, "16-bit indices, at most 16 members per thread");

struct MixLevels {
    double q[QL], z[QL];
};
struct EmpLevels {
    double q[QN_QUANT_MAX_Q];
};

__device__ __forceinline__ double spacing(double a) {        // of a >= 0: the distance to the next larger double
    return nextafter(a, INFINITY) - a;
}

template <typename T, bool HASV, int QT>
__global__ __launch_bounds__(MBLK) void k_quant_mix(const T* __restrict__ F, const T* __restrict__ V, const double* __restrict__ wm,
                                                    int64_t M, int64_t K, double sig2, MixLevels lv, int nl, int first,
                                                    double* __restrict__ out, int* __restrict__ iters) {
    const int64_t k = (int64_t)blockIdx.x * MBLK + threadIdx.x;
    if (k >= K) return;
    const T* f_col = F + k;
    const T* v_col = HASV ? V + k : nullptr;
    const double dm = (double)M, inf = INFINITY;
    double lo[QT], hi[QT], y[QT], rlo[QT], rhi[QT], e1[QT], e2[QT], res[QT];
    int cnt[QT];
    bool done[QT];
    bool bad = false, any = false;
    double smax = 0.0;
#pragma unroll
    for (int l = 0; l < QT; ++l) {
        lo[l] = inf;
        hi[l] = -inf;
        y[l] = 0.0;
    }
    // ---- pass 0: the bracket and the first iterate
    for (int64_t m = 0; m < M; ++m) {
        const double w = wm ? wm[m] : 1.0;
        if (wm) {                                               // the same in every lane
            if (!(w >= 0.0) || !isfinite(w)) bad = true;
            if (!(w > 0.0)) continue;
        }
        any = true;
        const double f = (double)f_col[m * K], v = HASV ? (double)v_col[m * K] : 0.0, s2 = sig2 + v;
        bad = bad || !isfinite(f) || !isfinite(v) || !(s2 > 0.0);
        const double s = sqrt(s2);
        smax = fmax(smax, s);
#pragma unroll
        for (int l = 0; l < QT; ++l) {
            const double a = f + s * lv.z[l];
            lo[l] = fmin(lo[l], a);
            hi[l] = fmax(hi[l], a);
            y[l] += w * a;
        }
    }
    bad = bad || !any;
#pragma unroll
    for (int l = 0; l < QT; ++l) {
        if (!wm) y[l] /= dm;
        lo[l] -= 1e-9 * (fabs(lo[l]) + smax);
        hi[l] += 1e-9 * (fabs(hi[l]) + smax);
        y[l] = fmin(fmax(y[l], lo[l]), hi[l]);
        rlo[l] = rhi[l] = inf;
        e1[l] = e2[l] = hi[l] - lo[l];
        res[l] = __builtin_nan("");
        cnt[l] = 0;
        done[l] = bad || l >= nl;
    }
    // ---- the evaluations
#pragma unroll 1
    for (int it = 1; it <= QN_QUANT_MAX_ITER; ++it) {
        bool all = true;
#pragma unroll
        for (int l = 0; l < QT; ++l) all = all && done[l];
        if (all) break;
        double G[QT], g[QT];
#pragma unroll
        for (int l = 0; l < QT; ++l) G[l] = g[l] = 0.0;
#pragma unroll 2
        for (int64_t m = 0; m < M; ++m) {
            const double w = wm ? wm[m] : 1.0;
            if (wm && !(w > 0.0)) continue;
            const double f = (double)f_col[m * K], v = HASV ? (double)v_col[m * K] : 0.0;
            const double inv_s = 1.0 / sqrt(sig2 + v);
#pragma unroll
            for (int l = 0; l < QT; ++l) {
                const double t = (y[l] - f) * inv_s;
                G[l] += w * (0.5 * erfc(-t * M_SQRT1_2));
                g[l] += w * (INV_SQRT_2PI * exp(-0.5 * t * t) * inv_s);
            }
        }
#pragma unroll
        for (int l = 0; l < QT; ++l) {
            if (done[l]) continue;
            if (!wm) {
                G[l] /= dm;
                g[l] /= dm;
            }
            cnt[l] = it;
            const double r = G[l] - lv.q[l];
            if (r == 0.0) {
                res[l] = y[l];
                done[l] = true;
                continue;
            }
            if (r < 0.0) {
                lo[l] = y[l];
                rlo[l] = -r;
            } else {
                hi[l] = y[l];
                rhi[l] = r;
            }
            if (hi[l] - lo[l] <= 2.0 * spacing(fmax(fabs(lo[l]), fabs(hi[l]))) || it == QN_QUANT_MAX_ITER) {
                res[l] = rlo[l] <= rhi[l] ? lo[l] : hi[l];
                done[l] = true;
                continue;
            }
            double step = -r / g[l];
            const double sp2 = 2.0 * spacing(fabs(y[l]));
            if (fabs(step) < sp2) step = copysign(sp2, -r);
            double yn = y[l] + step;
            const bool ok = isfinite(step) && yn > lo[l] && yn < hi[l] && fabs(step) <= 0.5 * e2[l];
            if (!ok) yn = lo[l] + 0.5 * (hi[l] - lo[l]);
            e2[l] = e1[l];
            e1[l] = fabs(yn - y[l]);
            y[l] = yn;
        }
    }
    int mx = 0;
#pragma unroll
    for (int l = 0; l < QT; ++l) {
        if (l < nl) {
            out[(int64_t)l * K + k] = res[l];
            mx = cnt[l] > mx ? cnt[l] : mx;
        }
    }
    if (iters) {
        const int was = first ? 0 : iters[k];
        iters[k] = mx > was ? mx : was;
    }
}

// numpy's two-sided interpolation: each product is rounded before its sum
__device__ __forceinline__ double lerp2(double a, double b, double g) {
#pragma clang fp contract(off)
    const double d = b - a;
    if (g < 0.5) {
        const double dg = d * g;
        return a + dg;
    }
    const double dg = d * (1.0 - g);
    return b - dg;
}

// the bitonic network on key[0 .. P) (and idx beside it when PAIRS: the order is (key, idx)), ascending; P a power of two >= 2.
// Ends behind a barrier.
template <bool PAIRS>
__device__ void sort_keys(double* key, uint16_t* idx, int P) {
    const int t = threadIdx.x, nt = blockDim.x;
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int p = t; p < (P >> 1); p += nt) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const double a = key[i], b = key[l];
                bool gt = a > b;
                uint16_t ia = 0, ib = 0;
                if (PAIRS) {
                    ia = idx[i];
                    ib = idx[l];
                    gt = gt || (a == b && ia > ib);
                }
                if (gt == ((i & k2) == 0)) {
                    key[i] = b;
                    key[l] = a;
                    if (PAIRS) {
                        idx[i] = ib;
                        idx[l] = ia;
                    }
                }
            }
            __syncthreads();
        }
}

template <typename T>
__global__ __launch_bounds__(ET) void k_quant_emp(const T* __restrict__ F, const double* __restrict__ wm, int64_t M, int64_t K,
                                                  int64_t k0, int P, EmpLevels lv, int Q, double* __restrict__ out,
                                                  uint16_t* __restrict__ gidx) {
    extern __shared__ __align__(16) double lds[];
    const int t = threadIdx.x, nt = blockDim.x;
    double* key = lds;                                   // P doubles
    double* sc = lds + P;                                // EMP_SCR doubles
    uint16_t* idx = gidx ? gidx + (size_t)blockIdx.x * (size_t)P : reinterpret_cast<uint16_t*>(sc + EMP_SCR);   // P words, only with wm
    const int64_t k = k0 + blockIdx.x;
    const double qnan = __builtin_nan("");
    int bad = 0;
    for (int p = t; p < P; p += nt) {
        const double w = p < M ? (wm ? wm[p] : 1.0) : 0.0;
        if (!(w >= 0.0) || !isfinite(w)) bad = 1;
        const bool live = p < M && w > 0.0;
        const double f = live ? (double)F[(int64_t)p * K + k] : INFINITY;
        if (live && !isfinite(f)) bad = 1;
        key[p] = f;
        if (wm) idx[p] = (uint16_t)p;
    }
    // the flag of the workgroup through the scratch: the kernel keeps no static LDS (the dynamic part may be all 160 KiB)
    int* flag = reinterpret_cast<int*>(sc);
    if (t == 0) *flag = 0;
    __syncthreads();
    if (bad) *flag = 1;
    __syncthreads();
    bad = *flag;
    if (bad) {                                           // the whole workgroup leaves
        if (t < Q) out[(int64_t)t * K + k] = qnan;
        return;
    }
    if (wm) sort_keys<true>(key, idx, P);
    else sort_keys<false>(key, idx, P);
    int n = 0;                                           // the members of weight: the keys before the first +Inf
    for (int len = P; len > 0;) {
        const int h = len >> 1;
        if (key[n + h] < INFINITY) {
            n += h + 1;
            len -= h + 1;
        } else
            len = h;
    }
    if (n <= 1) {
        if (t < Q) out[(int64_t)t * K + k] = n == 1 ? key[0] : qnan;
        return;
    }
    if (!wm) {
        if (t < Q) {
#pragma clang fp contract(off)
            const double h = lv.q[t] * (double)(n - 1);
            const int j = (int)floor(h), j1 = j + 1 < n ? j + 1 : n - 1;
            out[(int64_t)t * K + k] = lerp2(key[j], key[j1], h - (double)j);
        }
        return;
    }
    // ---- weighted: positions from the running weight sum in sorted order
    double* csum = sc;                                   // [nt] the chunks' weight sums
    double* cfirst = sc + ET;                            // [nt] the position of each chunk's first member
    int* red = reinterpret_cast<int*>(sc + 2 * ET);      // [waves][QN_QUANT_MAX_Q]
    const int c = (P + nt - 1) / nt;                     // members per thread
    const int i0 = t * c, i1 = (i0 + c < n) ? i0 + c : n;
    double own = 0.0;
    for (int i = i0; i < i1; ++i) own += wm[idx[i]];
    csum[t] = own;
    __syncthreads();
    const int tl = (n - 1) / c;                          // the thread of the last member
    double acc = 0.0, S = 0.0;                           // S: the chunk sums before this thread's, in thread order
    for (int u = 0; u < tl; ++u) {
        if (u == t) S = acc;
        acc += csum[u];
    }
    if (t >= tl) S = acc;
    double Sn = acc;                                     // the running sum at the last member, added as its thread adds it
    for (int i = tl * c; i < n; ++i) Sn += wm[idx[i]];
    const double wf = wm[idx[0]], wl = wm[idx[n - 1]];
    const double den = (Sn - 0.5 * wl) - 0.5 * wf;       // the last member's numerator: p_n = 1 exactly
    int cand[QN_QUANT_MAX_Q];
    double pc[QN_QUANT_MAX_Q], pn[QN_QUANT_MAX_Q];
#pragma unroll
    for (int l = 0; l < QN_QUANT_MAX_Q; ++l) {
        cand[l] = -1;
        pc[l] = pn[l] = 0.0;
    }
    cfirst[t] = 2.0;
    for (int i = i0; i < i1; ++i) {
        const double w = wm[idx[i]];
        S += w;
        const double p = (S - 0.5 * w - 0.5 * wf) / den;
        if (i == i0) cfirst[t] = p;
#pragma unroll
        for (int l = 0; l < QN_QUANT_MAX_Q; ++l) {
            if (l < Q) {
                if (cand[l] == i - 1 && cand[l] >= 0) pn[l] = p;
                if (i <= n - 2 && p <= lv.q[l]) {
                    cand[l] = i;
                    pc[l] = p;
                }
            }
        }
    }
    int jm[QN_QUANT_MAX_Q];
#pragma unroll
    for (int l = 0; l < QN_QUANT_MAX_Q; ++l) {
        int v = cand[l];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int u = __shfl_xor(v, o);
            v = u > v ? u : v;
        }
        jm[l] = v;
    }
    if ((t & 63) == 0) {
#pragma unroll
        for (int l = 0; l < QN_QUANT_MAX_Q; ++l) red[(t >> 6) * QN_QUANT_MAX_Q + l] = jm[l];
    }
    __syncthreads();
    const int nw = (nt + 63) >> 6;
#pragma unroll
    for (int l = 0; l < QN_QUANT_MAX_Q; ++l) {
        if (l >= Q) continue;
        int j = -1;
        for (int w = 0; w < nw; ++w) {
            const int u = red[w * QN_QUANT_MAX_Q + l];
            j = u > j ? u : j;
        }
        if (j < 0 || cand[l] != j) continue;             // the position of the first member is 0 <= q: some thread owns j
        const double pnext = j + 1 < i1 ? pn[l] : cfirst[t + 1];          // j <= n - 2: member j + 1 is this chunk's or the next's first
        const double dp = pnext - pc[l];
        double g = dp > 0.0 ? (lv.q[l] - pc[l]) / dp : 0.0;
        g = g < 0.0 ? 0.0 : (g > 1.0 ? 1.0 : g);
        out[(int64_t)l * K + k] = lerp2(key[j], key[j + 1], g);
    }
}

// Phi^-1 by Wichura's AS241 (PPND16, Appl. Statist. 37, 1988) with all three branches, on the host: a level may lie anywhere in
// (0, 1), and its z only places the first bracket.  (qn_rank.hip keeps its own device copy of the two branches its arguments
// can reach.)
double inv_normal_cdf_host(double p) {
    const double q = p - 0.5;
    if (std::fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                              1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                                2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                              4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    double r = std::sqrt(-std::log(q <= 0.0 ? p : 1.0 - p));
    double num, den;
    if (r <= 5.0) {
        r -= 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                   1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                   1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                 2.05319162663775882187e+0) * r + 1.0);
    } else {
        r -= 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                   2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                   7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                 5.99832206555887937690e-1) * r + 1.0);
    }
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

int pow2_at_least(int64_t M) {
    int P = 2;
    while (P < M) P <<= 1;
    return P;
}

// the shape checks shared by the workspace query and the call; 0 = refused (message set)
size_t checked_workspace(const char* who, int64_t M, int64_t K, int Q, int empirical) {
    if (M < 1 || M > QN_QUANT_MAX_M) {
        qn_set_error("%s: M = %lld members, 1 .. %d are needed", who, (long long)M, QN_QUANT_MAX_M);
        return 0;
    }
    if (K < 1 || K > (int64_t(1) << 31)) {
        qn_set_error("%s: K = %lld entries, 1 .. 2^31 are needed", who, (long long)K);
        return 0;
    }
    if (Q < 1 || Q > QN_QUANT_MAX_Q) {
        qn_set_error("%s: Q = %d levels, 1 .. %d are needed", who, Q, QN_QUANT_MAX_Q);
        return 0;
    }
    const int P = pow2_at_least(M);
    if (!empirical || P <= EMP_LDS_IDX) return qn_align(1);
    return qn_align((size_t)(K < EMP_CHUNK ? K : EMP_CHUNK) * (size_t)P * sizeof(uint16_t));
}

template <typename T, bool HASV>
void launch_mix(const T* F, const T* V, const double* wm, int64_t M, int64_t K, double sig2, const double* q, int Q, double* out,
                int* iters, hipStream_t st) {
    const dim3 grid((unsigned)((K + MBLK - 1) / MBLK));
    for (int l0 = 0; l0 < Q; l0 += QL) {
        const int nl = Q - l0 < QL ? Q - l0 : QL;
        MixLevels lv;
        for (int l = 0; l < QL; ++l) {
            lv.q[l] = q[l0 + (l < nl ? l : 0)];
            lv.z[l] = inv_normal_cdf_host(lv.q[l]);
        }
        double* o = out + (int64_t)l0 * K;
        const int first = l0 == 0;
        if (nl == 1) hipLaunchKernelGGL((k_quant_mix<T, HASV, 1>), grid, dim3(MBLK), 0, st, F, V, wm, M, K, sig2, lv, nl, first, o, iters);
        else if (nl == 2) hipLaunchKernelGGL((k_quant_mix<T, HASV, 2>), grid, dim3(MBLK), 0, st, F, V, wm, M, K, sig2, lv, nl, first, o, iters);
        else if (nl <= 4) hipLaunchKernelGGL((k_quant_mix<T, HASV, 4>), grid, dim3(MBLK), 0, st, F, V, wm, M, K, sig2, lv, nl, first, o, iters);
        else hipLaunchKernelGGL((k_quant_mix<T, HASV, QL>), grid, dim3(MBLK), 0, st, F, V, wm, M, K, sig2, lv, nl, first, o, iters);
    }
}

template <typename T>
int launch_emp(const T* F, const double* wm, int64_t M, int64_t K, const double* q, int Q, double* out, int* iters, void* ws,
               hipStream_t st) {
    const int P = pow2_at_least(M);
    const int nt = P / 2 < 64 ? 64 : (P / 2 > ET ? ET : P / 2);
    const bool in_ws = wm && P > EMP_LDS_IDX;
    const size_t lds = (size_t)(P + EMP_SCR) * sizeof(double) + ((wm && !in_ws) ? (size_t)P * sizeof(uint16_t) : 0);
    if (int rc = qn_arm_lds(reinterpret_cast<const void*>(k_quant_emp<T>), lds)) return rc;
    EmpLevels lv;
    for (int l = 0; l < QN_QUANT_MAX_Q; ++l) lv.q[l] = q[l < Q ? l : 0];
    if (iters) QN_HIP_CHECK(hipMemsetAsync(iters, 0, (size_t)K * sizeof(int), st));
    const int64_t chunk = in_ws ? EMP_CHUNK : K;
    for (int64_t k0 = 0; k0 < K; k0 += chunk) {
        const int64_t kc = K - k0 < chunk ? K - k0 : chunk;
        hipLaunchKernelGGL(k_quant_emp<T>, dim3((unsigned)kc), dim3(nt), lds, st, F, wm, M, K, k0, P, lv, Q, out,
                           in_ws ? static_cast<uint16_t*>(ws) : nullptr);
    }
    return QN_OK;
}

}  // namespace

extern "C" size_t qn_pred_quantile_workspace_bytes(int64_t M, int64_t K, int Q, int empirical) {
    return checked_workspace("qn_pred_quantile_workspace_bytes", M, K, Q, empirical);
}

extern "C" int qn_pred_quantile(const void* F, const void* V, int dtype, const double* wm, int64_t M, int64_t K, double sigma,
                                const double* q, int Q, double* out, int* iters, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const bool sigma_ok = sigma >= 0.0 && std::isfinite(sigma);
    const int empirical = sigma_ok && sigma == 0.0 && !V;
    const size_t need = checked_workspace("qn_pred_quantile", M, K, Q, empirical);
    if (need == 0) return QN_EINVAL;
    if (dtype != QN_F64 && dtype != QN_F32) {
        qn_set_error("qn_pred_quantile: dtype %d (QN_F64 or QN_F32)", dtype);
        return QN_EINVAL;
    }
    if (!sigma_ok) {
        qn_set_error("qn_pred_quantile: sigma = %g (finite and >= 0)", sigma);
        return QN_EINVAL;
    }
    if (!q) {
        qn_set_error("qn_pred_quantile: q (the levels, host memory) must not be NULL");
        return QN_EINVAL;
    }
    for (int l = 0; l < Q; ++l) {
        const bool ok = empirical ? (q[l] >= 0.0 && q[l] <= 1.0) : (q[l] > 0.0 && q[l] < 1.0);
        if (!ok) {
            qn_set_error("qn_pred_quantile: level %d is %g (%s)", l, q[l],
                         empirical ? "0 <= q <= 1 in empirical mode" : "0 < q < 1 in mixture mode: sigma > 0 or V given");
            return QN_EINVAL;
        }
    }
    if (!F || !out || !workspace) {
        qn_set_error("qn_pred_quantile: F, out and workspace must not be NULL");
        return QN_EINVAL;
    }
    if (workspace_bytes < need) {
        qn_set_error("qn_pred_quantile: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return QN_EWORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    int rc = QN_OK;
    const double sig2 = sigma * sigma;
    if (empirical) {
        if (dtype == QN_F32) rc = launch_emp(static_cast<const float*>(F), wm, M, K, q, Q, out, iters, workspace, st);
        else rc = launch_emp(static_cast<const double*>(F), wm, M, K, q, Q, out, iters, workspace, st);
    } else if (dtype == QN_F32) {
        if (V) launch_mix<float, true>(static_cast<const float*>(F), static_cast<const float*>(V), wm, M, K, sig2, q, Q, out, iters, st);
        else launch_mix<float, false>(static_cast<const float*>(F), nullptr, wm, M, K, sig2, q, Q, out, iters, st);
    } else {
        if (V) launch_mix<double, true>(static_cast<const double*>(F), static_cast<const double*>(V), wm, M, K, sig2, q, Q, out, iters, st);
        else launch_mix<double, false>(static_cast<const double*>(F), nullptr, wm, M, K, sig2, q, Q, out, iters, st);
    }
    if (rc) return rc;
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
