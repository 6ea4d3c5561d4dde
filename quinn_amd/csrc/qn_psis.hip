// Pareto-smoothed importance-sampling leave-one-out scores of a predictive ensemble: F [M, K] member means, optional V [M, K]
// member variances, Y [K] targets -> out [QN_LOO_NOUT, K] (elpd_loo, khat, ess, pit_loo per entry; the definitions are in
// include/quinn_amd_psis.h at qn_psis_loo, restated in numpy by quinn_amd/psis.py).  ll_mk is the log_lik of qn_score.hip, bit for
// bit; lr_m = -ll_m - max_m(-ll_m).  Three launches, F read three times, a workspace of [PS_WS_ROWS, K] doubles between them:
//
//   k_psis_max    one thread per entry, coalesced across entries (the layout of k_score_stream): mx = max_m(-ll_m), or NaN
//                 for an entry with a non-finite input or a variance <= 0 -- such an entry is skipped from here on.
//   k_psis_tail   a block of PE = 4 waves owns PE consecutive entries and walks the members in chunks of PCH = 512: the block
//                 loads the chunk (PE entries wide, so a row is one 32-byte segment of float64) and writes lr with the member
//                 index into LDS; wave e keeps entry e's largest 512 pairs in the total order (lr, m), sorted descending,
//                 in the lower half of its 1024-pair buffer: the chunk in the upper half is sorted ascending (bitonic network,
//                 pair index -> lane), then the whole buffer is one bitonic merge.  After the last chunk the first T pairs are
//                 the tail and pair T the cutoff.  The wave then fits the generalised Pareto distribution -- grid point i of
//                 the profile likelihood is lane i - 1 (m <= 49), which sums its T log1p terms in order j = 1 .. T -- forms
//                 the T smoothed log weights (six per lane in registers), reads f and V of the tail members back by index and
//                 reduces the tail's part of the four sums (a maximum, then a per-lane sum in order and a butterfly).
//   k_psis_rows   one thread per entry again: the members at or below the cutoff (lr, m) keep lw = lr, their sums are taken
//                 relative to the cutoff in member order and joined with the tail's.  ll + lw of such a member is -mx, so their
//                 part of logsumexp(ll + lw) is (M - T) exp(-mx): nothing is recovered as "all minus tail".
//
// No atomics, one writer per word, every order fixed by M alone (the rank of a tail member is a property of the entry): an
// entry's numbers do not depend on K, on the other entries of the call or on the launch geometry.
#include <cmath>

#include "qn_common.h"
#include "../../include/quinn_amd_psis.h"
#include "qn_loglik.h"

namespace {

constexpr int SBLK = 64;                 // streaming passes: one wave per block, as in qn_score.hip
constexpr int SUNROLL = 4;               // members whose loads are issued before the first is used
constexpr int PE = 4;                    // tail pass: entries (= waves) per block
constexpr int PCH = 512;                 // members per chunk
constexpr int PBUF = 2 * PCH;            // pairs per entry in LDS: the running top PCH, descending, and the chunk
constexpr int PTHREADS = 64 * PE;
constexpr int PTL = 6;                   // tail members per lane
constexpr int PS_WS_ROWS = 10;           // workspace rows, each [K]:
enum { WS_MX = 0, WS_CUT, WS_MCUT, WS_KHAT, WS_TMA, WS_TSA, WS_TMB, WS_TSB, WS_TSB2, WS_TSP };

// T = ceil(min(M / 5, 3 sqrt(M))); sqrt is correctly rounded, so this is the integer numpy forms
int tail_size(int64_t M) { return (int)std::ceil(std::fmin((double)M / 5.0, 3.0 * std::sqrt((double)M))); }

static_assert(PTL * 64 >= 384 && 385 <= PCH, "the tail of QN_PSIS_MAX_M members and its cutoff fit a lane's registers and half a buffer");
static_assert(QN_PSIS_MAX_M == 16384, "PTL and PCH are sized for T = 384");

template <typename T, bool HASV>
__global__ __launch_bounds__(SBLK) void k_psis_max(const T* __restrict__ F, const T* __restrict__ V, const double* __restrict__ Y,
                                                   int64_t M, int64_t K, double sig2, double sig2_lo, double* __restrict__ ws) {
    const int64_t k = (int64_t)blockIdx.x * SBLK + threadIdx.x;
    if (k >= K) return;
    const double y = Y[k];
    const LogNorm norm0 = log_norm(sig2, sig2_lo);
    bool bad = !isfinite(y);
    double mx = -INFINITY;
    const T* f_col = F + k;
    const T* v_col = HASV ? V + k : nullptr;
    auto member = [&](double f, double v) {
        double s2e;
        const double s2 = two_sum(sig2, v, &s2e);
        bad = bad || !isfinite(f) || !isfinite(v) || !(s2 > 0.0);
        const double nl = -log_lik(y, f, HASV ? log_norm(s2, s2e + sig2_lo) : norm0);
        mx = nl > mx ? nl : mx;
    };
    int64_t m = 0;
    for (; m + SUNROLL <= M; m += SUNROLL) {
        double f[SUNROLL], v[SUNROLL];
#pragma unroll
        for (int j = 0; j < SUNROLL; ++j) {
            f[j] = (double)f_col[(m + j) * K];
            v[j] = HASV ? (double)v_col[(m + j) * K] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < SUNROLL; ++j) member(f[j], v[j]);
    }
    for (; m < M; ++m) member((double)f_col[m * K], HASV ? (double)v_col[m * K] : 0.0);
    ws[WS_MX * K + k] = (bad || !isfinite(mx)) ? __builtin_nan("") : mx;
}

// pair (a, ia) above pair (b, ib) in the total order (lr, m)
__device__ __forceinline__ bool above(double a, int ia, double b, int ib) { return a > b || (a == b && ia > ib); }

// one compare-exchange of the bitonic network on the pairs i < l: afterwards pair i is the upper one iff desc
__device__ __forceinline__ void cmp_swap(double* key, int* idx, int i, int l, bool desc) {
    const double a = key[i], b = key[l];
    const int ia = idx[i], ib = idx[l];
    if (above(a, ia, b, ib) != desc) {
        key[i] = b;
        key[l] = a;
        idx[i] = ib;
        idx[l] = ia;
    }
}

__device__ __forceinline__ double wave_sum(double v) {          // butterfly: the same bits in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

template <typename T, bool HASV>
__global__ __launch_bounds__(PTHREADS) void k_psis_tail(const T* __restrict__ F, const T* __restrict__ V, const double* __restrict__ Y,
                                                        int64_t M, int64_t K, double sig2, double sig2_lo, int nt, int mg,
                                                        double* __restrict__ ws) {
    __shared__ double skey[PE][PBUF];
    __shared__ int sidx[PE][PBUF];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const LogNorm norm0 = log_norm(sig2, sig2_lo);

    // ---- selection: thread t loads entry le of the tile, members lr0 + 64 i of the chunk
    {
        const int le = t & (PE - 1), lr0 = t / PE;
        const int64_t k = (int64_t)blockIdx.x * PE + le;
        const bool live = k < K && !isnan(ws[WS_MX * K + (k < K ? k : K - 1)]);
        const int64_t kc = k < K ? k : K - 1;
        const double y = Y[kc], mx = ws[WS_MX * K + kc];
        for (int i = t; i < PE * PCH; i += PTHREADS) {
            skey[i / PCH][i % PCH] = -INFINITY;
            sidx[i / PCH][i % PCH] = -1;
        }
        for (int64_t c0 = 0; c0 < M; c0 += PCH) {
#pragma unroll
            for (int i = 0; i < PCH / 64; ++i) {
                const int mm = lr0 + 64 * i;
                const int64_t m = c0 + mm;
                double key = -INFINITY;
                int id = -1;
                if (live && m < M) {
                    const double f = (double)F[m * K + kc];
                    LogNorm n = norm0;
                    if (HASV) {
                        double s2e;
                        const double s2 = two_sum(sig2, (double)V[m * K + kc], &s2e);
                        n = log_norm(s2, s2e + sig2_lo);
                    }
                    key = -log_lik(y, f, n) - mx;
                    id = (int)m;
                }
                skey[le][PCH + mm] = key;
                sidx[le][PCH + mm] = id;
            }
            __syncthreads();
            // the chunk half ascending: the stages k2 <= PCH of the network on pairs PCH / 2 .. PCH - 1 (elements PCH .. PBUF - 1)
            for (int k2 = 2; k2 <= PCH; k2 <<= 1)
                for (int j = k2 >> 1; j > 0; j >>= 1) {
#pragma unroll
                    for (int q = 0; q < PCH / 128; ++q) {
                        const int p = PCH / 2 + lane + 64 * q, i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                        cmp_swap(skey[w], sidx[w], i, i | j, (i & k2) == 0);
                    }
                    __syncthreads();
                }
            // descending top half + ascending chunk half is bitonic: one merge, descending
            for (int j = PCH; j > 0; j >>= 1) {
#pragma unroll
                for (int q = 0; q < PCH / 64; ++q) {
                    const int p = lane + 64 * q, i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                    cmp_swap(skey[w], sidx[w], i, i | j, true);
                }
                __syncthreads();
            }
        }
    }

    // ---- wave w: the fit and the tail sums of entry w.  Pairs 0 .. nt - 1 are the tail, descending; pair nt is the cutoff.
    const int64_t k = (int64_t)blockIdx.x * PE + w;
    const int64_t kc = k < K ? k : K - 1;
    const double mx = ws[WS_MX * K + kc];
    const bool live = k < K && !isnan(mx);
    double* key = skey[w];
    const int* idx = sidx[w];
    double* x = key + PCH;                                       // the chunk half is free now: the ascending excesses
    const double cut = key[nt], ec = exp(cut), dn = (double)nt;
    const int mcut = idx[nt];
    for (int jj = lane; jj < nt; jj += 64) x[jj] = exp(key[nt - 1 - jj]) - ec;
    __syncthreads();
    const int q = (nt + 2) / 4 > 0 ? (nt + 2) / 4 : 1;            // floor(nt / 4 + 0.5)
    const double xq = x[q - 1], xn = x[nt - 1];
    // grid point i = lane + 1 of the profile likelihood (lanes >= mg compute a point nobody reads)
    const double bi = 1.0 / xn + (1.0 - sqrt((double)mg / ((double)lane + 0.5))) / (3.0 * xq);
    double ks = 0.0;
    for (int jj = 0; jj < nt; ++jj) ks += log1p(-bi * x[jj]);
    const double ki = ks / dn, Li = dn * (log(-bi / ki) - ki - 1.0);
    double den = 0.0;
    for (int l = 0; l < mg; ++l) den += exp(__shfl(Li, l) - Li);
    const double wi = 1.0 / den;
    double b = 0.0;
    for (int i = 0; i < mg; ++i) b += __shfl(wi, i) * __shfl(bi, i);
    double kp = 0.0;
    for (int jj = lane; jj < nt; jj += 64) kp += log1p(-b * x[jj]);
    kp = wave_sum(kp) / dn;
    const double sigma = -kp / b, khat = (dn * kp + 5.0) / (dn + 10.0);
    const bool smooth = nt >= 5 && xq > 0.0 && isfinite(khat) && isfinite(sigma);

    const double y = Y[kc];
    double a[PTL], lw[PTL], ph[PTL];
    double ma = -INFINITY, mb = -INFINITY;
#pragma unroll
    for (int i = 0; i < PTL; ++i) {
        const int jj = lane + 64 * i;                             // rank j = jj + 1 of the ascending tail
        a[i] = lw[i] = -INFINITY;
        ph[i] = 0.0;
        if (live && jj < nt && idx[nt - 1 - jj] >= 0) {
            const int pos = nt - 1 - jj;
            double l = key[pos];
            if (smooth) {
                const double l1p = log1p(-((double)jj + 0.5) / dn);
                const double qt = khat == 0.0 ? -sigma * l1p : sigma * expm1(-khat * l1p) / khat;
                l = log(ec + qt);
            }
            l = l < 0.0 ? l : 0.0;
            const int64_t m = idx[pos];
            const double f = (double)F[m * K + k];
            LogNorm n = norm0;
            double sd = sqrt(sig2);
            if (HASV) {
                double s2e;
                const double s2 = two_sum(sig2, (double)V[m * K + k], &s2e);
                n = log_norm(s2, s2e + sig2_lo);
                sd = sqrt(s2);
            }
            lw[i] = l;
            a[i] = log_lik(y, f, n) + l;
            ph[i] = 0.5 * erfc(-((y - f) / sd) * M_SQRT1_2);
            ma = fmax(ma, a[i]);
            mb = fmax(mb, l);
        }
    }
    ma = wave_max(ma);
    mb = wave_max(mb);
    double sa = 0.0, sb = 0.0, sb2 = 0.0, sp = 0.0;
#pragma unroll
    for (int i = 0; i < PTL; ++i)
        if (live && lane + 64 * i < nt) {
            const double e = exp(lw[i] - mb);
            sa += exp(a[i] - ma);
            sb += e;
            sb2 += e * e;
            sp += e * ph[i];
        }
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    sb2 = wave_sum(sb2);
    sp = wave_sum(sp);
    if (live && lane == 0) {
        ws[WS_CUT * K + k] = cut;
        ws[WS_MCUT * K + k] = (double)mcut;
        ws[WS_KHAT * K + k] = smooth ? khat : INFINITY;
        ws[WS_TMA * K + k] = ma;
        ws[WS_TSA * K + k] = sa;
        ws[WS_TMB * K + k] = mb;
        ws[WS_TSB * K + k] = sb;
        ws[WS_TSB2 * K + k] = sb2;
        ws[WS_TSP * K + k] = sp;
    }
}

template <typename T, bool HASV>
__global__ __launch_bounds__(SBLK) void k_psis_rows(const T* __restrict__ F, const T* __restrict__ V, const double* __restrict__ Y,
                                                    int64_t M, int64_t K, double sig2, double sig2_lo, int nt,
                                                    const double* __restrict__ ws, double* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * SBLK + threadIdx.x;
    if (k >= K) return;
    const double mx = ws[WS_MX * K + k];
    if (isnan(mx)) {
#pragma unroll
        for (int r = 0; r < QN_LOO_NOUT; ++r) out[r * K + k] = __builtin_nan("");
        return;
    }
    const double y = Y[k], cut = ws[WS_CUT * K + k], mcut = ws[WS_MCUT * K + k];
    const double sd0 = sqrt(sig2), inv_sd0 = 1.0 / sd0;
    const LogNorm norm0 = log_norm(sig2, sig2_lo);
    double sb = 0.0, sb2 = 0.0, sp = 0.0;                         // the members at or below the cutoff, relative to it
    const T* f_col = F + k;
    const T* v_col = HASV ? V + k : nullptr;
    auto member = [&](int64_t m, double f, double v) {
        double s2e, inv_sd = inv_sd0;
        LogNorm n = norm0;
        if (HASV) {
            const double s2 = two_sum(sig2, v, &s2e);
            n = log_norm(s2, s2e + sig2_lo);
            inv_sd = 1.0 / sqrt(s2);
        }
        // lr must come out in the bits k_psis_tail sorted: both kernels inline the same log_lik (qn_loglik.h, every fma written
        // out) on the same inputs in this one translation unit, and a member whose lr differed by an ulp at the cutoff would be
        // counted twice or not at all.  tests/test_gpu_psis.py would show it at 1e-3, not 1e-12.
        const double lr = -log_lik(y, f, n) - mx;
        if (lr > cut || (lr == cut && (double)m > mcut)) return;  // a tail member: k_psis_tail has it
        const double e = exp(lr - cut);
        sb += e;
        sb2 += e * e;
        sp += e * (0.5 * erfc(-((y - f) * inv_sd) * M_SQRT1_2));
    };
    int64_t m = 0;
    for (; m + SUNROLL <= M; m += SUNROLL) {
        double f[SUNROLL], v[SUNROLL];
#pragma unroll
        for (int j = 0; j < SUNROLL; ++j) {
            f[j] = (double)f_col[(m + j) * K];
            v[j] = HASV ? (double)v_col[(m + j) * K] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < SUNROLL; ++j) member(m + j, f[j], v[j]);
    }
    for (; m < M; ++m) member(m, (double)f_col[m * K], HASV ? (double)v_col[m * K] : 0.0);

    const double tma = ws[WS_TMA * K + k], tmb = ws[WS_TMB * K + k];
    const double mb = fmax(tmb, cut), et = exp(tmb - mb), eb = exp(cut - mb);
    const double wb = ws[WS_TSB * K + k] * et + sb * eb;
    const double wb2 = ws[WS_TSB2 * K + k] * et * et + sb2 * eb * eb;
    const double wp = ws[WS_TSP * K + k] * et + sp * eb;
    const double ma = fmax(tma, -mx);
    const double wa = ws[WS_TSA * K + k] * exp(tma - ma) + (double)(M - nt) * exp(-mx - ma);
    out[k] = (ma + log(wa)) - (mb + log(wb));
    out[K + k] = ws[WS_KHAT * K + k];
    out[2 * K + k] = wb * wb / wb2;
    out[3 * K + k] = wp / wb;
}

// the argument checks shared by the workspace query and the call; 0 = refused (message set)
size_t checked_workspace(const char* who, int64_t M, int64_t K) {
    if (M < 2 || K < 1) {
        qn_set_error("%s: need M >= 2 members and K >= 1 entries (M=%lld K=%lld)", who, (long long)M, (long long)K);
        return 0;
    }
    if (M > QN_PSIS_MAX_M) {
        qn_set_error("%s: M = %lld members, at most %d", who, (long long)M, QN_PSIS_MAX_M);
        return 0;
    }
    if (K > (int64_t(1) << 31)) {
        qn_set_error("%s: shape too large (M=%lld K=%lld)", who, (long long)M, (long long)K);
        return 0;
    }
    return qn_align((size_t)PS_WS_ROWS * (size_t)K * sizeof(double));
}

template <typename T>
void launch(const T* F, const T* V, const double* Y, int64_t M, int64_t K, double sigma, double* out, double* ws, hipStream_t st) {
    const double sig2 = sigma * sigma, sig2_lo = std::fma(sigma, sigma, -sig2);
    const int nt = tail_size(M), mg = 30 + (int)std::floor(std::sqrt((double)nt));
    const dim3 sgrid((unsigned)((K + SBLK - 1) / SBLK)), pgrid((unsigned)((K + PE - 1) / PE));
    if (V) {
        hipLaunchKernelGGL((k_psis_max<T, true>), sgrid, dim3(SBLK), 0, st, F, V, Y, M, K, sig2, sig2_lo, ws);
        hipLaunchKernelGGL((k_psis_tail<T, true>), pgrid, dim3(PTHREADS), 0, st, F, V, Y, M, K, sig2, sig2_lo, nt, mg, ws);
        hipLaunchKernelGGL((k_psis_rows<T, true>), sgrid, dim3(SBLK), 0, st, F, V, Y, M, K, sig2, sig2_lo, nt, ws, out);
    } else {
        hipLaunchKernelGGL((k_psis_max<T, false>), sgrid, dim3(SBLK), 0, st, F, V, Y, M, K, sig2, sig2_lo, ws);
        hipLaunchKernelGGL((k_psis_tail<T, false>), pgrid, dim3(PTHREADS), 0, st, F, V, Y, M, K, sig2, sig2_lo, nt, mg, ws);
        hipLaunchKernelGGL((k_psis_rows<T, false>), sgrid, dim3(SBLK), 0, st, F, V, Y, M, K, sig2, sig2_lo, nt, ws, out);
    }
}

}  // namespace

extern "C" size_t qn_psis_loo_workspace_bytes(int64_t M, int64_t K) {
    return checked_workspace("qn_psis_loo_workspace_bytes", M, K);
}

extern "C" int qn_psis_loo(const void* F, const void* V, int dtype, const double* Y, int64_t M, int64_t K, double sigma,
                           double* out, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = checked_workspace("qn_psis_loo", M, K);
    if (need == 0) return QN_EINVAL;
    if (dtype != QN_F64 && dtype != QN_F32) {
        qn_set_error("qn_psis_loo: dtype %d (QN_F64 or QN_F32)", dtype);
        return QN_EINVAL;
    }
    if (!(sigma >= 0.0) || !std::isfinite(sigma)) {
        qn_set_error("qn_psis_loo: sigma = %g (finite and >= 0)", sigma);
        return QN_EINVAL;
    }
    if (sigma == 0.0 && !V) {
        qn_set_error("qn_psis_loo: the log density needs a predictive variance (sigma = 0 and V = NULL)");
        return QN_EINVAL;
    }
    if (!F || !Y || !out || !workspace) {
        qn_set_error("qn_psis_loo: F, Y, out and workspace must not be NULL");
        return QN_EINVAL;
    }
    if (workspace_bytes < need) {
        qn_set_error("qn_psis_loo: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return QN_EWORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (dtype == QN_F32)
        launch(static_cast<const float*>(F), static_cast<const float*>(V), Y, M, K, sigma, out, static_cast<double*>(workspace), st);
    else
        launch(static_cast<const double*>(F), static_cast<const double*>(V), Y, M, K, sigma, out, static_cast<double*>(workspace), st);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
