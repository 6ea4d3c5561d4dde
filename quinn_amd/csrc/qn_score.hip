// Scores of a predictive ensemble against data: F [M, K] member means (K = N * o entries), optional V [M, K] member
// variances, Y [K] targets -> out [QN_SCORE_NOUT, K] (lppd, p_waic, pit, crps, mean, var per entry; the definitions are in
// include/quinn_amd.h at qn_pred_score).  Member m predicts N(f_mk, s_mk^2), s_mk^2 = sigma^2 + V_mk.
//
//   k_score_stream   one thread per entry k, one pass over the members in member order, coalesced across entries (the
//                    layout of k_pred_moments, qn_api.hip).  ll with its roundings carried along (log_lik), online
//                    log-sum-exp (running maximum), Welford for the two variances (identical members give exactly 0; a
//                    common offset costs no digits), Phi through erfc.
//                    Writes rows 0, 1, 2, 4, 5 and (1/M) sum_i A(y - f_i, s_i^2), a running mean, into row 3.
//   k_score_pairs    sum_i sum_j A(f_i - f_j, s_i^2 + s_j^2) over j < i.  A block owns a tile of PT = 64 entries (lane =
//                    entry, so every global and LDS access is contiguous across lanes) and PIB = 32 members i: wave w holds
//                    members i0 + 8 w .. + 7 in registers and walks j = 0 .. i in chunks of PJC = 32 members staged in LDS.
//                    Chunks below the diagonal chunk need no test; in the diagonal chunk `j < i` is wave-uniform (i and j are
//                    the same in every lane).  Every (i, k) sum runs over j ascending; a thread adds its 8 members in
//                    order, the block its 4 waves in order, and writes  2 * (sum over j < i) + (diagonal terms)  to
//                    parts [i-block, K].
//   k_score_finish   row 3 -= (sum of the entry's parts in block order) / (2 M^2).
//
// No atomics, one writer per output, every order fixed by M alone: an entry's numbers do not depend on K, on the other
// entries of the call or on the launch geometry, and two calls give the same bits.
#include <cmath>

#include "qn_common.h"
#include "qn_loglik.h"

namespace {

constexpr int SBLK = 64;                 // streaming pass: one wave per block, so that a few thousand entries already spread over the CUs
constexpr int SUNROLL = 4;               // members whose loads are issued before the first is used
constexpr int PT = 64;                   // pair pass: entries per tile (= lanes of a wave)
constexpr int PW = 4;                    // waves per block
constexpr int PR = 8;                    // members i per thread
constexpr int PIB = PW * PR;             // members i per block
constexpr int PJC = PIB;                 // members j per staged chunk; equal to PIB, so the diagonal chunk is a block's last
constexpr int ALL_BITS = QN_SCORE_LPPD | QN_SCORE_PWAIC | QN_SCORE_PIT | QN_SCORE_CRPS | QN_SCORE_MOMENTS;

constexpr double INV_SQRT_2PI = 0.39894228040143267794;

// A(mu, sd^2) = 2 sd phi(mu / sd) + mu (2 Phi(mu / sd) - 1) for sd > 0 (inv_sd = 1 / sd)
__device__ __forceinline__ double crps_a(double mu, double sd, double inv_sd) {
    const double z = mu * inv_sd;
    return sd * (2.0 * INV_SQRT_2PI) * exp(-0.5 * z * z) + mu * erf(z * M_SQRT1_2);
}

template <typename T, bool HASV>
__global__ __launch_bounds__(SBLK) void k_score_stream(const T* __restrict__ F, const T* __restrict__ V,
                                                       const double* __restrict__ Y, int64_t M, int64_t K, double sig2, double sig2_lo,
                                                       int what, double* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * SBLK + threadIdx.x;
    if (k >= K) return;
    const bool want_ll = what & (QN_SCORE_LPPD | QN_SCORE_PWAIC), want_pit = what & QN_SCORE_PIT;
    const bool want_crps = what & QN_SCORE_CRPS;
    const double y = Y[k];
    // without V every member has the same s^2: its root, reciprocals and log term are formed once
    const double sd0 = sqrt(sig2), inv_sd0 = 1.0 / sd0;
    const LogNorm norm0 = log_norm(sig2, sig2_lo);            // sigma^2 = sig2 + sig2_lo
    bool bad = !isfinite(y), zero_s = false;
    double lmax = 0.0, lsum = 0.0;                // log-sum-exp: sum_m exp(ll_m - lmax)
    double lmean = 0.0, lm2 = 0.0;                // Welford on ll
    double fmean = 0.0, fm2 = 0.0;                // Welford on f
    double pit = 0.0, c1 = 0.0;
    const T* f_col = F + k;
    const T* v_col = HASV ? V + k : nullptr;

    auto member = [&](int64_t m, double f, double v) {
        double s2e;
        const double s2 = two_sum(sig2, v, &s2e), r = y - f, n = (double)(m + 1);
        bad = bad || !isfinite(f) || !isfinite(v) || !(s2 >= 0.0);
        double sd = sd0, inv_sd = inv_sd0;
        if (HASV) {
            sd = sqrt(s2);
            inv_sd = 1.0 / sd;
            zero_s = zero_s || s2 == 0.0;
        }
        const bool pos = s2 > 0.0;
        if (want_ll) {
            const double ll = log_lik(y, f, HASV ? log_norm(s2, s2e + sig2_lo) : norm0);
            if (m == 0) {
                lmax = ll;
                lsum = 1.0;
            } else if (ll > lmax) {
                lsum = lsum * exp(lmax - ll) + 1.0;
                lmax = ll;
            } else {
                lsum += exp(ll - lmax);
            }
            const double d = ll - lmean;
            lmean += d / n;
            lm2 += d * (ll - lmean);
        }
        {
            const double d = f - fmean;
            fmean += d / n;
            fm2 += d * (f - fmean);
        }
        if (want_pit) pit += pos ? 0.5 * erfc(-(r * inv_sd) * M_SQRT1_2) : (r > 0.0 ? 1.0 : (r == 0.0 ? 0.5 : 0.0));
        if (want_crps) c1 += ((pos ? crps_a(r, sd, inv_sd) : fabs(r)) - c1) / n;      // running mean: exact for identical members
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

    const double nan = __builtin_nan(""), dm = (double)M;
    if (what & QN_SCORE_LPPD) out[k] = (bad || zero_s) ? nan : lmax + log(lsum) - log(dm);
    if (what & QN_SCORE_PWAIC) out[K + k] = (bad || zero_s) ? nan : lm2 / (dm - 1.0);
    if (want_pit) out[2 * K + k] = bad ? nan : pit / dm;
    if (want_crps) out[3 * K + k] = bad ? nan : c1;
    if (what & QN_SCORE_MOMENTS) {
        out[4 * K + k] = bad ? nan : fmean;
        out[5 * K + k] = bad ? nan : fm2 / (dm - 1.0);
    }
}

// MODE 0: every s = 0 (A = |mu|);  1: one s^2 = sig2 > 0 for all members;  2: per-member s^2 = sig2 + V (may be 0)
template <int MODE>
__device__ __forceinline__ double pair_a(double mu, double vsum, double sdc, double inv_sdc) {
    if (MODE == 0) return fabs(mu);
    if (MODE == 1) return crps_a(mu, sdc, inv_sdc);
    if (vsum > 0.0) {
        const double sd = sqrt(vsum);
        return crps_a(mu, sd, 1.0 / sd);
    }
    return vsum == 0.0 ? fabs(mu) : __builtin_nan("");
}

template <typename T, int MODE>
__global__ __launch_bounds__(PT * PW) void k_score_pairs(const T* __restrict__ F, const T* __restrict__ V, int64_t M, int64_t K,
                                                         double sig2, double* __restrict__ parts) {
    __shared__ double sf[PJC][PT];
    __shared__ double sv[MODE == 2 ? PJC : 1][PT];
    __shared__ double red[PW][PT];
    const int lane = threadIdx.x & (PT - 1), w = threadIdx.x / PT;
    const int64_t k = (int64_t)blockIdx.x * PT + lane;
    const int64_t kc = k < K ? k : K - 1;                       // lanes past the last entry read the last one and write nothing
    const int64_t ib = blockIdx.y, i0 = ib * PIB + (int64_t)w * PR;
    const double sdc = sqrt(2.0 * sig2), inv_sdc = 1.0 / sdc;     // MODE 1: the root of s_i^2 + s_j^2 = 2 sig2
    double fi[PR], vi[PR], acc[PR];
#pragma unroll
    for (int r = 0; r < PR; ++r) {
        const int64_t ic = i0 + r < M ? i0 + r : M - 1;         // members past the last are left out of the sum below
        fi[r] = (double)F[ic * K + kc];
        vi[r] = MODE == 2 ? sig2 + (double)V[ic * K + kc] : sig2;
        acc[r] = 0.0;
    }
    const int64_t jend = (ib + 1) * PIB < M ? (ib + 1) * PIB : M;
    for (int64_t j0 = 0; j0 < jend; j0 += PJC) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PJC / PW; ++q) {
            const int row = w + PW * q;
            if (j0 + row < jend) {
                sf[row][lane] = (double)F[(j0 + row) * K + kc];
                if (MODE == 2) sv[row][lane] = sig2 + (double)V[(j0 + row) * K + kc];
            }
        }
        __syncthreads();
        const int jn = jend - j0 < PJC ? (int)(jend - j0) : PJC;
        if (j0 + PJC <= ib * PIB) {                             // below the diagonal chunk: j < i for every i of the block
            for (int jj = 0; jj < jn; ++jj) {
                const double fj = sf[jj][lane], vj = MODE == 2 ? sv[jj][lane] : sig2;
#pragma unroll
                for (int r = 0; r < PR; ++r) acc[r] += pair_a<MODE>(fi[r] - fj, vi[r] + vj, sdc, inv_sdc);
            }
        } else {
            for (int jj = 0; jj < jn && j0 + jj < i0 + PR - 1; ++jj) {
                const int64_t j = j0 + jj;
                const double fj = sf[jj][lane], vj = MODE == 2 ? sv[jj][lane] : sig2;
#pragma unroll
                for (int r = 0; r < PR; ++r)
                    if (j < i0 + r) acc[r] += pair_a<MODE>(fi[r] - fj, vi[r] + vj, sdc, inv_sdc);
            }
        }
    }
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < PR; ++r)
        if (i0 + r < M) t += 2.0 * acc[r] + pair_a<MODE>(0.0, vi[r] + vi[r], sdc, inv_sdc);
    red[w][lane] = t;
    __syncthreads();
    if (w == 0 && k < K) {
        double p = red[0][lane];
#pragma unroll
        for (int q = 1; q < PW; ++q) p += red[q][lane];
        parts[ib * K + k] = p;
    }
}

__global__ __launch_bounds__(256) void k_score_finish(const double* __restrict__ parts, int64_t nib, int64_t M, int64_t K,
                                                      double* __restrict__ crps) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int64_t b = 0; b < nib; ++b) s += parts[b * K + k];
    const double dm = (double)M;
    crps[k] -= s / (2.0 * dm * dm);
}

// the argument checks shared by the workspace query and the call; 0 = refused (message set).  A call that does not ask for
// the CRPS needs no workspace and is told one alignment unit, so that 0 always means "refused".
size_t checked_workspace(const char* who, int64_t M, int64_t K, int what) {
    if (M < 2 || K < 1) {
        qn_set_error("%s: need M >= 2 members and K >= 1 entries (M=%lld K=%lld)", who, (long long)M, (long long)K);
        return 0;
    }
    if (what == 0 || (what & ~ALL_BITS)) {
        qn_set_error("%s: what = %d (a non-empty OR of the QN_SCORE_ bits, at most %d)", who, what, ALL_BITS);
        return 0;
    }
    const int64_t nib = (M + PIB - 1) / PIB;
    if (nib > 65535 || K > (int64_t(1) << 36) || M > (int64_t(1) << 56) / K) {
        qn_set_error("%s: shape too large (M=%lld K=%lld)", who, (long long)M, (long long)K);
        return 0;
    }
    return (what & QN_SCORE_CRPS) ? qn_align((size_t)nib * (size_t)K * sizeof(double)) : qn_align(1);
}

template <typename T>
void launch(const T* F, const T* V, const double* Y, int64_t M, int64_t K, double sigma, int what, double* out, double* parts,
            hipStream_t st) {
    const double sig2 = sigma * sigma, sig2_lo = std::fma(sigma, sigma, -sig2);
    const dim3 sgrid((unsigned)((K + SBLK - 1) / SBLK));
    if (V) hipLaunchKernelGGL((k_score_stream<T, true>), sgrid, dim3(SBLK), 0, st, F, V, Y, M, K, sig2, sig2_lo, what,
                              out);
    else hipLaunchKernelGGL((k_score_stream<T, false>), sgrid, dim3(SBLK), 0, st, F, V, Y, M, K, sig2, sig2_lo, what, out);
    if (!(what & QN_SCORE_CRPS)) return;
    const int64_t nib = (M + PIB - 1) / PIB;
    const dim3 pgrid((unsigned)((K + PT - 1) / PT), (unsigned)nib);
    if (V) hipLaunchKernelGGL((k_score_pairs<T, 2>), pgrid, dim3(PT * PW), 0, st, F, V, M, K, sig2, parts);
    else if (sigma > 0.0) hipLaunchKernelGGL((k_score_pairs<T, 1>), pgrid, dim3(PT * PW), 0, st, F, V, M, K, sig2, parts);
    else hipLaunchKernelGGL((k_score_pairs<T, 0>), pgrid, dim3(PT * PW), 0, st, F, V, M, K, sig2, parts);
    hipLaunchKernelGGL(k_score_finish, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, parts, nib, M, K, out + 3 * K);
}

}  // namespace

extern "C" size_t qn_pred_score_workspace_bytes(int64_t M, int64_t K, int what) {
    return checked_workspace("qn_pred_score_workspace_bytes", M, K, what);
}

extern "C" int qn_pred_score(const void* F, const void* V, int dtype, const double* Y, int64_t M, int64_t K, double sigma,
                             int what, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = checked_workspace("qn_pred_score", M, K, what);
    if (need == 0) return QN_EINVAL;
    if (dtype != QN_F64 && dtype != QN_F32) {
        qn_set_error("qn_pred_score: dtype %d (QN_F64 or QN_F32)", dtype);
        return QN_EINVAL;
    }
    if (!(sigma >= 0.0) || !std::isfinite(sigma)) {
        qn_set_error("qn_pred_score: sigma = %g (finite and >= 0)", sigma);
        return QN_EINVAL;
    }
    if (sigma == 0.0 && !V && (what & (QN_SCORE_LPPD | QN_SCORE_PWAIC | QN_SCORE_PIT))) {
        qn_set_error("qn_pred_score: lppd, p_waic and pit need a predictive variance (sigma = 0 and V = NULL)");
        return QN_EINVAL;
    }
    if (!F || !Y || !out || ((what & QN_SCORE_CRPS) && !workspace)) {
        qn_set_error("qn_pred_score: F, Y, out and (for the CRPS) workspace must not be NULL");
        return QN_EINVAL;
    }
    if (workspace_bytes < need) {
        qn_set_error("qn_pred_score: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return QN_EWORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (dtype == QN_F32)
        launch(static_cast<const float*>(F), static_cast<const float*>(V), Y, M, K, sigma, what, out,
               static_cast<double*>(workspace), st);
    else
        launch(static_cast<const double*>(F), static_cast<const double*>(V), Y, M, K, sigma, what, out,
               static_cast<double*>(workspace), st);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
