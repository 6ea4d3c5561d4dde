// Multi-chain MCMC diagnostics: one streaming pass over a [C, T, K] stack of chains -> per-chain, per-entry statistics of
// two half-windows (split-R-hat, batch-means ESS and pooled moments are a small host combine of them; the definitions are
// in include/quinn_amd.h at qn_chain_stats).
//
//   stage 1  k_batch_stats   one thread per (chain, batch, entry k): walks the batch's `blen` rows in row order with the
//                            batch's first row as shift, x0:  s = sum (x - x0),  q = sum (x - x0)^2  (float64 whatever the
//                            input type) and writes  delta = (x0 - r_h) + s / blen  (batch mean relative to r_h, the first row
//                            of the batch's half; x0 - r_h is exact for neighbouring values) and  M2 = q - s^2 / blen  to the
//                            workspace [C, 2 nbatch, 2, K].  Consecutive threads take consecutive k, then the next batch.
//   stage 2  k_half_stats    one thread per (chain, half, k): merges the half's batches in batch order (equal counts, so
//                            Chan's merge is  M2_h = sum M2_b + blen * sum (delta_b - mean delta)^2).
//
// The chain is read once.  No atomics, one writer per output and a summation order fixed by (nbatch, blen) alone: the
// result does not depend on C, K or the launch geometry, and two calls give the same bits.  A NaN / Inf in (c, t, k) only
// ever enters sums of (c, half of t, k).
#include <algorithm>

#include "qn_common.h"

namespace {

constexpr int DBLK = 256;
constexpr int DUNROLL = 8;      // rows whose loads are issued before the first is used (scalar loads: rows of odd K are unaligned)

template <typename T>
__global__ __launch_bounds__(DBLK) void k_batch_stats(const T* __restrict__ chain, int64_t T_rows, int64_t K, int64_t t0,
                                                      int nbatch, int64_t blen, double* __restrict__ ws) {
    const int64_t NB = 2 * (int64_t)nbatch;
    const int64_t item = (int64_t)blockIdx.x * DBLK + threadIdx.x;
    if (item >= NB * K) return;
    const int c = blockIdx.y;
    const int64_t b = item / K, k = item - b * K;
    const int64_t half0 = t0 + (b >= nbatch ? (int64_t)nbatch * blen : 0);      // first row of this batch's half
    const T* base = chain + ((int64_t)c * T_rows) * K + k;
    const double rh = (double)base[half0 * K];
    const T* x = base + (t0 + b * blen) * K;
    const double x0 = (double)x[0];
    double s = 0.0, q = 0.0;
    int64_t r = 0;
    for (; r + DUNROLL <= blen; r += DUNROLL) {
        double v[DUNROLL];
#pragma unroll
        for (int j = 0; j < DUNROLL; ++j) v[j] = (double)x[(r + j) * K];
#pragma unroll
        for (int j = 0; j < DUNROLL; ++j) {
            const double d = v[j] - x0;
            s += d;
            q += d * d;
        }
    }
    for (; r < blen; ++r) {
        const double d = (double)x[r * K] - x0;
        s += d;
        q += d * d;
    }
    const double bl = (double)blen;
    double m2 = q - s * s / bl;
    if (m2 < 0.0) m2 = 0.0;                                   // rounding of a (near-)constant batch; NaN stays NaN
    double* o = ws + (((int64_t)c * NB + b) * 2) * K + k;
    o[0] = (x0 - rh) + s / bl;
    o[K] = m2;
}

template <typename T>
__global__ __launch_bounds__(DBLK) void k_half_stats(const T* __restrict__ chain, int64_t T_rows, int64_t K, int64_t t0,
                                                     int nbatch, int64_t blen, const double* __restrict__ ws,
                                                     double* __restrict__ stats) {
    const int64_t k = (int64_t)blockIdx.x * DBLK + threadIdx.x;
    if (k >= K) return;
    const int c = blockIdx.y >> 1, h = blockIdx.y & 1;
    const int64_t NB = 2 * (int64_t)nbatch;
    const double rh = (double)chain[((int64_t)c * T_rows + t0 + (int64_t)h * nbatch * blen) * K + k];
    const double* w = ws + (((int64_t)c * NB + (int64_t)h * nbatch) * 2) * K + k;
    double sd = 0.0, sm2 = 0.0;
    for (int b = 0; b < nbatch; ++b) {
        sd += w[(int64_t)b * 2 * K];
        sm2 += w[((int64_t)b * 2 + 1) * K];
    }
    const double dbar = sd / (double)nbatch;
    double sb = 0.0;
    for (int b = 0; b < nbatch; ++b) {
        const double e = w[(int64_t)b * 2 * K] - dbar;
        sb += e * e;
    }
    double* o = stats + (int64_t)c * 6 * K + k;
    o[(int64_t)h * K] = rh + dbar;
    o[(int64_t)(2 + h) * K] = sm2 + (double)blen * sb;
    o[(int64_t)(4 + h) * K] = sb;
}

// the argument checks shared by the workspace query and the call; 0 = refused (message set)
size_t checked_workspace(const char* who, int dtype, int C, int64_t T, int64_t K, int64_t t0, int nbatch, int64_t blen) {
    if (dtype != QN_F64 && dtype != QN_F32) {
        qn_set_error("%s: dtype %d (QN_F64 or QN_F32)", who, dtype);
        return 0;
    }
    if (C < 1 || C > 32767 || T < 1 || K < 1) {
        qn_set_error("%s: need 1 <= C <= 32767, T >= 1, K >= 1 (C=%d T=%lld K=%lld)", who, C, (long long)T, (long long)K);
        return 0;
    }
    // blen <= T and nbatch <= T first: the products below then stay far inside int64 for any array that fits a device
    if (nbatch < 2 || blen < 1 || t0 < 0 || blen > T || nbatch > T || 2 * (int64_t)nbatch > T / blen ||
        t0 > T - 2 * (int64_t)nbatch * blen) {
        qn_set_error("%s: need nbatch >= 2, blen >= 1, t0 >= 0 and t0 + 2 * nbatch * blen <= T (t0=%lld nbatch=%d blen=%lld T=%lld)",
                     who, (long long)t0, nbatch, (long long)blen, (long long)T);
        return 0;
    }
    const int64_t NB = 2 * (int64_t)nbatch;
    if (K > (int64_t(1) << 40) / NB || T > (int64_t(1) << 56) / K / C || (NB * K + DBLK - 1) / DBLK > 0x7fffffff) {
        qn_set_error("%s: shape too large (C=%d T=%lld K=%lld nbatch=%d)", who, C, (long long)T, (long long)K, nbatch);
        return 0;
    }
    return (size_t)C * (size_t)NB * 2 * (size_t)K * sizeof(double);
}

template <typename T>
void launch(const T* chain, int C, int64_t T_rows, int64_t K, int64_t t0, int nbatch, int64_t blen, double* stats, double* ws,
            hipStream_t st) {
    const int64_t items = 2 * (int64_t)nbatch * K;
    hipLaunchKernelGGL((k_batch_stats<T>), dim3((unsigned)((items + DBLK - 1) / DBLK), (unsigned)C), dim3(DBLK), 0, st, chain,
                       T_rows, K, t0, nbatch, blen, ws);
    hipLaunchKernelGGL((k_half_stats<T>), dim3((unsigned)((K + DBLK - 1) / DBLK), (unsigned)(2 * C)), dim3(DBLK), 0, st, chain,
                       T_rows, K, t0, nbatch, blen, ws, stats);
}

}  // namespace

extern "C" size_t qn_chain_stats_workspace_bytes(int C, int64_t T, int64_t K, int nbatch, int64_t blen) {
    return checked_workspace("qn_chain_stats_workspace_bytes", QN_F64, C, T, K, 0, nbatch, blen);
}

extern "C" int qn_chain_stats(const void* chain, int dtype, int C, int64_t T, int64_t K, int64_t t0, int nbatch,
                              int64_t blen, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = checked_workspace("qn_chain_stats", dtype, C, T, K, t0, nbatch, blen);
    if (need == 0) return QN_EINVAL;
    if (!chain || !stats || !workspace) {
        qn_set_error("qn_chain_stats: chain, stats and workspace must not be NULL");
        return QN_EINVAL;
    }
    if (workspace_bytes < need) {
        qn_set_error("qn_chain_stats: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return QN_EWORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (dtype == QN_F32)
        launch(static_cast<const float*>(chain), C, T, K, t0, nbatch, blen, stats, static_cast<double*>(workspace), st);
    else
        launch(static_cast<const double*>(chain), C, T, K, t0, nbatch, blen, stats, static_cast<double*>(workspace), st);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
