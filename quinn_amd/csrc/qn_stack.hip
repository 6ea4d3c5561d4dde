// Stacking of predictive distributions (include/quinn_amd_stack.h; quinn_amd/stacking.py is the contract in numpy).
//
//   k_group_lpd      one thread per entry k, one pass over the members in member order, coalesced across entries: the
//                    streaming pass of qn_score.hip with the online log-sum-exp restarted at every group boundary.  The
//                    G + 1 offsets sit in the workspace (uniform loads).  Writes L [G, K].
//   k_stack_prep     one thread per entry: m_k, E_gk = exp(L_gk - m_k) and the entry's count of NaN / +Inf elements.
//   k_stack_iter     launch t of the EM iteration.  Every workgroup first adds the previous launch's per-block partial sums in
//                    block order (so all of them hold the same grad, obj and K'), decides whether iterate t - 1 stops -- block
//                    0 then writes w, the status and the done flag, and everybody returns -- or forms w_t; then block b walks
//                    its tiles of TK = 256 entries (b, b + nb, ...): mix_k over g ascending, r_k = 1 / mix_k, and for every g
//                    the sum of E_gk r_k over its entries (thread: tile order; wave: xor butterfly; block: waves in order)
//                    into parts [t & 1][b].  w and parts are double-buffered on t, so that a launch never reads what it writes.
//   k_scorew_stream, k_scorew_pairs, k_scorew_finish   the three kernels of qn_score.hip with member weights: weighted online
//                    log-sum-exp, West's weighted Welford recurrence, and the pair sum with wm_i wm_j; a member of weight 0
//                    is skipped by a wave-uniform branch (the weights are the same in every lane).
//
// No atomics, one writer per output, every order fixed by the shape alone.
#include <cmath>

#include "qn_common.h"
#include "qn_loglik.h"
#include "../../include/quinn_amd_stack.h"

namespace {

constexpr int SBLK = 64;                 // streaming passes: one wave per block
constexpr int SUNROLL = 4;               // members whose loads are issued before the first is used
constexpr int TK = 256;                  // stack iteration: entries per tile = threads per block
constexpr int TW = TK / 64;              // its waves
constexpr int NBMAX = 256;               // its blocks at most
constexpr int GMAX = QN_STACK_MAX_G;
constexpr int XC = 3;                    // columns of a partial-sum row after the G of grad: obj, K', n_nonfinite
constexpr int PT = 64, PW = 4, PR = 8, PIB = PW * PR, PJC = PIB;        // pair pass: the tiling of qn_score.hip
constexpr int ALL_BITS = QN_SCORE_LPPD | QN_SCORE_PWAIC | QN_SCORE_PIT | QN_SCORE_CRPS | QN_SCORE_MOMENTS;
constexpr double INV_SQRT_2PI = 0.39894228040143267794;

__device__ __forceinline__ double crps_a(double mu, double sd, double inv_sd) {
    const double z = mu * inv_sd;
    return sd * (2.0 * INV_SQRT_2PI) * exp(-0.5 * z * z) + mu * erf(z * M_SQRT1_2);
}

// ---------------------------------------------------------------------------------------------------- qn_group_lpd
template <typename T, bool HASV>
__global__ __launch_bounds__(SBLK) void k_group_lpd(const T* __restrict__ F, const T* __restrict__ V, const double* __restrict__ Y,
                                                    int64_t K, double sig2, double sig2_lo, const int64_t* __restrict__ off,
                                                    int64_t G, double* __restrict__ L) {
    const int64_t k = (int64_t)blockIdx.x * SBLK + threadIdx.x;
    if (k >= K) return;
    const double y = Y[k];
    const LogNorm norm0 = log_norm(sig2, sig2_lo);
    const T* f_col = F + k;
    const T* v_col = HASV ? V + k : nullptr;
    const double nan = __builtin_nan("");
    for (int64_t g = 0; g < G; ++g) {
        const int64_t m0 = off[g], m1 = off[g + 1];
        bool bad = !isfinite(y);
        double lmax = 0.0, lsum = 0.0;
        auto member = [&](int64_t m, double f, double v) {
            double s2e;
            const double s2 = two_sum(sig2, v, &s2e);
            bad = bad || !isfinite(f) || !isfinite(v) || !(s2 > 0.0);
            const double ll = log_lik(y, f, HASV ? log_norm(s2, s2e + sig2_lo) : norm0);
            if (m == m0) {
                lmax = ll;
                lsum = 1.0;
            } else if (ll > lmax) {
                lsum = lsum * exp(lmax - ll) + 1.0;
                lmax = ll;
            } else {
                lsum += exp(ll - lmax);
            }
        };
        int64_t m = m0;
        for (; m + SUNROLL <= m1; m += SUNROLL) {
            double f[SUNROLL], v[SUNROLL];
#pragma unroll
            for (int j = 0; j < SUNROLL; ++j) {
                f[j] = (double)f_col[(m + j) * K];
                v[j] = HASV ? (double)v_col[(m + j) * K] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < SUNROLL; ++j) member(m + j, f[j], v[j]);
        }
        for (; m < m1; ++m) member(m, (double)f_col[m * K], HASV ? (double)v_col[m * K] : 0.0);
        L[g * K + k] = bad ? nan : lmax + log(lsum) - log((double)(m1 - m0));
    }
}

bool score_args_ok(const char* who, int dtype, double sigma, bool needs_var, bool has_v) {
    if (dtype != QN_F64 && dtype != QN_F32) {
        qn_set_error("%s: dtype %d (QN_F64 or QN_F32)", who, dtype);
        return false;
    }
    if (!(sigma >= 0.0) || !std::isfinite(sigma)) {
        qn_set_error("%s: sigma = %g (finite and >= 0)", who, sigma);
        return false;
    }
    if (sigma == 0.0 && !has_v && needs_var) {
        qn_set_error("%s: the log density needs a predictive variance (sigma = 0 and V = NULL)", who);
        return false;
    }
    return true;
}

size_t lpd_workspace(const char* who, int64_t M, int64_t K, int64_t G) {
    if (M < 1 || K < 1 || G < 1 || G > M) {
        qn_set_error("%s: need M >= 1 members, K >= 1 entries and 1 <= G <= M groups (M=%lld K=%lld G=%lld)", who, (long long)M,
                     (long long)K, (long long)G);
        return 0;
    }
    if (K > (int64_t(1) << 36) || M > (int64_t(1) << 56) / K) {
        qn_set_error("%s: shape too large (M=%lld K=%lld)", who, (long long)M, (long long)K);
        return 0;
    }
    return qn_align((size_t)(G + 1) * sizeof(int64_t));
}

// ---------------------------------------------------------------------------------------------------- qn_stack_weights
struct StackWs {
    double *E, *mk, *nf, *rk, *parts, *wbuf;
    int nb;
    size_t bytes;
};

StackWs stack_layout(void* base, int64_t G, int64_t K) {
    StackWs s;
    const int64_t ntiles = (K + TK - 1) / TK;
    s.nb = (int)(ntiles < NBMAX ? ntiles : NBMAX);
    double* p = static_cast<double*>(base);
    s.E = p;
    s.mk = s.E + (size_t)G * K;
    s.nf = s.mk + K;
    s.rk = s.nf + K;
    s.parts = s.rk + K;
    s.wbuf = s.parts + (size_t)2 * s.nb * (G + XC);
    s.bytes = qn_align((size_t)((s.wbuf + 2 * G) - p) * sizeof(double));
    return s;
}

size_t stack_workspace(const char* who, int64_t G, int64_t K) {
    if (G < 1 || G > GMAX) {
        qn_set_error("%s: need 1 <= G <= %d groups (G=%lld)", who, GMAX, (long long)G);
        return 0;
    }
    if (K < 1) {
        qn_set_error("%s: need K >= 1 entries (K=%lld)", who, (long long)K);
        return 0;
    }
    if (K > (int64_t(1) << 31)) {
        qn_set_error("%s: shape too large (K=%lld)", who, (long long)K);
        return 0;
    }
    return stack_layout(nullptr, G, K).bytes;
}

__global__ __launch_bounds__(TK) void k_stack_prep(const double* __restrict__ L, int64_t G, int64_t K, double* __restrict__ E,
                                                   double* __restrict__ mk, double* __restrict__ nf, double* __restrict__ status) {
    const int64_t k = (int64_t)blockIdx.x * TK + threadIdx.x;
    if (k == 0) status[QN_STACK_NSTATUS - 1] = 0.0;
    if (k >= K) return;
    const double ninf = -__builtin_inf();
    double m = ninf;
    int bad = 0;
    for (int64_t g = 0; g < G; ++g) {
        const double l = L[g * K + k];
        if (l != l || l == __builtin_inf()) ++bad;
        else m = l > m ? l : m;
    }
    for (int64_t g = 0; g < G; ++g) {
        const double l = L[g * K + k];
        const bool ok = !(l != l || l == __builtin_inf()) && m > ninf;
        E[g * K + k] = ok ? exp(l - m) : 0.0;
    }
    mk[k] = m;
    nf[k] = (double)bad;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(TK) void k_stack_iter(const double* __restrict__ E, const double* __restrict__ mk,
                                                   const double* __restrict__ nf, double* __restrict__ rk, int64_t G, int64_t K,
                                                   int nb, int64_t t, double tol, int64_t max_iter, double* __restrict__ parts,
                                                   double* __restrict__ wbuf, double* __restrict__ w_out, double* __restrict__ status) {
    __shared__ double sw[GMAX];                  // the iterate this launch evaluates
    __shared__ double col[GMAX + XC];            // the previous launch's sums
    __shared__ double tree[GMAX];
    __shared__ double red[TW][GMAX + XC];
    __shared__ int sdone;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, NC = (int)G + XC;
    const int b = blockIdx.x;
    // the flag is set by block 0 of the launch that stops, possibly THIS one: one thread reads it for the block, and a block
    // that still reads 0 in the stopping launch reaches the same decision from the same sums below
    if (tid == 0) sdone = status[QN_STACK_NSTATUS - 1] != 0.0;
    __syncthreads();
    if (sdone) return;
    if (t == 0) {
        for (int g = tid; g < G; g += TK) {
            sw[g] = 1.0 / (double)G;
            if (b == 0) wbuf[g] = sw[g];
        }
    } else {
        const double* prev = parts + (size_t)((t - 1) & 1) * nb * NC;
        const double* wprev = wbuf + ((t - 1) & 1) * G;
        for (int c = tid; c < NC; c += TK) {
            double s = 0.0;
            for (int q = 0; q < nb; ++q) s += prev[(size_t)q * NC + c];
            col[c] = s;
        }
        __syncthreads();
        const double obj = col[G], Kp = col[G + 1], nnf = col[G + 2];
        double gm = 0.0;
        for (int g = tid; g < G; g += TK) {
            const double gr = col[g] / Kp;
            gm = gr > gm ? gr : gm;
        }
        tree[tid] = gm;
        __syncthreads();
        for (int d = TK / 2; d > 0; d >>= 1) {
            if (tid < d) tree[tid] = tree[tid + d] > tree[tid] ? tree[tid + d] : tree[tid];
            __syncthreads();
        }
        const bool empty = Kp == 0.0;
        const double gap = empty ? 0.0 : Kp * (tree[0] - 1.0);
        const bool stop = empty || gap <= tol || t - 1 == max_iter;
        __syncthreads();
        if (b == 0 && tid == 0 && t == 1) status[6] = empty ? 0.0 : obj;                    // iterate 0: obj at w = 1 / G
        if (stop) {
            if (b == 0) {
                for (int g = tid; g < G; g += TK) w_out[g] = empty ? 1.0 / (double)G : wprev[g];
                if (tid == 0) {
                    status[0] = empty ? 0.0 : obj;
                    status[1] = gap;
                    status[2] = (double)(t - 1);
                    status[3] = Kp;
                    status[4] = nnf;
                    status[5] = (double)K - Kp;
                    status[QN_STACK_NSTATUS - 1] = 1.0;
                }
            }
            return;
        }
        for (int g = tid; g < GMAX; g += TK) {
            const double u = g < G ? wprev[g] * (col[g] / Kp) : 0.0;
            sw[g] = u;
            tree[g] = u;
        }
        __syncthreads();
        for (int d = GMAX / 2; d > 0; d >>= 1) {
            for (int g = tid; g < d; g += TK) tree[g] += tree[g + d];
            __syncthreads();
        }
        const double tot = tree[0];
        for (int g = tid; g < G; g += TK) {
            sw[g] = sw[g] / tot;
            if (b == 0) wbuf[(t & 1) * G + g] = sw[g];
        }
    }
    __syncthreads();
    // ---- this block's entries: mix_k, r_k = 1 / mix_k, the obj and count columns
    const int64_t ntiles = (K + TK - 1) / TK;
    double r0 = 0.0, objp = 0.0, keepp = 0.0, nfp = 0.0;
    for (int64_t j = b; j < ntiles; j += nb) {
        const int64_t k = j * TK + tid;
        double r = 0.0;
        if (k < K) {
            nfp += nf[k];
            const double m = mk[k];
            if (m > -__builtin_inf()) {
                double mix = 0.0;
                for (int g = 0; g < G; ++g) mix += sw[g] * E[(size_t)g * K + k];
                r = 1.0 / mix;
                objp += log(mix) + m;
                keepp += 1.0;
            }
            if (j != b) rk[k] = r;               // read back by this thread alone
        }
        if (j == b) r0 = r;
    }
    const int64_t kf = (int64_t)b * TK + tid;
    for (int g = 0; g < G; ++g) {
        const double* e = E + (size_t)g * K;
        double s = kf < K ? e[kf] * r0 : 0.0;
        for (int64_t j = b + nb; j < ntiles; j += nb) {
            const int64_t k = j * TK + tid;
            if (k < K) s += e[k] * rk[k];
        }
        s = wave_sum(s);
        if (lane == 0) red[wv][g] = s;
    }
    objp = wave_sum(objp);
    keepp = wave_sum(keepp);
    nfp = wave_sum(nfp);
    if (lane == 0) {
        red[wv][G] = objp;
        red[wv][G + 1] = keepp;
        red[wv][G + 2] = nfp;
    }
    __syncthreads();
    double* mine = parts + ((size_t)(t & 1) * nb + b) * NC;
    for (int c = tid; c < NC; c += TK) {
        double s = red[0][c];
#pragma unroll
        for (int q = 1; q < TW; ++q) s += red[q][c];
        mine[c] = s;
    }
}

// ---------------------------------------------------------------------------------------------------- qn_pred_score_w
template <typename T, bool HASV>
__global__ __launch_bounds__(SBLK) void k_scorew_stream(const T* __restrict__ F, const T* __restrict__ V,
                                                        const double* __restrict__ Y, const double* __restrict__ wm, int64_t M,
                                                        int64_t K, double sig2, double sig2_lo, int what, double* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * SBLK + threadIdx.x;
    if (k >= K) return;
    const bool want_ll = what & (QN_SCORE_LPPD | QN_SCORE_PWAIC), want_pit = what & QN_SCORE_PIT;
    const bool want_crps = what & QN_SCORE_CRPS;
    const double y = Y ? Y[k] : 0.0;
    const double sd0 = sqrt(sig2), inv_sd0 = 1.0 / sd0;
    const LogNorm norm0 = log_norm(sig2, sig2_lo);
    bool bad = !isfinite(y), zero_s = false, badw = false, first = true;
    double lmax = 0.0, lsum = 0.0, lmean = 0.0, lm2 = 0.0, fmean = 0.0, fm2 = 0.0, pit = 0.0, c1 = 0.0;
    double wtot = 0.0, sw2 = 0.0;
    const T* f_col = F + k;
    const T* v_col = HASV ? V + k : nullptr;
    auto member = [&](double w, double f, double v) {
        if (!(w >= 0.0) || !isfinite(w)) badw = true;
        if (!(w > 0.0)) return;                                 // weight 0 (the same in every lane): f and v play no part
        double s2e;
        const double s2 = two_sum(sig2, v, &s2e), r = y - f;
        bad = bad || !isfinite(f) || !isfinite(v) || !(s2 >= 0.0);
        double sd = sd0, inv_sd = inv_sd0;
        if (HASV) {
            sd = sqrt(s2);
            inv_sd = 1.0 / sd;
            zero_s = zero_s || s2 == 0.0;
        }
        const bool pos = s2 > 0.0;
        wtot += w;
        sw2 += w * w;
        const double share = w / wtot;
        if (want_ll) {
            const double ll = log_lik(y, f, HASV ? log_norm(s2, s2e + sig2_lo) : norm0);
            if (first) {
                lmax = ll;
                lsum = w;
            } else if (ll > lmax) {
                lsum = lsum * exp(lmax - ll) + w;
                lmax = ll;
            } else {
                lsum += w * exp(ll - lmax);
            }
            const double d = ll - lmean;
            lmean += share * d;
            lm2 += w * d * (ll - lmean);
        }
        {
            const double d = f - fmean;
            fmean += share * d;
            fm2 += w * d * (f - fmean);
        }
        if (want_pit) pit += w * (pos ? 0.5 * erfc(-(r * inv_sd) * M_SQRT1_2) : (r > 0.0 ? 1.0 : (r == 0.0 ? 0.5 : 0.0)));
        if (want_crps) c1 += w * (pos ? crps_a(r, sd, inv_sd) : fabs(r));
        first = false;
    };
    int64_t m = 0;
    for (; m + SUNROLL <= M; m += SUNROLL) {
        double w[SUNROLL], f[SUNROLL], v[SUNROLL];
#pragma unroll
        for (int j = 0; j < SUNROLL; ++j) {
            w[j] = wm[m + j];
            f[j] = (double)f_col[(m + j) * K];
            v[j] = HASV ? (double)v_col[(m + j) * K] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < SUNROLL; ++j) member(w[j], f[j], v[j]);
    }
    for (; m < M; ++m) member(wm[m], (double)f_col[m * K], HASV ? (double)v_col[m * K] : 0.0);
    const double nan = __builtin_nan(""), den = 1.0 - sw2;
    if (first) badw = true;                                     // no member carries weight
    bad = bad || badw;
    if (what & QN_SCORE_LPPD) out[k] = (bad || zero_s) ? nan : lmax + log(lsum);
    if (what & QN_SCORE_PWAIC) out[K + k] = (bad || zero_s) ? nan : (den == 0.0 ? 0.0 : lm2 / den);
    if (want_pit) out[2 * K + k] = bad ? nan : pit;
    if (want_crps) out[3 * K + k] = bad ? nan : c1;
    if (what & QN_SCORE_MOMENTS) {
        out[4 * K + k] = bad ? nan : fmean;
        out[5 * K + k] = bad ? nan : (den == 0.0 ? 0.0 : fm2 / den);
    }
}

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

// sum_i sum_{j < i} wm_i wm_j A(f_i - f_j, s_i^2 + s_j^2), tiled as k_score_pairs of qn_score.hip; parts [i-block, K] gets
// 2 * (that sum) + sum_i wm_i^2 A(0, 2 s_i^2).  A pair with a weight of 0 is selected away, never multiplied.
template <typename T, int MODE>
__global__ __launch_bounds__(PT * PW) void k_scorew_pairs(const T* __restrict__ F, const T* __restrict__ V,
                                                          const double* __restrict__ wm, int64_t M, int64_t K, double sig2,
                                                          double* __restrict__ parts) {
    __shared__ double sf[PJC][PT];
    __shared__ double sv[MODE == 2 ? PJC : 1][PT];
    __shared__ double red[PW][PT];
    const int lane = threadIdx.x & (PT - 1), w = threadIdx.x / PT;
    const int64_t k = (int64_t)blockIdx.x * PT + lane;
    const int64_t kc = k < K ? k : K - 1;
    const int64_t ib = blockIdx.y, i0 = ib * PIB + (int64_t)w * PR;
    const double sdc = sqrt(2.0 * sig2), inv_sdc = 1.0 / sdc;
    double fi[PR], vi[PR], wi[PR], acc[PR];
#pragma unroll
    for (int r = 0; r < PR; ++r) {
        const int64_t ic = i0 + r < M ? i0 + r : M - 1;
        wi[r] = i0 + r < M ? wm[ic] : 0.0;
        const bool on = wi[r] != 0.0;
        fi[r] = on ? (double)F[ic * K + kc] : 0.0;
        vi[r] = MODE == 2 ? (on ? sig2 + (double)V[ic * K + kc] : 1.0) : sig2;
        acc[r] = 0.0;
    }
    const int64_t jend = (ib + 1) * PIB < M ? (ib + 1) * PIB : M;
    for (int64_t j0 = 0; j0 < jend; j0 += PJC) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PJC / PW; ++q) {
            const int row = w + PW * q;
            if (j0 + row < jend && wm[j0 + row] != 0.0) {
                sf[row][lane] = (double)F[(j0 + row) * K + kc];
                if (MODE == 2) sv[row][lane] = sig2 + (double)V[(j0 + row) * K + kc];
            }
        }
        __syncthreads();
        const int jn = jend - j0 < PJC ? (int)(jend - j0) : PJC;
        if (j0 + PJC <= ib * PIB) {                             // below the diagonal chunk: j < i for every i of the block
            for (int jj = 0; jj < jn; ++jj) {
                const double wj = wm[j0 + jj];
                if (wj == 0.0) continue;                        // wave-uniform
                const double fj = sf[jj][lane], vj = MODE == 2 ? sv[jj][lane] : sig2;
#pragma unroll
                for (int r = 0; r < PR; ++r)
                    if (wi[r] != 0.0) acc[r] += wi[r] * wj * pair_a<MODE>(fi[r] - fj, vi[r] + vj, sdc, inv_sdc);
            }
        } else {
            for (int jj = 0; jj < jn && j0 + jj < i0 + PR - 1; ++jj) {
                const int64_t j = j0 + jj;
                const double wj = wm[j];
                if (wj == 0.0) continue;
                const double fj = sf[jj][lane], vj = MODE == 2 ? sv[jj][lane] : sig2;
#pragma unroll
                for (int r = 0; r < PR; ++r)
                    if (j < i0 + r && wi[r] != 0.0) acc[r] += wi[r] * wj * pair_a<MODE>(fi[r] - fj, vi[r] + vj, sdc, inv_sdc);
            }
        }
    }
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < PR; ++r)
        if (wi[r] != 0.0) t += 2.0 * acc[r] + wi[r] * wi[r] * pair_a<MODE>(0.0, vi[r] + vi[r], sdc, inv_sdc);
    red[w][lane] = t;
    __syncthreads();
    if (w == 0 && k < K) {
        double p = red[0][lane];
#pragma unroll
        for (int q = 1; q < PW; ++q) p += red[q][lane];
        parts[ib * K + k] = p;
    }
}

__global__ __launch_bounds__(256) void k_scorew_finish(const double* __restrict__ parts, int64_t nib, int64_t K,
                                                       double* __restrict__ crps) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int64_t b = 0; b < nib; ++b) s += parts[b * K + k];
    crps[k] -= 0.5 * s;
}

size_t scorew_workspace(const char* who, int64_t M, int64_t K, int what) {
    if (M < 1 || K < 1) {
        qn_set_error("%s: need M >= 1 members and K >= 1 entries (M=%lld K=%lld)", who, (long long)M, (long long)K);
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
void launch_lpd(const T* F, const T* V, const double* Y, int64_t K, double sigma, const int64_t* off, int64_t G, double* L,
                hipStream_t st) {
    const double sig2 = sigma * sigma, sig2_lo = std::fma(sigma, sigma, -sig2);
    const dim3 grid((unsigned)((K + SBLK - 1) / SBLK));
    if (V) hipLaunchKernelGGL((k_group_lpd<T, true>), grid, dim3(SBLK), 0, st, F, V, Y, K, sig2, sig2_lo, off, G, L);
    else hipLaunchKernelGGL((k_group_lpd<T, false>), grid, dim3(SBLK), 0, st, F, V, Y, K, sig2, sig2_lo, off, G, L);
}

template <typename T>
void launch_scorew(const T* F, const T* V, const double* Y, const double* wm, int64_t M, int64_t K, double sigma, int what,
                   double* out, double* parts, hipStream_t st) {
    const double sig2 = sigma * sigma, sig2_lo = std::fma(sigma, sigma, -sig2);
    const dim3 sgrid((unsigned)((K + SBLK - 1) / SBLK));
    if (V) hipLaunchKernelGGL((k_scorew_stream<T, true>), sgrid, dim3(SBLK), 0, st, F, V, Y, wm, M, K, sig2, sig2_lo, what, out);
    else hipLaunchKernelGGL((k_scorew_stream<T, false>), sgrid, dim3(SBLK), 0, st, F, V, Y, wm, M, K, sig2, sig2_lo, what, out);
    if (!(what & QN_SCORE_CRPS)) return;
    const int64_t nib = (M + PIB - 1) / PIB;
    const dim3 pgrid((unsigned)((K + PT - 1) / PT), (unsigned)nib);
    if (V) hipLaunchKernelGGL((k_scorew_pairs<T, 2>), pgrid, dim3(PT * PW), 0, st, F, V, wm, M, K, sig2, parts);
    else if (sigma > 0.0) hipLaunchKernelGGL((k_scorew_pairs<T, 1>), pgrid, dim3(PT * PW), 0, st, F, V, wm, M, K, sig2, parts);
    else hipLaunchKernelGGL((k_scorew_pairs<T, 0>), pgrid, dim3(PT * PW), 0, st, F, V, wm, M, K, sig2, parts);
    hipLaunchKernelGGL(k_scorew_finish, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, parts, nib, K, out + 3 * K);
}

}  // namespace

extern "C" size_t qn_group_lpd_workspace_bytes(int64_t M, int64_t K, int64_t G) {
    return lpd_workspace("qn_group_lpd_workspace_bytes", M, K, G);
}

extern "C" int qn_group_lpd(const void* F, const void* V, int dtype, const double* Y, int64_t M, int64_t K, double sigma,
                            const int64_t* offsets, int64_t G, double* L, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = lpd_workspace("qn_group_lpd", M, K, G);
    if (need == 0 || !score_args_ok("qn_group_lpd", dtype, sigma, true, V != nullptr)) return QN_EINVAL;
    if (!F || !Y || !offsets || !L || !workspace) {
        qn_set_error("qn_group_lpd: F, Y, offsets, L and workspace must not be NULL");
        return QN_EINVAL;
    }
    if (workspace_bytes < need) {
        qn_set_error("qn_group_lpd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return QN_EWORKSPACE;
    }
    bool rising = offsets[0] == 0 && offsets[G] == M;
    for (int64_t g = 0; g < G && rising; ++g) rising = offsets[g + 1] > offsets[g];
    if (!rising) {
        qn_set_error("qn_group_lpd: offsets must rise strictly from 0 to M = %lld", (long long)M);
        return QN_EINVAL;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    int64_t* off = static_cast<int64_t*>(workspace);
    QN_HIP_CHECK(hipMemcpyAsync(off, offsets, (size_t)(G + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (dtype == QN_F32) launch_lpd(static_cast<const float*>(F), static_cast<const float*>(V), Y, K, sigma, off, G, L, st);
    else launch_lpd(static_cast<const double*>(F), static_cast<const double*>(V), Y, K, sigma, off, G, L, st);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}

extern "C" size_t qn_stack_weights_workspace_bytes(int64_t G, int64_t K) {
    return stack_workspace("qn_stack_weights_workspace_bytes", G, K);
}

extern "C" int qn_stack_weights(const double* L, int64_t G, int64_t K, double tol, int64_t max_iter, int64_t t0, int64_t nlaunch,
                                double* w, double* status, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = stack_workspace("qn_stack_weights", G, K);
    if (need == 0) return QN_EINVAL;
    if (!(tol >= 0.0) || !std::isfinite(tol) || max_iter < 0 || t0 < 0 || nlaunch < 1) {
        qn_set_error("qn_stack_weights: need tol >= 0 and finite, max_iter >= 0, t0 >= 0, nlaunch >= 1 (tol=%g max_iter=%lld t0=%lld "
                     "nlaunch=%lld)", tol, (long long)max_iter, (long long)t0, (long long)nlaunch);
        return QN_EINVAL;
    }
    if (!L || !w || !status || !workspace) {
        qn_set_error("qn_stack_weights: L, w, status and workspace must not be NULL");
        return QN_EINVAL;
    }
    if (workspace_bytes < need) {
        qn_set_error("qn_stack_weights: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return QN_EWORKSPACE;
    }
    const StackWs s = stack_layout(workspace, G, K);
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (t0 == 0)
        hipLaunchKernelGGL(k_stack_prep, dim3((unsigned)((K + TK - 1) / TK)), dim3(TK), 0, st, L, G, K, s.E, s.mk, s.nf, status);
    for (int64_t t = t0; t < t0 + nlaunch; ++t)
        hipLaunchKernelGGL(k_stack_iter, dim3((unsigned)s.nb), dim3(TK), 0, st, s.E, s.mk, s.nf, s.rk, G, K, s.nb, t, tol, max_iter,
                           s.parts, s.wbuf, w, status);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}

extern "C" size_t qn_pred_score_w_workspace_bytes(int64_t M, int64_t K, int what) {
    return scorew_workspace("qn_pred_score_w_workspace_bytes", M, K, what);
}

extern "C" int qn_pred_score_w(const void* F, const void* V, int dtype, const double* Y, const double* wm, int64_t M, int64_t K,
                               double sigma, int what, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = scorew_workspace("qn_pred_score_w", M, K, what);
    if (need == 0) return QN_EINVAL;
    if (!score_args_ok("qn_pred_score_w", dtype, sigma, what & (QN_SCORE_LPPD | QN_SCORE_PWAIC | QN_SCORE_PIT), V != nullptr))
        return QN_EINVAL;
    if (!F || !wm || !out || (!Y && what != QN_SCORE_MOMENTS) || ((what & QN_SCORE_CRPS) && !workspace)) {
        qn_set_error("qn_pred_score_w: F, wm, out, Y (unless what is QN_SCORE_MOMENTS) and (for the CRPS) workspace must not be NULL");
        return QN_EINVAL;
    }
    if (workspace_bytes < need) {
        qn_set_error("qn_pred_score_w: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return QN_EWORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (dtype == QN_F32)
        launch_scorew(static_cast<const float*>(F), static_cast<const float*>(V), Y, wm, M, K, sigma, what, out,
                      static_cast<double*>(workspace), st);
    else
        launch_scorew(static_cast<const double*>(F), static_cast<const double*>(V), Y, wm, M, K, sigma, what, out,
                      static_cast<double*>(workspace), st);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
