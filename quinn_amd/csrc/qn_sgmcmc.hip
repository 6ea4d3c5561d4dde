// Stochastic-gradient MCMC on the device (SGLD, Welling & Teh 2011; SGHMC, Chen et al. 2014; cyclical step size, Zhang et al.
// 2020) around the batched gradient kernel evaluated on each chain's OWN minibatch:
//   qn_sg_rows : rows[c, j] of an inner step, drawn uniformly with replacement -- pure integer arithmetic on Philox words
//   qn_sg_step : v <- (1 - alpha) v - eta g + on sqrt(2 alpha eta T) z;  theta <- theta + v;  log-posterior trace of the
//                incoming state, history row of the outgoing one, the NEXT step's rows, the device step counter
// A step is qn_mlp_sse_fwdbwd + qn_sg_step and nothing else.  The step kernel is elementwise over [C, p] and HBM-bound: per
// element it reads theta, v, g and writes theta, v (40 B; SGLD, alpha = 1: no v, 24 B), plus 8 B on the steps whose state is
// stored.  Same geometry as the HMC elementwise kernels (hmc_parts(p) workgroups of HBLK threads per chain), pairs of elements
// per 16-byte access and per Philox block as in k_accept.  The per-chain scalars (inner step, SSE, best log-posterior) are
// read by every workgroup of a chain from the slot of the step's parity and written by workgroup 0 to the other slot: no
// fence, atomic or arrival counter.
#include "qn_mcmc_shared.h"

namespace {

// Philox purposes of this file (qn_mcmc_shared.h lists 0-3): 4 minibatch rows (index = entry / 4), 5 step noise (index =
// element pair).  The stream is the inner step itself.
constexpr int PURPOSE_ROWS = 4;
constexpr int PURPOSE_NOISE = 5;
constexpr int SPT = HUB / 2;              // pairs per thread and pass

// entries 4 q .. 4 q + 3 of chain `chain`'s rows at inner step t: word w of one Philox block scaled to [0, N)
__device__ __forceinline__ void rows_quad(int32_t* __restrict__ row, int q, int Nb, int N, int chain, uint64_t seed, uint64_t t,
                                          bool vec) {
    Philox ph;
    ph.gen(seed, t, ctr_of(chain, PURPOSE_ROWS, (uint64_t)q));
    const int j = 4 * q;
    const int32_t r0 = (int32_t)__umulhi(ph.c[0], (uint32_t)N), r1 = (int32_t)__umulhi(ph.c[1], (uint32_t)N),
                  r2 = (int32_t)__umulhi(ph.c[2], (uint32_t)N), r3 = (int32_t)__umulhi(ph.c[3], (uint32_t)N);
    if (vec) {                             // Nb % 4 == 0 and a 16-byte aligned buffer: every quad is whole and aligned
        *reinterpret_cast<int4*>(row + j) = make_int4(r0, r1, r2, r3);
    } else {
        row[j] = r0;
        if (j + 1 < Nb) row[j + 1] = r1;
        if (j + 2 < Nb) row[j + 2] = r2;
        if (j + 3 < Nb) row[j + 3] = r3;
    }
}

__global__ __launch_bounds__(HBLK) void k_sg_rows(int32_t* __restrict__ rows, int Nb, int N, int chain0, uint64_t seed,
                                                  const int64_t* __restrict__ step_ptr, int64_t step_off, int vec) {
    const int b = blockIdx.y;
    const uint64_t t = (uint64_t)((step_ptr ? *step_ptr : 0) + step_off);
    const int nquad = (Nb + 3) / 4;
    int32_t* row = rows + (int64_t)b * Nb;
    for (int q = blockIdx.x * HBLK + threadIdx.x; q < nquad; q += gridDim.x * HBLK)
        rows_quad(row, q, Nb, N, chain0 + b, seed, t, vec != 0);
}

template <typename TG> struct Pair;
template <> struct Pair<double> { typedef d2u type; };
template <> struct Pair<float> { typedef f2u type; };
template <typename TG>
__device__ __forceinline__ d2u ldg2(const TG* p, bool both) {
    d2u v;
    if (both) {
        const typename Pair<TG>::type w = *reinterpret_cast<const typename Pair<TG>::type*>(p);
        v.x = (double)w.x; v.y = (double)w.y;
    } else {
        v.x = (double)p[0]; v.y = 0.0;
    }
    return v;
}

struct SgArgs {
    double gscale;                        // (N / Nb) / (2 sigma^2): SSE of the minibatch -> full-data potential
    double lp_const;                      // (N / 2) log 2 pi + N log sigma
    double eta0, alpha, temperature, explore_frac;
    int64_t K;                            // inner steps per cycle; 0: constant step size, noise always on
    int thin, fin, par, C, chain0, nstore, Nb, N, rows_vec;
    int64_t p;
    uint64_t seed;
};

template <typename TG>
__global__ __launch_bounds__(HBLK) void k_sg_step(SgArgs a, double* __restrict__ theta, double* __restrict__ v,
                                                  const TG* __restrict__ grad, const double* __restrict__ sse,
                                                  float* __restrict__ theta32, double* __restrict__ best,
                                                  double* __restrict__ best_lp, double* __restrict__ chain,
                                                  double* __restrict__ lps, int32_t* __restrict__ rows,
                                                  int64_t* __restrict__ step_ptr) {
    const int b = blockIdx.y, part = blockIdx.x;
    const int so = a.par * a.C + b, sn = (1 - a.par) * a.C + b;
    const int64_t base = (int64_t)b * a.p;
    const int64_t npair = (a.p + 1) / 2;
    const bool move = !a.fin, mom = move && a.alpha != 1.0;
    d2u tv[SPT], vv[SPT], gv[SPT];
    auto load = [&](int64_t pair0) {
#pragma unroll
        for (int h = 0; h < SPT; ++h) {
            const int64_t pair = pair0 + (int64_t)h * HBLK, e = 2 * pair;
            const bool in = pair < npair, both = e + 1 < a.p;
            const d2u zero = {0.0, 0.0};
            tv[h] = in ? ld2(theta + base + e, both) : zero;
            vv[h] = (in && mom) ? ld2(v + base + e, both) : zero;
            gv[h] = (in && move) ? ldg2<TG>(grad + base + e, both) : zero;
        }
    };
    // ---- issue the thread's first pairs, then the chain's scalars: one round trip before the first use
    int64_t pair0 = (int64_t)part * (SPT * HBLK) + threadIdx.x;
    load(pair0);
    const int64_t t = step_ptr[a.par];
    const double sse_c = sse[b];
    const double blp = best_lp[so];
    // ---- the step's scalars (every workgroup of every chain forms the same numbers)
    const int64_t r = a.K > 0 ? t % a.K : 0;
    const double eta = a.K > 0 ? 0.5 * a.eta0 * (cos(M_PI * (double)r / (double)a.K) + 1.0) : a.eta0;
    const bool on = a.K > 0 ? (double)r / (double)a.K >= a.explore_frac : true;
    const double ns = (on && move) ? sqrt(2.0 * a.alpha * eta * a.temperature) : 0.0;
    const double keep = 1.0 - a.alpha;
    // log-posterior estimate of the INCOMING state theta_t, on the stored steps
    const bool trace = t % a.thin == 0 && t / a.thin <= a.nstore;
    const double lp = -(a.gscale * sse_c + a.lp_const);
    const bool better = trace && lp >= blp;                         // (NaN: never)
    const int64_t rown = (t + 1) / a.thin;
    double* crow = (move && chain && (t + 1) % a.thin == 0 && rown <= a.nstore)
                       ? chain + ((int64_t)b * (a.nstore + 1) + rown) * a.p : nullptr;
    const int64_t stride = (int64_t)gridDim.x * (SPT * HBLK);
    while (pair0 < npair) {
#pragma unroll
        for (int h = 0; h < SPT; ++h) {
            const int64_t pair = pair0 + (int64_t)h * HBLK, e = 2 * pair;
            if (pair >= npair) break;
            const bool both = e + 1 < a.p;
            if (better) st2(best + base + e, tv[h].x, tv[h].y, both);
            if (!move) continue;
            double za = 0.0, zb = 0.0;
            if (ns != 0.0) {
                Philox ph;
                ph.gen(a.seed, (uint64_t)t, ctr_of(a.chain0 + b, PURPOSE_NOISE, (uint64_t)pair));
                normal2(ph, za, zb);
            }
            // same association as sgmcmc.sg_step: (1 - alpha) v + (-eta g + noise)
            double v0 = -eta * (a.gscale * gv[h].x) + ns * za, v1 = -eta * (a.gscale * gv[h].y) + ns * zb;
            if (mom) { v0 = keep * vv[h].x + v0; v1 = keep * vv[h].y + v1; }
            const double x0 = tv[h].x + v0, x1 = tv[h].y + v1;
            st2(theta + base + e, x0, x1, both);
            if (mom) st2(v + base + e, v0, v1, both);
            if (crow) st2(crow + e, x0, x1, both);
            if (theta32) {                                          // float32 operator: the positions its next call reads
                if (both) { f2u w; w.x = (float)x0; w.y = (float)x1; *reinterpret_cast<f2u*>(theta32 + base + e) = w; }
                else theta32[base + e] = (float)x0;
            }
        }
        pair0 += stride;
        if (pair0 < npair) load(pair0);
    }
    // ---- rows of step t + 1 into the other half of rows [2, C, Nb]
    if (move && rows) {
        int32_t* row = rows + ((int64_t)(1 - a.par) * a.C + b) * a.Nb;
        const int nquad = (a.Nb + 3) / 4;
        for (int q = part * HBLK + threadIdx.x; q < nquad; q += gridDim.x * HBLK)
            rows_quad(row, q, a.Nb, a.N, a.chain0 + b, a.seed, (uint64_t)(t + 1), a.rows_vec != 0);
    }
    if (part == 0 && threadIdx.x == 0) {
        if (trace) lps[(int64_t)b * (a.nstore + 1) + t / a.thin] = lp;
        best_lp[sn] = better ? lp : blp;
        if (b == 0) step_ptr[1 - a.par] = move ? t + 1 : t;
    }
}

}  // namespace

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int qn_sg_rows(int32_t* rows, int C, int Nb, int N, int chain0, uint64_t seed, const int64_t* step_ptr,
                          int64_t step_off, void* stream) {
    if (!rows || C <= 0 || C > 65535 || Nb <= 0 || N <= 0 || chain0 < 0 || step_off < 0) {
        qn_set_error("qn_sg_rows: bad argument");
        return QN_EINVAL;
    }
    int gx = ((Nb + 3) / 4 + HBLK - 1) / HBLK;
    if (gx > 64) gx = 64;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_sg_rows, dim3(gx, C), dim3(HBLK), 0, static_cast<hipStream_t>(stream), rows, Nb, N, chain0, seed,
                       step_ptr, step_off, (Nb % 4 == 0 && aligned16(rows)) ? 1 : 0);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}

extern "C" int qn_sg_step(double* theta, double* v, const void* grad, int dtype, const double* sse, double sigma, int n_rows,
                          int n_batch, double eta0, double alpha, double temperature, int schedule, int64_t cycle_len,
                          double explore_frac, int thin, int final, int C, int chain0, int64_t p, int nstore, uint64_t seed,
                          void* theta_op, double* best, double* best_lp, double* chain, double* lps, int32_t* rows,
                          int64_t* step_ptr, int parity, void* stream) {
    const bool cyclic = schedule == 1;
    if (!theta || !grad || !sse || !best || !best_lp || !lps || !step_ptr || (alpha != 1.0 && !v) || C <= 0 || C > 65535 ||
        chain0 < 0 || p <= 0 || nstore < 0 || thin < 1 || n_rows <= 0 || n_batch <= 0 || !(sigma > 0.0) || !(eta0 > 0.0) ||
        !(alpha > 0.0 && alpha <= 1.0) || !(temperature >= 0.0) || (schedule != 0 && schedule != 1) ||
        (cyclic && (cycle_len < 2 || !(explore_frac >= 0.0 && explore_frac <= 1.0))) || (parity != 0 && parity != 1) ||
        (dtype != QN_F64 && dtype != QN_F32) || (theta_op && dtype != QN_F32)) {
        qn_set_error("qn_sg_step: bad argument");
        return QN_EINVAL;
    }
    SgArgs a;
    a.gscale = ((double)n_rows / (double)n_batch) * (0.5 / (sigma * sigma));
    a.lp_const = 0.5 * n_rows * std::log(2.0 * M_PI) + n_rows * std::log(sigma);
    a.eta0 = eta0; a.alpha = alpha; a.temperature = temperature; a.explore_frac = explore_frac;
    a.K = cyclic ? cycle_len : 0;
    a.thin = thin; a.fin = final ? 1 : 0; a.par = parity; a.C = C; a.chain0 = chain0; a.nstore = nstore; a.Nb = n_batch;
    a.N = n_rows; a.rows_vec = (rows && n_batch % 4 == 0 && aligned16(rows) && ((int64_t)C * n_batch) % 4 == 0) ? 1 : 0;
    a.p = p; a.seed = seed;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(hmc_parts(p), C), blk(HBLK);
    (void)hipGetLastError();
    if (dtype == QN_F32)
        hipLaunchKernelGGL(k_sg_step<float>, grid, blk, 0, st, a, theta, v, (const float*)grad, sse, (float*)theta_op, best,
                           best_lp, chain, lps, rows, step_ptr);
    else
        hipLaunchKernelGGL(k_sg_step<double>, grid, blk, 0, st, a, theta, v, (const double*)grad, sse, (float*)nullptr, best,
                           best_lp, chain, lps, rows, step_ptr);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
