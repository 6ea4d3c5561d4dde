// Elliptical slice sampling on the device (Murray, Adams & MacKay 2010; build-only, the reference has no such sampler) with
// ASYNCHRONOUS chain steps: every chain keeps its own step counter t and shrink count j, and one qn_ess_iter launch either
// shrinks a chain's bracket or, its pending proposal accepted, starts the chain's next step right away -- so every forward
// evaluation between two launches is one some chain needs.  quinn_amd/mcmc/ess.py states the rule and restates it in numpy.
//   qn_ess_begin : start of step 0 of every chain (nu = s z, theta, logy, bracket, prop = cur cos theta + nu sin theta)
//   qn_ess_iter  : one iteration on the SSE parts of the pending proposals
// Geometry of the HMC elementwise kernels: hmc_parts(p) workgroups of HBLK threads per chain, a pair of elements per 16-byte
// access and per Philox block.  Every workgroup of a chain reads the chain's scalars (es, ei, best_lp, sq_parts: slot
// `parity`) and the SSE parts and comes to the same decision; workgroup 0 alone writes the scalars, to slot 1 - parity, and
// every workgroup its own partial sum of squares of the proposal it wrote: no workgroup sees a half-updated chain, no atomics,
// no fences, equal inputs give equal bits.  An element is read and written by one thread only, so cur / nu / prop are updated
// in place.  HBM-bound: an accepting chain moves 5 x 8 B per element (read prop; write cur, chain row, nu, prop), a shrinking
// chain 3 x 8 B (read cur, nu; write prop), a done chain nothing.  FP contraction is off for the whole file: the scalars and
// the ellipse are formed with one rounding per operation, as the numpy restatement forms them.
#include "qn_mcmc_shared.h"

#pragma clang fp contract(off)

namespace {

// Philox purposes of this file (qn_mcmc_shared.h lists them all): 7 the ellipse partner (index = column pair), 8 the angle
// uniforms (index 0: start of the step, index j + 1: shrink j + 1).  The stream is the chain's own step t.
constexpr int PURPOSE_NU = 7;
constexpr int PURPOSE_ANGLE = 8;
constexpr double TWO_PI = 2.0 * M_PI;
constexpr int NES = 6;                    // es: theta, tmin, tmax, logy, sse_cur, lp_cur
constexpr int NEI = 4;                    // ei: t, j, ntrunc, nevals

struct EssArgs {
    double gs;                            // -0.5 / sigma^2
    double lik_const;                     // (N / 2) log 2 pi + N log sigma
    double s;                             // priorsigma
    double pscale;                        // -0.5 / s^2
    double prior_const;                   // (p / 2) log(2 pi s^2)
    int C, chain0, nmcmc, max_shrink, nparts, par;
    int64_t p;
    uint64_t seed;
};

struct Pass {                             // the arrays of one elementwise pass over a chain's row (offsets applied)
    const double* x;                      // the point the pass starts from: cur, or the accepted prop
    double *to_cur, *to_row, *to_best;    // copies of x (NULL: none)
    double *nu, *prop;
    float* prop_op;
};

// The pairs [lo, hi) of one row: x is copied where asked; with `ell`, prop = x cs + nu sn, where nu = s z is drawn for step t
// and stored (draw) or read.  Returns the thread's sum of squares of the prop elements it wrote.
__device__ __forceinline__ double ellipse_pass(const EssArgs& a, const Pass& q, int chain, int64_t lo, int64_t hi, bool ell,
                                               bool draw, uint64_t t, double cs, double sn) {
    double ss = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += HBLK) {
        const int64_t e = 2 * j;
        const bool both = e + 1 < a.p;
        const d2u xv = ld2(q.x + e, both);
        if (q.to_cur) st2(q.to_cur + e, xv.x, xv.y, both);
        if (q.to_row) st2(q.to_row + e, xv.x, xv.y, both);
        if (q.to_best) st2(q.to_best + e, xv.x, xv.y, both);
        if (!ell) continue;
        double n0, n1;
        if (draw) {
            Philox ph;
            ph.gen(a.seed, t, ctr_of(chain, PURPOSE_NU, (uint64_t)j));
            normal2(ph, n0, n1);
            n0 = a.s * n0;
            n1 = a.s * n1;
            st2(q.nu + e, n0, n1, both);
        } else {
            const d2u nv = ld2(q.nu + e, both);
            n0 = nv.x;
            n1 = nv.y;
        }
        const double p0 = xv.x * cs + n0 * sn, p1 = xv.y * cs + n1 * sn;
        st2(q.prop + e, p0, p1, both);
        if (q.prop_op) {                                            // float32 operator: what its next forward reads
            if (both) { f2u w; w.x = (float)p0; w.y = (float)p1; *reinterpret_cast<f2u*>(q.prop_op + e) = w; }
            else q.prop_op[e] = (float)p0;
        }
        ss = ss + p0 * p0;
        if (both) ss = ss + p1 * p1;
    }
    return ss;
}

// Start of step t of a chain from the point q.x with SSE sse_cur: the angle and the slice level from the block (seed, t,
// ctr_of(chain, 8, 0)), then the pass that draws nu and writes the first proposal.  Shared by both kernels.
__device__ __forceinline__ double start_step(const EssArgs& a, const Pass& q, int chain, int64_t lo, int64_t hi, uint64_t t,
                                             double sse_cur, double& theta, double& logy) {
    Philox ph;
    ph.gen(a.seed, t, ctr_of(chain, PURPOSE_ANGLE, 0));
    theta = TWO_PI * u01(ph.c[0], ph.c[1]);
    logy = a.gs * sse_cur + log(u01(ph.c[2], ph.c[3]));
    double sn, cs;
    sincos(theta, &sn, &cs);
    return ellipse_pass(a, q, chain, lo, hi, true, true, t, cs, sn);
}

__device__ __forceinline__ void pair_range(int64_t p, int64_t& lo, int64_t& hi) {
    const int64_t npair = (p + 1) / 2;
    const int64_t pchunk = (npair + gridDim.x - 1) / gridDim.x;
    lo = blockIdx.x * pchunk;
    hi = lo + pchunk < npair ? lo + pchunk : npair;
}

__global__ __launch_bounds__(HBLK) void k_ess_begin(EssArgs a, const double* __restrict__ cur, const double* __restrict__ sse_cur,
                                                    const double* __restrict__ lp_cur, double* __restrict__ nu,
                                                    double* __restrict__ prop, float* __restrict__ prop_op,
                                                    double* __restrict__ sq_parts, double* __restrict__ es,
                                                    int64_t* __restrict__ ei) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const int64_t base = (int64_t)b * a.p;
    int64_t lo, hi;
    pair_range(a.p, lo, hi);
    const double sse_c = sse_cur[b];
    const Pass q = {cur + base, nullptr, nullptr, nullptr, nu + base, prop + base, prop_op ? prop_op + base : nullptr};
    double theta, logy;
    const double ss = start_step(a, q, a.chain0 + b, lo, hi, 0, sse_c, theta, logy);
    const double tot = block_sum_256(ss, red);
    if (threadIdx.x != 0) return;
    sq_parts[(int64_t)b * gridDim.x + blockIdx.x] = tot;            // slot 0
    if (blockIdx.x != 0) return;
    double* eo = es + (int64_t)b * NES;
    eo[0] = theta; eo[1] = theta - TWO_PI; eo[2] = theta; eo[3] = logy; eo[4] = sse_c; eo[5] = lp_cur[b];
    int64_t* io = ei + (int64_t)b * NEI;
    io[0] = 0; io[1] = 0; io[2] = 0; io[3] = 0;
}

// cur / nu / prop are read and written through the same pointers (in place, element by element): no __restrict__ on them
__global__ __launch_bounds__(HBLK) void k_ess_iter(EssArgs a, const double* __restrict__ sse_prop, double* cur, double* nu,
                                                   double* prop, float* __restrict__ prop_op, double* __restrict__ best,
                                                   double* best_lp, double* __restrict__ chain, double* __restrict__ lps,
                                                   int32_t* __restrict__ nev, double* sq_parts, double* es, int64_t* ei) {
    __shared__ double red[4];
    const int b = blockIdx.y, part = blockIdx.x, nwg = gridDim.x;
    const int64_t so = (int64_t)a.par * a.C + b, sn = (int64_t)(1 - a.par) * a.C + b;
    const int64_t* ii = ei + so * NEI;
    const double* ein = es + so * NES;
    int64_t* io = ei + sn * NEI;
    double* eo = es + sn * NES;
    const bool w0 = part == 0 && threadIdx.x == 0;
    // ---- the chain's scalars: every workgroup of the chain reads the same numbers
    const int64_t t = ii[0], j = ii[1], ntrunc = ii[2], nevals = ii[3];
    double theta = ein[0], tmin = ein[1], tmax = ein[2], logy = ein[3];
    const double sse_c = ein[4], lp_c = ein[5], blp = best_lp[so];
    if (t >= a.nmcmc) {                                             // done: the scalars are carried over, nothing else is touched
        if (threadIdx.x == 0) sq_parts[sn * nwg + part] = sq_parts[so * nwg + part];
        if (w0) {
            eo[0] = theta; eo[1] = tmin; eo[2] = tmax; eo[3] = logy; eo[4] = sse_c; eo[5] = lp_c;
            io[0] = t; io[1] = j; io[2] = ntrunc; io[3] = nevals;
            best_lp[sn] = blp;
        }
        return;
    }
    double ssep = sse_prop[(int64_t)b * a.nparts];
    for (int k = 1; k < a.nparts; ++k) ssep = ssep + sse_prop[(int64_t)b * a.nparts + k];
    const bool acc = isfinite(ssep) && a.gs * ssep > logy;           // (NaN: a rejection)
    const int64_t base = (int64_t)b * a.p;
    const int chain_id = a.chain0 + b;
    int64_t lo, hi;
    pair_range(a.p, lo, hi);
    float* pop = prop_op ? prop_op + base : nullptr;
    if (!acc && j + 1 < a.max_shrink) {
        // ---- shrink the bracket towards theta = 0 (the current point) and propose again
        if (theta < 0.0) tmin = theta; else tmax = theta;
        Philox ph;
        ph.gen(a.seed, (uint64_t)t, ctr_of(chain_id, PURPOSE_ANGLE, (uint64_t)(j + 1)));
        theta = tmin + u01(ph.c[0], ph.c[1]) * (tmax - tmin);
        double sv, cv;
        sincos(theta, &sv, &cv);
        const Pass q = {cur + base, nullptr, nullptr, nullptr, nu + base, prop + base, pop};
        const double tot = block_sum_256(ellipse_pass(a, q, chain_id, lo, hi, true, false, 0, cv, sv), red);
        if (threadIdx.x == 0) sq_parts[sn * nwg + part] = tot;
        if (w0) {
            eo[0] = theta; eo[1] = tmin; eo[2] = tmax; eo[3] = logy; eo[4] = sse_c; eo[5] = lp_c;
            io[0] = t; io[1] = j + 1; io[2] = ntrunc; io[3] = nevals + 1;
            best_lp[sn] = blp;
        }
        return;
    }
    // ---- the step ends: the proposal is accepted, or the step is truncated and the chain stays where it is
    const int64_t t1 = t + 1;
    double lp_new = lp_c, sse_new = sse_c;
    bool better = false;
    if (acc) {
        double sq = sq_parts[so * nwg];
        for (int k = 1; k < nwg; ++k) sq = sq + sq_parts[so * nwg + k];
        lp_new = (a.gs * ssep - a.lik_const) + (a.pscale * sq - a.prior_const);
        sse_new = ssep;
        better = lp_new >= blp;                                     // (NaN: never)
    }
    const int64_t row = (int64_t)b * (a.nmcmc + 1) + t1;              // t1 <= nmcmc: inside [C, nmcmc + 1]
    const Pass q = {(acc ? prop : cur) + base, acc ? cur + base : nullptr, chain ? chain + row * a.p : nullptr,
                    better ? best + base : nullptr, nu + base, prop + base, pop};
    double ss;
    if (t1 < a.nmcmc) {                                             // the next step starts in the same launch
        ss = start_step(a, q, chain_id, lo, hi, (uint64_t)t1, sse_new, theta, logy);
        tmin = theta - TWO_PI;
        tmax = theta;
    } else {
        ss = ellipse_pass(a, q, chain_id, lo, hi, false, false, 0, 0.0, 0.0);
    }
    const double tot = block_sum_256(ss, red);
    if (threadIdx.x == 0) sq_parts[sn * nwg + part] = tot;
    if (w0) {
        lps[row] = lp_new;
        nev[row] = acc ? (int32_t)(j + 1) : a.max_shrink;
        eo[0] = theta; eo[1] = tmin; eo[2] = tmax; eo[3] = logy; eo[4] = sse_new; eo[5] = lp_new;
        io[0] = t1; io[1] = 0; io[2] = acc ? ntrunc : ntrunc + 1; io[3] = nevals + 1;
        best_lp[sn] = better ? lp_new : blp;
    }
}

bool ess_common_bad(const char* who, double sigma, double priorsigma, int C, int chain0, int64_t p, int dtype, const void* prop_op) {
    if (C < 1 || C > 65535 || chain0 < 0 || p < 1) {
        qn_set_error("%s: bad size (1 <= C = %d <= 65535, chain0 = %d >= 0, p = %lld >= 1)", who, C, chain0, (long long)p);
        return true;
    }
    if (!(sigma > 0.0) || !std::isfinite(sigma) || !(priorsigma > 0.0) || !std::isfinite(priorsigma)) {
        qn_set_error("%s: sigma = %g and priorsigma = %g must be > 0 and finite", who, sigma, priorsigma);
        return true;
    }
    if (dtype != QN_F64 && dtype != QN_F32) {
        qn_set_error("%s: dtype = %d is neither QN_F64 nor QN_F32", who, dtype);
        return true;
    }
    if (prop_op && dtype != QN_F32) {
        qn_set_error("%s: prop_op (the proposal as float32) goes with dtype QN_F32 only", who);
        return true;
    }
    return false;
}

EssArgs ess_args(double sigma, double priorsigma, int n_rows, int C, int chain0, int64_t p, uint64_t seed) {
    EssArgs a;
    a.gs = -0.5 / (sigma * sigma);
    a.lik_const = 0.5 * n_rows * std::log(2.0 * M_PI) + n_rows * std::log(sigma);
    a.s = priorsigma;
    a.pscale = -0.5 / (priorsigma * priorsigma);
    a.prior_const = 0.5 * (double)p * std::log(2.0 * M_PI * priorsigma * priorsigma);
    a.C = C; a.chain0 = chain0; a.nmcmc = 0; a.max_shrink = 0; a.nparts = 0; a.par = 0;
    a.p = p; a.seed = seed;
    return a;
}

}  // namespace

extern "C" int qn_ess_begin(const double* cur, const double* sse_cur, const double* lp_cur, double sigma, double priorsigma,
                            int C, int chain0, int64_t p, uint64_t seed, double* nu, double* prop, void* prop_op, int dtype,
                            double* sq_parts, double* es, int64_t* ei, void* stream) {
    if (ess_common_bad("qn_ess_begin", sigma, priorsigma, C, chain0, p, dtype, prop_op)) return QN_EINVAL;
    if (!cur || !sse_cur || !lp_cur || !nu || !prop || !sq_parts || !es || !ei) {
        qn_set_error("qn_ess_begin: a NULL pointer (only prop_op may be NULL)");
        return QN_EINVAL;
    }
    const EssArgs a = ess_args(sigma, priorsigma, 0, C, chain0, p, seed);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ess_begin, dim3(hmc_parts(p), C), dim3(HBLK), 0, static_cast<hipStream_t>(stream), a, cur, sse_cur,
                       lp_cur, nu, prop, static_cast<float*>(prop_op), sq_parts, es, ei);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}

extern "C" int qn_ess_iter(const double* sse_prop, int nparts, double sigma, double priorsigma, int n_rows, int max_shrink, int C,
                           int chain0, int64_t p, int nmcmc, uint64_t seed, double* cur, double* nu, double* prop, void* prop_op,
                           int dtype, double* best, double* best_lp, double* chain, double* lps, int32_t* nev, double* sq_parts,
                           double* es, int64_t* ei, int parity, void* stream) {
    if (ess_common_bad("qn_ess_iter", sigma, priorsigma, C, chain0, p, dtype, prop_op)) return QN_EINVAL;
    if (nmcmc < 1 || max_shrink < 1 || nparts < 1 || n_rows < 1 || (parity != 0 && parity != 1)) {
        qn_set_error("qn_ess_iter: nmcmc = %d, max_shrink = %d, nparts = %d and n_rows = %d must be >= 1, parity = %d 0 or 1",
                     nmcmc, max_shrink, nparts, n_rows, parity);
        return QN_EINVAL;
    }
    if (!sse_prop || !cur || !nu || !prop || !best || !best_lp || !lps || !nev || !sq_parts || !es || !ei) {
        qn_set_error("qn_ess_iter: a NULL pointer (only chain and prop_op may be NULL)");
        return QN_EINVAL;
    }
    EssArgs a = ess_args(sigma, priorsigma, n_rows, C, chain0, p, seed);
    a.nmcmc = nmcmc; a.max_shrink = max_shrink; a.nparts = nparts; a.par = parity;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ess_iter, dim3(hmc_parts(p), C), dim3(HBLK), 0, static_cast<hipStream_t>(stream), a, sse_prop, cur, nu,
                       prop, static_cast<float*>(prop_op), best, best_lp, chain, lps, nev, sq_parts, es, ei);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
