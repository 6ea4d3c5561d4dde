// The No-U-Turn sampler on the device (Hoffman & Gelman 2014; multinomial weights, Betancourt 2017; build-only, the reference
// has no such sampler) in its ITERATIVE form with ASYNCHRONOUS chain steps: one leapfrog -- one gradient call -- per
// iteration, every U-turn test of the trajectory's binary tree from O(depth) checkpoints, every chain on its own step counter.
// quinn_amd/mcmc/nuts.py states the rule and restates it in numpy; include/quinn_amd.h has the contract of the entry points.
//   qn_nuts_begin : start of step 0 of every chain (momenta, edges, the first half kick and drift)
//   qn_nuts_iter  : one iteration on the SSE and d SSE / d W of the pending points; two launches
//       k_nuts_reduce  completes the kick (u' = u + (hk s) g'), adds u' to the subtree's momentum sum, stores an even leaf's
//                      checkpoint, and writes per workgroup the partial sums of every dot product the decision can need:
//                      |u'|^2, two per live checkpoint of an odd leaf, and, at the last leaf of a subtree, the two of the tree
//                      with rho + rho_sub and the edges as they would stand after the merge
//       k_nuts_decide  every workgroup adds the partials left to right and comes to the same decision -- divergent, turning,
//                      next leaf, merge and double, step end and the start of the next step -- and performs its slice of the
//                      copies (subtree proposal, tree proposal, edge, chain row, MAP) and of the next half kick and drift
// Geometry of the HMC elementwise kernels: hmc_parts(p) workgroups of HBLK threads per chain, a pair of elements per 16-byte
// access and per Philox block; an element belongs to the same thread in both kernels, so the vectors are updated in place.  The
// chain's scalars are read from slot `parity` and written, by workgroup 0 alone, to slot 1 - parity: no workgroup sees a
// half-updated chain, no atomics, no fences, equal inputs give equal bits, and a chain does not see the others.  HBM-bound: a
// leaf in the middle of a subtree moves 10 x 8 B per element (reduce: u, g', rho_sub read, u, rho_sub written; decide: q, u, g'
// read, q, u written; + the scale) plus 2 per checkpoint stored or tested; a done chain nothing.  FP contraction is off for the
// whole file: every elementwise update takes one rounding per operation, as the numpy restatement does.
#include "qn_mcmc_shared.h"

#pragma clang fp contract(off)

namespace {

// Philox purposes of this file (qn_mcmc_shared.h lists them all): 9 the momenta (index = column pair), 10 the scalar uniforms
// (index = (kind << 32) | n; kind 0: direction of doubling n, 1: merge of doubling n, 2: the leaf whose n_leap was n).  The
// stream is the chain's own step t.
constexpr int PURPOSE_MOM = 9;
constexpr int PURPOSE_UNIF = 10;
constexpr int KIND_DIR = 0, KIND_MERGE = 1, KIND_LEAF = 2;
constexpr int MAXD = 12;                       // max_depth <= 12
constexpr int NDOT = 3 + 2 * MAXD;             // slots of dot_parts: 0 |u'|^2; 1 + 2k, 2 + 2k checkpoint k; 25, 26 the tree
constexpr int NES = 12;  // es: eps, mu, hbar, logbar, H0, logW, logW_sub, sum_a, sse_cur, lp_cur, sse_sub, lp_sub
constexpr int NEI = 8;   // ei: t, d, i, v, n_leap, ndiv, ntreedepth, ngrad
constexpr double DIVERGENCE = 1000.0;

struct NutsArgs {
    double gs;                                 // -0.5 / sigma^2
    double lik_const;                          // (N / 2) log 2 pi + N log sigma
    double target;                             // target_accept
    int C, chain0, nmcmc, max_depth, adapt, par;
    int64_t p;
    uint64_t seed;
};

struct NutsVec {                               // the [C, p] arrays (ck_u, ck_rho: [C, max_depth, p]); scale may be NULL (1)
    double *cur, *gcur, *ql, *ul, *gl, *qr, *ur, *gr, *rho, *q, *u, *rho_sub, *sub_q, *sub_g, *ck_u, *ck_rho, *best;
    const double* scale;
};

__device__ __forceinline__ void pair_range(int64_t p, int64_t& lo, int64_t& hi) {
    const int64_t npair = (p + 1) / 2;
    const int64_t pchunk = (npair + gridDim.x - 1) / gridDim.x;
    lo = blockIdx.x * pchunk;
    hi = lo + pchunk < npair ? lo + pchunk : npair;
}

// Counters a caller-written state must respect for every index below to stay inside its array (t, d, i of ei): a chain whose
// counters do not is left alone like a done one.
__device__ __forceinline__ bool state_ok(const NutsArgs& a, const int64_t* ii) {
    return ii[0] >= 0 && ii[1] >= 0 && ii[1] < a.max_depth && ii[2] >= 0 && ii[2] < ((int64_t)1 << ii[1]);
}

__device__ __forceinline__ double nuts_unif(const NutsArgs& a, uint64_t t, int chain, int kind, uint64_t n) {
    Philox ph;
    ph.gen(a.seed, t, ctr_of(chain, PURPOSE_UNIF, ((uint64_t)kind << 32) | n));
    return u01(ph.c[0], ph.c[1]);
}

// log(exp(x) + exp(y)) = max + log1p(exp(-|x - y|)); an infinite or NaN difference gives max (nuts.py: logaddexp)
__device__ __forceinline__ double log_add_exp(double x, double y) {
    const double hi = x >= y ? x : y, lo = x >= y ? y : x;
    const double d = lo - hi;
    if (!(d > -INFINITY)) return hi;
    return hi + log1p(exp(d));
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// first half of a leapfrog in direction v from the node (q, u, g): u_half = u + (hk s) g, q' = q + (dr s) u_half
__device__ __forceinline__ void kick_drift(double hk, double dr, const d2u& s, const d2u& q, const d2u& u, const d2u& g,
                                           double* q_out, double* u_out, bool both) {
    const double u0 = u.x + (hk * s.x) * g.x, u1 = u.y + (hk * s.y) * g.y;
    const double q0 = q.x + (dr * s.x) * u0, q1 = q.y + (dr * s.y) * u1;
    st2(u_out, u0, u1, both);
    st2(q_out, q0, q1, both);
}

// Start of step t of a chain from the point x with gradient xg (one pair of elements): momenta z, both edges = (x, z, xg),
// rho = z, the first half kick and drift in direction v.  Returns the pair's z^2.
__device__ __forceinline__ double start_pair(const NutsArgs& a, const NutsVec& w, int chain, uint64_t t, int64_t base, int64_t j,
                                             const d2u& x, const d2u& xg, const d2u& s, double hk, double dr) {
    const int64_t e = 2 * j, o = base + e;
    const bool both = e + 1 < a.p;
    Philox ph;
    ph.gen(a.seed, t, ctr_of(chain, PURPOSE_MOM, (uint64_t)j));
    d2u z;
    double z0, z1;
    normal2(ph, z0, z1);
    z.x = z0; z.y = both ? z1 : 0.0;
    st2(w.ql + o, x.x, x.y, both); st2(w.qr + o, x.x, x.y, both);
    st2(w.ul + o, z.x, z.y, both); st2(w.ur + o, z.x, z.y, both);
    st2(w.gl + o, xg.x, xg.y, both); st2(w.gr + o, xg.x, xg.y, both);
    st2(w.rho + o, z.x, z.y, both);
    kick_drift(hk, dr, s, x, z, xg, w.q + o, w.u + o, both);
    return z.x * z.x + z.y * z.y;
}

__global__ __launch_bounds__(HBLK) void k_nuts_begin(NutsArgs a, NutsVec w, const double* __restrict__ sse_cur,
                                                     const double* __restrict__ eps0, double* __restrict__ zz_parts,
                                                     double* __restrict__ best_lp, double* __restrict__ es,
                                                     int64_t* __restrict__ ei) {
    __shared__ double red[4];
    const int b = blockIdx.y, chain = a.chain0 + b;
    const int64_t base = (int64_t)b * a.p;
    int64_t lo, hi;
    pair_range(a.p, lo, hi);
    const double eps = eps0[b];
    const int v = nuts_unif(a, 0, chain, KIND_DIR, 0) < 0.5 ? 1 : -1;
    const double hk = (double)v * ((0.5 * eps) * a.gs), dr = (double)v * eps;
    const d2u one = {1.0, 1.0};
    double zz = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += HBLK) {
        const int64_t o = base + 2 * j;
        const bool both = 2 * j + 1 < a.p;
        zz = zz + start_pair(a, w, chain, 0, base, j, ld2(w.cur + o, both), ld2(w.gcur + o, both),
                             w.scale ? ld2(w.scale + o, both) : one, hk, dr);
    }
    const double tot = block_sum_256(zz, red);
    if (threadIdx.x != 0) return;
    zz_parts[(int64_t)b * gridDim.x + blockIdx.x] = tot;            // slot 0
    if (blockIdx.x != 0) return;
    const double lp = a.gs * sse_cur[b] - a.lik_const;
    double* eo = es + (int64_t)b * NES;
    eo[0] = eps; eo[1] = log(10.0 * eps); eo[2] = 0.0; eo[3] = 0.0; eo[4] = 0.0; eo[5] = 0.0; eo[6] = 0.0; eo[7] = 0.0;
    eo[8] = sse_cur[b]; eo[9] = lp; eo[10] = 0.0; eo[11] = 0.0;
    int64_t* io = ei + (int64_t)b * NEI;
    io[0] = 0; io[1] = 0; io[2] = 0; io[3] = v; io[4] = 0; io[5] = 0; io[6] = 0; io[7] = 0;
    best_lp[b] = lp;
}

// the vectors are read and written through the same pointers (in place, element by element): no __restrict__ on them
__global__ __launch_bounds__(HBLK) void k_nuts_reduce(NutsArgs a, NutsVec w, const double* __restrict__ grad,
                                                      const double* __restrict__ es, const int64_t* __restrict__ ei,
                                                      double* __restrict__ dot_parts) {
    __shared__ double red[NDOT][4];
    const int b = blockIdx.y;
    const int64_t so = (int64_t)a.par * a.C + b;
    const int64_t* ii = ei + so * NEI;
    if (ii[0] >= a.nmcmc || !state_ok(a, ii)) return;               // done: nothing is read or written
    const int d = (int)ii[1], v = (int)ii[3];
    const int64_t i = ii[2];
    const double hk = (double)v * ((0.5 * es[so * NES]) * a.gs);
    const bool first = i == 0, odd = (i & 1) != 0, complete = i + 1 == ((int64_t)1 << d);
    const int kmax = __popcll((unsigned long long)(i >> 1));
    const int kmin = kmax - (__ffsll(~(long long)i) - 1) + 1;       // (trailing one bits of i; an even leaf has no test)
    const bool store_ck = !odd && !complete;
    const int64_t base = (int64_t)b * a.p, cbase = (int64_t)b * a.max_depth * a.p;
    const double* uo = v > 0 ? w.ul : w.ur;                         // the edge the subtree does not move
    int64_t lo, hi;
    pair_range(a.p, lo, hi);
    const d2u one = {1.0, 1.0};
    double uu = 0.0, tl = 0.0, tr = 0.0, ca[MAXD], cb[MAXD];
#pragma unroll
    for (int k = 0; k < MAXD; ++k) ca[k] = cb[k] = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += HBLK) {
        const int64_t e = 2 * j, o = base + e;
        const bool both = e + 1 < a.p;
        const d2u uh = ld2(w.u + o, both), g = ld2(grad + o, both), s = w.scale ? ld2(w.scale + o, both) : one;
        d2u u1, rs;
        u1.x = uh.x + (hk * s.x) * g.x;
        u1.y = both ? uh.y + (hk * s.y) * g.y : 0.0;
        if (first) rs = u1;
        else { const d2u r0 = ld2(w.rho_sub + o, both); rs.x = r0.x + u1.x; rs.y = r0.y + u1.y; }
        st2(w.u + o, u1.x, u1.y, both);
        st2(w.rho_sub + o, rs.x, rs.y, both);
        uu = uu + (u1.x * u1.x + u1.y * u1.y);
        if (store_ck) {
            st2(w.ck_u + cbase + kmax * a.p + e, u1.x, u1.y, both);
            st2(w.ck_rho + cbase + kmax * a.p + e, rs.x, rs.y, both);
        }
        if (odd) {
#pragma unroll
            for (int k = 0; k < MAXD - 1; ++k) {
                if (k < kmin || k > kmax) continue;
                const d2u cu = ld2(w.ck_u + cbase + k * a.p + e, both), cr = ld2(w.ck_rho + cbase + k * a.p + e, both);
                const double r0 = (rs.x - cr.x) + cu.x, r1 = (rs.y - cr.y) + cu.y;
                ca[k] = ca[k] + (r0 * cu.x + r1 * cu.y);
                cb[k] = cb[k] + (r0 * u1.x + r1 * u1.y);
            }
        }
        if (complete) {
            const d2u r = ld2(w.rho + o, both), eo = ld2(uo + o, both);
            const double r0 = r.x + rs.x, r1 = r.y + rs.y;
            const double de = r0 * eo.x + r1 * eo.y, dl = r0 * u1.x + r1 * u1.y;
            tl = tl + (v > 0 ? de : dl);
            tr = tr + (v > 0 ? dl : de);
        }
    }
    // ---- one fixed-order block sum per live slot (the conditions are uniform over the workgroup)
    const int wv = threadIdx.x >> 6;
    const bool l0 = (threadIdx.x & 63) == 0;
    double x = wave_sum(uu);
    if (l0) red[0][wv] = x;
    if (odd) {
#pragma unroll
        for (int k = 0; k < MAXD - 1; ++k) {
            if (k < kmin || k > kmax) continue;
            x = wave_sum(ca[k]);
            if (l0) red[1 + 2 * k][wv] = x;
            x = wave_sum(cb[k]);
            if (l0) red[2 + 2 * k][wv] = x;
        }
    }
    if (complete) {
        x = wave_sum(tl);
        if (l0) red[NDOT - 2][wv] = x;
        x = wave_sum(tr);
        if (l0) red[NDOT - 1][wv] = x;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double* out = dot_parts + ((int64_t)b * gridDim.x + blockIdx.x) * NDOT;
    out[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    if (odd)
        for (int k = kmin; k <= kmax; ++k) {
            out[1 + 2 * k] = (red[1 + 2 * k][0] + red[1 + 2 * k][1]) + (red[1 + 2 * k][2] + red[1 + 2 * k][3]);
            out[2 + 2 * k] = (red[2 + 2 * k][0] + red[2 + 2 * k][1]) + (red[2 + 2 * k][2] + red[2 + 2 * k][3]);
        }
    if (complete)
        for (int k = NDOT - 2; k < NDOT; ++k) out[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
}

__device__ __forceinline__ double dot_total(const double* dot_parts, int64_t b, int nwg, int slot) {
    double s = dot_parts[(b * nwg) * NDOT + slot];
    for (int k = 1; k < nwg; ++k) s = s + dot_parts[(b * nwg + k) * NDOT + slot];
    return s;
}

__global__ __launch_bounds__(HBLK) void k_nuts_decide(NutsArgs a, NutsVec w, const double* __restrict__ sse_in,
                                                      const double* __restrict__ grad, double* best_lp,
                                                      double* __restrict__ chain, double* __restrict__ lps,
                                                      double* __restrict__ alphas, int32_t* __restrict__ depth,
                                                      int32_t* __restrict__ nleap, const double* __restrict__ dot_parts,
                                                      double* zz_parts, double* es, int64_t* ei) {
    __shared__ double red[4];
    const int b = blockIdx.y, part = blockIdx.x, nwg = gridDim.x, chain_id = a.chain0 + b;
    const int64_t so = (int64_t)a.par * a.C + b, sn = (int64_t)(1 - a.par) * a.C + b;
    const int64_t* ii = ei + so * NEI;
    const double* ein = es + so * NES;
    int64_t* io = ei + sn * NEI;
    double* eo = es + sn * NES;
    const bool w0 = part == 0 && threadIdx.x == 0;
    // ---- the chain's scalars: every workgroup of the chain reads the same numbers
    int64_t t = ii[0], d = ii[1], i = ii[2], v = ii[3], n_leap = ii[4], ndiv = ii[5], ntd = ii[6], ngrad = ii[7];
    double eps = ein[0], mu = ein[1], hbar = ein[2], logbar = ein[3], H0 = ein[4], logW = ein[5], logWs = ein[6], suma = ein[7],
           sse_c = ein[8], lp_c = ein[9], sse_s = ein[10], lp_s = ein[11];
    const double blp = best_lp[so];
    if (t >= a.nmcmc || !state_ok(a, ii)) {                         // done: the scalars are carried over, nothing else is touched
        if (w0) {
#pragma unroll
            for (int k = 0; k < NES; ++k) eo[k] = ein[k];
#pragma unroll
            for (int k = 0; k < NEI; ++k) io[k] = ii[k];
            best_lp[sn] = blp;
        }
        return;
    }
    const int64_t bb = b;
    if (n_leap == 0) {                                              // the first leaf of the step: H0 from the momenta's parts
        double zz = zz_parts[so * nwg];
        for (int k = 1; k < nwg; ++k) zz = zz + zz_parts[so * nwg + k];
        H0 = -lp_c + 0.5 * zz;
    }
    // ---- the leaf
    const double sse = sse_in[b], lp1 = a.gs * sse - a.lik_const;
    double dE = (-lp1 + 0.5 * dot_total(dot_parts, bb, nwg, 0)) - H0;
    if (!(dE == dE)) dE = INFINITY;
    const int64_t n0 = n_leap;
    suma = suma + fmin(1.0, exp(-dE));
    n_leap += 1;
    ngrad += 1;
    const bool divergent = dE > DIVERGENCE, complete = i + 1 == ((int64_t)1 << d);
    const double hk = (double)v * ((0.5 * eps) * a.gs), dr = (double)v * eps;     // (of the subtree's direction)
    bool turn = false, sel = false, merged = false;
    if (!divergent) {
        logWs = i == 0 ? -dE : log_add_exp(logWs, -dE);
        sel = nuts_unif(a, (uint64_t)t, chain_id, KIND_LEAF, (uint64_t)n0) < exp(-dE - logWs);
        if (sel) { sse_s = sse; lp_s = lp1; }
        if (i & 1) {
            const int kmax = __popcll((unsigned long long)(i >> 1));
            const int kmin = kmax - (__ffsll(~(long long)i) - 1) + 1;
            for (int k = kmax; k >= kmin; --k)
                turn = turn || dot_total(dot_parts, bb, nwg, 1 + 2 * k) <= 0.0 || dot_total(dot_parts, bb, nwg, 2 + 2 * k) <= 0.0;
        }
    }
    const int64_t base = (int64_t)b * a.p;
    int64_t lo, hi;
    pair_range(a.p, lo, hi);
    const d2u one = {1.0, 1.0};
    bool end = divergent || turn;
    int dep = (int)d + 1;                                           // (ended inside a subtree: the doublings started)
    if (!end && !complete) {
        // ---- the subtree goes on: the next leapfrog starts from this leaf
        for (int64_t j = lo + threadIdx.x; j < hi; j += HBLK) {
            const int64_t e = 2 * j, o = base + e;
            const bool both = e + 1 < a.p;
            const d2u qv = ld2(w.q + o, both), uv = ld2(w.u + o, both), gv = ld2(grad + o, both);
            if (sel) { st2(w.sub_q + o, qv.x, qv.y, both); st2(w.sub_g + o, gv.x, gv.y, both); }
            kick_drift(hk, dr, w.scale ? ld2(w.scale + o, both) : one, qv, uv, gv, w.q + o, w.u + o, both);
        }
        if (w0) {
            eo[0] = eps; eo[1] = mu; eo[2] = hbar; eo[3] = logbar; eo[4] = H0; eo[5] = logW; eo[6] = logWs; eo[7] = suma;
            eo[8] = sse_c; eo[9] = lp_c; eo[10] = sse_s; eo[11] = lp_s;
            io[0] = t; io[1] = d; io[2] = i + 1; io[3] = v; io[4] = n_leap; io[5] = ndiv; io[6] = ntd; io[7] = ngrad;
            best_lp[sn] = blp;
        }
        return;
    }
    int64_t v2 = v;
    if (!end) {
        // ---- the subtree is complete: merge it, double, and see whether the tree goes on
        merged = nuts_unif(a, (uint64_t)t, chain_id, KIND_MERGE, (uint64_t)d) < exp(logWs - logW);
        if (merged) { sse_c = sse_s; lp_c = lp_s; }
        logW = log_add_exp(logW, logWs);
        d += 1;
        dep = (int)d;
        if (dot_total(dot_parts, bb, nwg, NDOT - 2) <= 0.0 || dot_total(dot_parts, bb, nwg, NDOT - 1) <= 0.0) end = true;
        else if (d == a.max_depth) { end = true; ntd += 1; }
        else v2 = nuts_unif(a, (uint64_t)t, chain_id, KIND_DIR, (uint64_t)d) < 0.5 ? 1 : -1;
    }
    const bool leafvals = !(divergent || turn);                     // the leaf's vectors are needed: it is merged
    // ---- the step's end, in scalars
    const int64_t t1 = t + 1;
    const int64_t row = (int64_t)b * (a.nmcmc + 1) + t1;            // t1 <= nmcmc: inside [C, nmcmc + 1]
    const double astat = suma / (double)n_leap;
    bool better = false, next = false;
    int64_t v0 = 1;
    double hk0 = 0.0, dr0 = 0.0;
    if (end) {
        better = lp_c >= blp;                                       // (NaN: never)
        if (t < a.adapt) {                                          // dual averaging of the step size (qn_hmc_adapt's formula)
            const double m = (double)t1, acc = astat == astat ? fmin(1.0, astat) : 0.0, wgt = 1.0 / (m + 10.0);
            hbar = (1.0 - wgt) * hbar + (a.target - acc) * wgt;
            const double logeps = mu - (sqrt(m) / 0.05) * hbar, eta = pow(m, -0.75);
            logbar = eta * logeps + (1.0 - eta) * logbar;
            eps = exp(t1 == a.adapt ? logbar : logeps);
        }
        next = t1 < a.nmcmc;
        if (next) {
            v0 = nuts_unif(a, (uint64_t)t1, chain_id, KIND_DIR, 0) < 0.5 ? 1 : -1;
            hk0 = (double)v0 * ((0.5 * eps) * a.gs);
            dr0 = (double)v0 * eps;
        }
    }
    const double hk2 = (double)v2 * ((0.5 * eps) * a.gs), dr2 = (double)v2 * eps;
    double* eq = v > 0 ? w.qr : w.ql;                               // the edge the subtree moved
    double* eu = v > 0 ? w.ur : w.ul;
    double* eg = v > 0 ? w.gr : w.gl;
    const double* oq = v2 > 0 ? w.qr : w.ql;                        // the edge the next subtree starts from
    const double* ou = v2 > 0 ? w.ur : w.ul;
    const double* og = v2 > 0 ? w.gr : w.gl;
    double* crow = chain ? chain + row * a.p : nullptr;
    double zz = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += HBLK) {
        const int64_t e = 2 * j, o = base + e;
        const bool both = e + 1 < a.p;
        const d2u zero = {0.0, 0.0};
        d2u qv = zero, uv = zero, gv = zero, x = zero, xg = zero;
        bool have_x = false;
        if (leafvals) {
            qv = ld2(w.q + o, both); uv = ld2(w.u + o, both); gv = ld2(grad + o, both);
            if (sel) { st2(w.sub_q + o, qv.x, qv.y, both); st2(w.sub_g + o, gv.x, gv.y, both); }
            if (merged) {                                           // the tree's proposal becomes the subtree's
                if (sel) { x = qv; xg = gv; }
                else { x = ld2(w.sub_q + o, both); xg = ld2(w.sub_g + o, both); }
                st2(w.cur + o, x.x, x.y, both);
                st2(w.gcur + o, xg.x, xg.y, both);
                have_x = true;
            }
            if (!end) {                                             // the tree goes on: rho, the moved edge, the next subtree's leaf 0
                const d2u r = ld2(w.rho + o, both), rs = ld2(w.rho_sub + o, both);
                st2(w.rho + o, r.x + rs.x, r.y + rs.y, both);
                st2(eq + o, qv.x, qv.y, both); st2(eu + o, uv.x, uv.y, both); st2(eg + o, gv.x, gv.y, both);
                const d2u s = w.scale ? ld2(w.scale + o, both) : one;
                if (v2 == v) kick_drift(hk2, dr2, s, qv, uv, gv, w.q + o, w.u + o, both);
                else kick_drift(hk2, dr2, s, ld2(oq + o, both), ld2(ou + o, both), ld2(og + o, both), w.q + o, w.u + o, both);
            }
        }
        if (end) {
            if (!have_x) {
                x = ld2(w.cur + o, both);
                if (next) xg = ld2(w.gcur + o, both);
            }
            if (crow) st2(crow + e, x.x, x.y, both);
            if (better) st2(w.best + o, x.x, x.y, both);
            if (next) zz = zz + start_pair(a, w, chain_id, (uint64_t)t1, base, j, x, xg, w.scale ? ld2(w.scale + o, both) : one, hk0, dr0);
        }
    }
    if (end && next) {
        const double tot = block_sum_256(zz, red);
        if (threadIdx.x == 0) zz_parts[sn * nwg + part] = tot;
    }
    if (!w0) return;
    if (end) {
        lps[row] = lp_c;
        alphas[row] = astat;
        depth[row] = dep;
        nleap[row] = (int32_t)n_leap;
        eo[0] = eps; eo[1] = mu; eo[2] = hbar; eo[3] = logbar; eo[4] = H0; eo[5] = 0.0; eo[6] = logWs; eo[7] = 0.0;
        eo[8] = sse_c; eo[9] = lp_c; eo[10] = sse_s; eo[11] = lp_s;
        io[0] = t1; io[1] = next ? 0 : d; io[2] = next ? 0 : i; io[3] = next ? v0 : v; io[4] = next ? 0 : n_leap;
        io[5] = ndiv + (divergent ? 1 : 0); io[6] = ntd; io[7] = ngrad;
        if (!next) { eo[5] = logW; eo[7] = suma; }
        best_lp[sn] = better ? lp_c : blp;
    } else {
        eo[0] = eps; eo[1] = mu; eo[2] = hbar; eo[3] = logbar; eo[4] = H0; eo[5] = logW; eo[6] = logWs; eo[7] = suma;
        eo[8] = sse_c; eo[9] = lp_c; eo[10] = sse_s; eo[11] = lp_s;
        io[0] = t; io[1] = d; io[2] = 0; io[3] = v2; io[4] = n_leap; io[5] = ndiv; io[6] = ntd; io[7] = ngrad;
        best_lp[sn] = blp;
    }
}

bool nuts_common_bad(const char* who, double sigma, int n_rows, int C, int chain0, int64_t p, const NutsVec& w,
                     const void* zz_parts, const void* best_lp, const void* es, const void* ei) {
    if (C < 1 || C > 65535 || chain0 < 0 || p < 1 || n_rows < 1) {
        qn_set_error("%s: bad size (1 <= C = %d <= 65535, chain0 = %d >= 0, p = %lld >= 1, n_rows = %d >= 1)", who, C, chain0,
                     (long long)p, n_rows);
        return true;
    }
    if (!(sigma > 0.0) || !std::isfinite(sigma)) {
        qn_set_error("%s: sigma = %g must be > 0 and finite", who, sigma);
        return true;
    }
    if (!w.cur || !w.gcur || !w.ql || !w.ul || !w.gl || !w.qr || !w.ur || !w.gr || !w.rho || !w.q || !w.u || !zz_parts ||
        !best_lp || !es || !ei) {
        qn_set_error("%s: a NULL pointer (only scale and chain may be NULL)", who);
        return true;
    }
    return false;
}

NutsArgs nuts_args(double sigma, int n_rows, int C, int chain0, int64_t p, uint64_t seed) {
    NutsArgs a;
    a.gs = -0.5 / (sigma * sigma);
    a.lik_const = 0.5 * n_rows * std::log(2.0 * M_PI) + n_rows * std::log(sigma);
    a.target = 0.0;
    a.C = C; a.chain0 = chain0; a.nmcmc = 0; a.max_depth = 0; a.adapt = 0; a.par = 0;
    a.p = p; a.seed = seed;
    return a;
}

}  // namespace

extern "C" int qn_nuts_begin(const double* sse_cur, const double* eps0, const double* scale, double sigma, int n_rows, int C,
                             int chain0, int64_t p, uint64_t seed, const double* cur, const double* gcur, double* ql, double* ul,
                             double* gl, double* qr, double* ur, double* gr, double* rho, double* q, double* u, double* zz_parts,
                             double* best_lp, double* es, int64_t* ei, void* stream) {
    const NutsVec w = {const_cast<double*>(cur), const_cast<double*>(gcur), ql, ul, gl, qr, ur, gr, rho, q, u, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, scale};
    if (nuts_common_bad("qn_nuts_begin", sigma, n_rows, C, chain0, p, w, zz_parts, best_lp, es, ei)) return QN_EINVAL;
    if (!sse_cur || !eps0) {
        qn_set_error("qn_nuts_begin: a NULL pointer (only scale may be NULL)");
        return QN_EINVAL;
    }
    const NutsArgs a = nuts_args(sigma, n_rows, C, chain0, p, seed);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_nuts_begin, dim3(hmc_parts(p), C), dim3(HBLK), 0, static_cast<hipStream_t>(stream), a, w, sse_cur, eps0,
                       zz_parts, best_lp, es, ei);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}

extern "C" int qn_nuts_iter(const double* sse, const double* grad, const double* scale, double sigma, int n_rows, int max_depth,
                            int adapt, double target_accept, int C, int chain0, int64_t p, int nmcmc, uint64_t seed, double* cur,
                            double* gcur, double* ql, double* ul, double* gl, double* qr, double* ur, double* gr, double* rho,
                            double* q, double* u, double* rho_sub, double* sub_q, double* sub_g, double* ck_u, double* ck_rho,
                            double* best, double* best_lp, double* chain, double* lps, double* alphas, int32_t* depth,
                            int32_t* nleap, double* dot_parts, double* zz_parts, double* es, int64_t* ei, int parity,
                            void* stream) {
    const NutsVec w = {cur, gcur, ql, ul, gl, qr, ur, gr, rho, q, u, rho_sub, sub_q, sub_g, ck_u, ck_rho, best, scale};
    if (nuts_common_bad("qn_nuts_iter", sigma, n_rows, C, chain0, p, w, zz_parts, best_lp, es, ei)) return QN_EINVAL;
    if (nmcmc < 1 || max_depth < 1 || max_depth > MAXD || adapt < 0 || adapt > nmcmc || (parity != 0 && parity != 1) ||
        !(target_accept > 0.0 && target_accept < 1.0)) {
        qn_set_error("qn_nuts_iter: nmcmc = %d must be >= 1, max_depth = %d in 1 .. %d, adapt = %d in 0 .. nmcmc, target_accept = %g "
                     "in (0, 1), parity = %d 0 or 1", nmcmc, max_depth, MAXD, adapt, target_accept, parity);
        return QN_EINVAL;
    }
    if (!sse || !grad || !rho_sub || !sub_q || !sub_g || !ck_u || !ck_rho || !best || !lps || !alphas || !depth || !nleap ||
        !dot_parts) {
        qn_set_error("qn_nuts_iter: a NULL pointer (only scale and chain may be NULL)");
        return QN_EINVAL;
    }
    NutsArgs a = nuts_args(sigma, n_rows, C, chain0, p, seed);
    a.target = target_accept; a.nmcmc = nmcmc; a.max_depth = max_depth; a.adapt = adapt; a.par = parity;
    const dim3 grid(hmc_parts(p), C), blk(HBLK);
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_nuts_reduce, grid, blk, 0, st, a, w, grad, es, ei, dot_parts);
    hipLaunchKernelGGL(k_nuts_decide, grid, blk, 0, st, a, w, sse, grad, best_lp, chain, lps, alphas, depth, nleap, dot_parts,
                       zz_parts, es, ei);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
