// Isotropic Gaussian weight prior N(0, priorsigma^2 I) for the device samplers, folded into what the forward / gradient
// kernels return (build-only: the reference has no prior in NN_MCMC).  Every device engine turns a bare SSE and d SSE / d W into
// log-posteriors and forces with gs = -0.5 / sigma^2, so in those units, with lam = sigma^2 / priorsigma^2 and
// c0 = sigma^2 p log(2 pi priorsigma^2),
//     sse' = sse + (lam |w|^2 + c0)      ->  gs sse' = gs sse + log N(w; 0, priorsigma^2 I)
//     g'   = g + (2 lam) w               ->  gs g'   = gs g - w / priorsigma^2
// and one qn_prior_fold launch behind a forward / gradient call hands every accept, leapfrog, adapt, swap and SG kernel the
// posterior with the prior, their code untouched.
// qn_prior_fold_g is the same fold with one precision per weight group and chain, read from device arrays (quinn_amd/mcmc/hyper.py),
// and qn_noise_fold the same with a per-chain noise level kappa, d0 on top (quinn_amd/mcmc/noise.py).  All three are ONE kernel,
// k_fold, driven by a by-value FoldArgs and instantiated per gradient type (float64, float32) and per entry point (a
// compile-time mode of the same body): the scalar prior is one group [0, p) whose factor comes from the arguments (no device
// array is read for it, nothing is staged in LDS for it), no prior is G = 0, the noise term exists in the noise mode alone.  What keeps the three entry points' bits:
//   - FP contraction is off for the whole file (hipcc would fuse a product into the sum): every entry is formed in float64
//     with one rounding per operation, a float32 gradient is widened, updated and rounded once;
//   - the expression at the gradient's store is chosen by the mode and a workgroup-uniform branch on G, never by multiplying by
//     1.0 or adding 0.0:  gv + t  without kappa,  ka gv + t  with kappa and G > 0,  ka gv  with kappa and G = 0 (t = (2 lam) w:
//     a non-finite weight never reaches a gradient that has no prior);
//   - the SSE is  *out + (term + c0)  without kappa,  ((ka *out) + (term + c0)) + d0  with it,  (ka *out) + d0  at G = 0,
//     term = sum_g lam_g S_g accumulated left to right;
//   - the sums of squares S_g run on workgroup 0 of a chain alone, which sums the WHOLE row group by group (group_sumsq), so
//     their order is a function of (p, seg) alone -- not of the grid, not of C, not of the chain's place in the launch -- and
//     that workgroup is the only writer of the chain's SSE entry;
//   - the grid is (grad ? hmc_parts(p) : 1, C) with HBLK threads, the element -> thread map that of k_hmc_leap (group_map).
// Plain vector loads and stores, no atomics, no fences: two calls on equal inputs give equal bits.  A row is 68 KB at cfg2
// (p = 8513).
#include "qn_group_shared.h"

#pragma clang fp contract(off)

namespace {

struct FoldArgs {
    const double *kappa, *d0;             // [C] each (FOLD_NOISE)
    const double *lam, *c0;               // [C, G], [C] (not FOLD_SCALAR)
    const int64_t* seg;                   // [G + 1]
    int G;                                // 0: no weight prior
    double lam1, c01;                     // the scalar prior (FOLD_SCALAR)
    double* sse;
    int sse_stride;
    int64_t p;
};

// The entry point is a compile-time MODE of the one body, so each compiles to the code it needs and no more: FOLD_SCALAR keeps
// nothing in LDS before the gradient pass (the one group [0, p) and its factor come from the arguments) and sums the row as
// group_sumsq sums one segment, operation for operation; FOLD_GROUPS has G >= 1 and no noise term; FOLD_NOISE has 0 <= G.
enum FoldMode { FOLD_SCALAR, FOLD_GROUPS, FOLD_NOISE };

template <typename TG, int MODE>
__global__ __launch_bounds__(HBLK) void k_fold(FoldArgs a, const double* __restrict__ W, TG* __restrict__ g) {
    constexpr bool SCALAR = MODE == FOLD_SCALAR, NOISE = MODE == FOLD_NOISE;
    __shared__ GroupLds l;
    const int b = blockIdx.y, G = SCALAR ? 1 : a.G, GL = SCALAR ? 0 : G;   // GL: the groups kept in LDS
    const int64_t base = (int64_t)b * a.p;
    const double* lam = GL > 0 ? a.lam + (int64_t)b * G : nullptr;
    const double ka = NOISE ? a.kappa[b] : 0.0, f0 = 2.0 * a.lam1;         // (ka: loaded ahead of the staging; f0: the scalar prior's factor)
    if (GL > 0) {
        load_segs(l, a.seg, G, a.p);
        if (threadIdx.x < G) l.fac[threadIdx.x] = 2.0 * lam[threadIdx.x];
        __syncthreads();
    }
    if (g) {
        if (!NOISE) group_map<TG>(l, W + base, g + base, GL, a.p, f0, [](double gv, double t) { return gv + t; });
        else if (G > 0) group_map<TG>(l, W + base, g + base, GL, a.p, f0, [ka](double gv, double t) { return ka * gv + t; });
        else group_map<TG>(l, W + base, g + base, GL, a.p, f0, [ka](double gv, double) { return ka * gv; });
    }
    if (!a.sse || blockIdx.x != 0) return;                                 // (uniform over the workgroup)
    double tot = 0.0;
    if (SCALAR) tot = block_sum_256(segment_sumsq(W + base, 0, a.p), l.red);
    else if (G > 0) group_sumsq(l, W + base, G);
    if (threadIdx.x == 0) {
        double* out = a.sse + (int64_t)b * a.sse_stride;
        double v = NOISE ? ka * *out : *out;
        if (SCALAR) v = v + (a.lam1 * tot + a.c01);
        else if (G > 0) v = v + prior_term(l, lam, a.c0[b], G);
        *out = NOISE ? v + a.d0[b] : v;
    }
}

template <typename TG>
void fold_go(int mode, dim3 grid, hipStream_t st, const FoldArgs& a, const double* W, TG* g) {
    if (mode == FOLD_SCALAR) hipLaunchKernelGGL((k_fold<TG, FOLD_SCALAR>), grid, dim3(HBLK), 0, st, a, W, g);
    else if (mode == FOLD_GROUPS) hipLaunchKernelGGL((k_fold<TG, FOLD_GROUPS>), grid, dim3(HBLK), 0, st, a, W, g);
    else hipLaunchKernelGGL((k_fold<TG, FOLD_NOISE>), grid, dim3(HBLK), 0, st, a, W, g);
}

// what the three entry points refuse alike once their own arguments are through, and the one launch
int fold_launch(const char* fn, int mode, const FoldArgs& a, const double* W, void* grad, int gdtype, int C, void* stream) {
    if (C < 1 || C > 65535 || a.p < 1 || a.p < a.G) {
        if (mode == FOLD_SCALAR) qn_set_error("%s: bad size (1 <= C = %d <= 65535, p = %lld >= 1)", fn, C, (long long)a.p);
        else qn_set_error("%s: bad size (1 <= C = %d <= 65535, p = %lld >= max(1, G = %d))", fn, C, (long long)a.p, a.G);
        return QN_EINVAL;
    }
    if (a.sse && a.sse_stride < 1) {
        qn_set_error("%s: sse_stride = %d must be >= 1", fn, a.sse_stride);
        return QN_EINVAL;
    }
    if (grad && gdtype != QN_F64 && gdtype != QN_F32) {
        qn_set_error("%s: gdtype = %d is neither QN_F64 nor QN_F32", fn, gdtype);
        return QN_EINVAL;
    }
    const dim3 grid(grad ? hmc_parts(a.p) : 1, C);
    hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (grad && gdtype == QN_F32) fold_go(mode, grid, st, a, W, static_cast<float*>(grad));
    else fold_go(mode, grid, st, a, W, static_cast<double*>(grad));
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}

bool fold_has_output(const char* fn, const char* into, const void* grad, const void* sse) {
    if (!grad && !sse) qn_set_error("%s: grad and sse are both NULL (nothing to fold %s)", fn, into);
    return grad || sse;
}

}  // namespace

extern "C" int qn_prior_fold(const double* W, double lam, double c0, void* grad, int gdtype, double* sse, int sse_stride, int C,
                             int64_t p, void* stream) {
    if (!W) {
        qn_set_error("qn_prior_fold: W is NULL");
        return QN_EINVAL;
    }
    if (!fold_has_output("qn_prior_fold", "the prior into", grad, sse)) return QN_EINVAL;
    if (!(lam > 0.0) || !std::isfinite(lam) || !std::isfinite(c0)) {
        qn_set_error("qn_prior_fold: lam = %g must be > 0 and finite, c0 = %g finite", lam, c0);
        return QN_EINVAL;
    }
    return fold_launch("qn_prior_fold", FOLD_SCALAR, FoldArgs{nullptr, nullptr, nullptr, nullptr, nullptr, 1, lam, c0, sse, sse_stride, p}, W,
                       grad, gdtype, C, stream);
}

extern "C" int qn_prior_fold_g(const double* W, const double* lam, const double* c0, const int64_t* seg, int G, void* grad,
                               int gdtype, double* sse, int sse_stride, int C, int64_t p, void* stream) {
    if (!W || !lam || !c0 || !seg) {
        qn_set_error("qn_prior_fold_g: W, lam, c0 or seg is NULL");
        return QN_EINVAL;
    }
    if (!fold_has_output("qn_prior_fold_g", "the prior into", grad, sse)) return QN_EINVAL;
    if (G < 1 || G > GMAX) {
        qn_set_error("qn_prior_fold_g: G = %d groups, 1 <= G <= %d", G, GMAX);
        return QN_EINVAL;
    }
    return fold_launch("qn_prior_fold_g", FOLD_GROUPS, FoldArgs{nullptr, nullptr, lam, c0, seg, G, 0.0, 0.0, sse, sse_stride, p}, W, grad,
                       gdtype, C, stream);
}

extern "C" int qn_noise_fold(const double* W, const double* kappa, const double* d0, const double* lam, const double* c0,
                             const int64_t* seg, int G, void* grad, int gdtype, double* sse, int sse_stride, int C, int64_t p,
                             void* stream) {
    if (!W || !kappa || !d0) {
        qn_set_error("qn_noise_fold: W, kappa or d0 is NULL");
        return QN_EINVAL;
    }
    if (G < 0 || G > GMAX) {
        qn_set_error("qn_noise_fold: G = %d groups, 0 <= G <= %d", G, GMAX);
        return QN_EINVAL;
    }
    if (G > 0 && (!lam || !c0 || !seg)) {
        qn_set_error("qn_noise_fold: lam, c0 or seg is NULL with G = %d groups (G = 0: no weight prior)", G);
        return QN_EINVAL;
    }
    if (!fold_has_output("qn_noise_fold", "into", grad, sse)) return QN_EINVAL;
    return fold_launch("qn_noise_fold", FOLD_NOISE, FoldArgs{kappa, d0, lam, c0, seg, G, 0.0, 0.0, sse, sse_stride, p}, W, grad, gdtype, C,
                       stream);
}
