// Per-data-row forward / backward passes shared by the curvature kernels (qn_curv.hip) and the linearised predictive
// (qn_glm.hip), float64.  Notation as in qn_curv.hip: ~in_i = [in_i; 1] input of Linear layer i, z_i = W_i in_i + b_i,
// g_i = backward signal at z_i;  d(.)/dW_i[a][b] = g_i[a] ~in_i[b].
#pragma once
#include "qn_common.h"
#include "qn_math.h"

namespace {

struct CurvArgs {
    int L, act, hb, d, o;
    int64_t p;
    int dims[QN_MAX_LAYERS + 1];
    int64_t offW[QN_MAX_LAYERS], offB[QN_MAX_LAYERS];
    int offIN[QN_MAX_LAYERS];   // column of ~in_i in a row of IN (width EI)
    int offG[QN_MAX_LAYERS];    // column of layer i's units in a row of G / SP / S2U / ZG / AD (width D)
    int EI, D, RT;
};

typedef double dv4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ dv4 mfma64(double a, double b, dv4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// flat index of parameter (layer i, unit a, input slot b); b == dims[i] is the bias slot
__device__ __forceinline__ int64_t param_index(const CurvArgs& g, int i, int a, int b) {
    return b < g.dims[i] ? g.offW[i] + (int64_t)a * g.dims[i] + b : g.offB[i] + a;
}

// the descriptor's shape and the column offsets of the per-row arrays (everything of CurvArgs but RT)
inline void curv_fill_dims(const qn_desc* d, CurvArgs* g) {
    g->L = d->nlayers;
    g->act = d->act;
    g->hb = d->has_bias;
    g->d = d->dims[0];
    g->o = d->dims[d->nlayers];
    g->p = d->p;
    int ei = 0, dd = 0;
    for (int i = 0; i <= d->nlayers; ++i) g->dims[i] = d->dims[i];
    for (int i = 0; i < d->nlayers; ++i) {
        g->offW[i] = d->offW[i];
        g->offB[i] = d->offB[i];
        g->offIN[i] = ei;
        g->offG[i] = dd;
        ei += d->dims[i] + d->has_bias;
        dd += d->dims[i + 1];
    }
    g->EI = ei;
    g->D = dd;
}

// forward of data row `row`: in [EI] := ~in_i of every layer, f [o] := z_{L-1}; with CURV2 also sp [D] := act'(z_i) and
// s2 [D] := act''(z_i) (1 and 0 on the output layer)
template <bool CURV2>
__device__ __forceinline__ void curv_row_forward(const CurvArgs& g, const double* __restrict__ W, const double* __restrict__ X,
                                                 int64_t row, double* in, double* sp, double* s2, double* f) {
    for (int k = 0; k < g.d; ++k) in[g.offIN[0] + k] = X[row * g.d + k];
    if (g.hb) in[g.offIN[0] + g.d] = 1.0;
    for (int i = 0; i < g.L; ++i) {
        const int hi = g.dims[i], ho = g.dims[i + 1];
        const double* Wl = W + g.offW[i];
        const double* x = in + g.offIN[i];
        for (int j = 0; j < ho; ++j) {
            double z = 0.0;
            for (int k = 0; k < hi; ++k) z = fma(Wl[(int64_t)j * hi + k], x[k], z);
            if (g.hb) z += W[g.offB[i] + j];
            if (i + 1 < g.L) {
                double a, d1, d2;
                if (g.act == QN_ACT_TANH) {
                    a = qn_tanh_f64(z);
                    d1 = 1.0 - a * a;
                    d2 = -2.0 * a * d1;
                } else if (g.act == QN_ACT_RELU) {
                    a = qn_relu<double>(z);
                    d1 = a <= 0.0 ? 0.0 : 1.0;      // the select of the gradient kernels (qn_act_bwd)
                    d2 = 0.0;
                } else {
                    a = z; d1 = 1.0; d2 = 0.0;
                }
                in[g.offIN[i + 1] + j] = a;
                if (CURV2) {
                    sp[g.offG[i] + j] = d1;
                    s2[g.offG[i] + j] = d2;         // times u_i in the backward pass
                }
            } else {
                f[j] = z;
                if (CURV2) {
                    sp[g.offG[i] + j] = 1.0;
                    s2[g.offG[i] + j] = 0.0;
                }
            }
        }
        if (i + 1 < g.L && g.hb) in[g.offIN[i + 1] + ho] = 1.0;
    }
}

// backward from the seed already in gr [offG[L-1] ..]: gr [D] := g_i of every layer; with CURV2 s2 *= u_i
template <bool CURV2>
__device__ __forceinline__ void curv_row_backward(const CurvArgs& g, const double* __restrict__ W, const double* in, double* gr,
                                                  double* s2) {
    for (int i = g.L - 2; i >= 0; --i) {
        const int hi = g.dims[i + 1], ho = g.dims[i + 2];
        const double* Wn = W + g.offW[i + 1];
        const double* gn = gr + g.offG[i + 1];
        for (int c = 0; c < hi; ++c) {
            double u = 0.0;
            for (int j = 0; j < ho; ++j) u = fma(Wn[(int64_t)j * hi + c], gn[j], u);
            const int col = g.offG[i] + c;
            gr[col] = qn_act_bwd<double>(u, in[g.offIN[i + 1] + c], g.act);
            if (CURV2) s2[col] *= u;
        }
    }
}

// ---- Jacobian rows of a tile of RT data rows for the members blockIdx.y: forward, then one backward per output k started
// from the unit vector e_k.  IN [members][RT][EI]: ~in_i;  GK [members][o][RT][D]: g^k_i, so that
// d f_k(x_n) / dW_i[a][b] = GK[k][n][offG[i] + a] * IN[n][offIN[i] + b].  Rows past nrows are zero in both.  `rows`
// (optional, [members][rows_stride]) picks the data rows; mean_out (optional, [members][mean_stride][o]) receives f.
__global__ __launch_bounds__(256) void k_jac_rows(CurvArgs g, const double* __restrict__ W, const double* __restrict__ X,
                                                  const int32_t* __restrict__ rows, int64_t rows_stride, int n0, int nrows,
                                                  double* __restrict__ IN, double* __restrict__ GK,
                                                  double* __restrict__ mean_out, int64_t mean_stride) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= g.RT) return;
    const int mb = blockIdx.y;
    double* in = IN + ((size_t)mb * g.RT + n) * g.EI;
    double* gk = GK + (size_t)mb * g.o * g.RT * g.D + (size_t)n * g.D;
    const size_t kstride = (size_t)g.RT * g.D;
    if (n >= nrows) {
        for (int j = 0; j < g.EI; ++j) in[j] = 0.0;
        for (int k = 0; k < g.o; ++k)
            for (int j = 0; j < g.D; ++j) gk[k * kstride + j] = 0.0;
        return;
    }
    const double* Wb = W + (int64_t)mb * g.p;
    const int64_t row = rows ? rows[mb * rows_stride + n0 + n] : (int64_t)(n0 + n);
    // f lands in the output-layer slots of g^0 and is replaced by the seed afterwards
    double* f = gk + g.offG[g.L - 1];
    curv_row_forward<false>(g, Wb, X, row, in, nullptr, nullptr, f);
    if (mean_out)
        for (int j = 0; j < g.o; ++j) mean_out[((int64_t)mb * mean_stride + n0 + n) * g.o + j] = f[j];
    for (int k = 0; k < g.o; ++k) {
        double* gr = gk + k * kstride;
        for (int j = 0; j < g.o; ++j) gr[g.offG[g.L - 1] + j] = j == k ? 1.0 : 0.0;
        curv_row_backward<false>(g, Wb, in, gr, nullptr);
    }
}

}  // namespace
