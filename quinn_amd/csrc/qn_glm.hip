// Linearised ("GLM") predictive of a Gaussian weight posterior N(W_b, Sigma_b) of a batched MLP, float64:
//   mean[b][n] = f_{W_b}(x_n),   cov[b][n][k][l] = J_nk Sigma_b J_nl^T,   J_nk = d f_k(x_n) / dW  (flat order of p_flatten).
//
// J is never stored.  k_jac_rows (qn_curv_rows.h, shared with the Gauss-Newton curvature) leaves, per query row n of a tile,
// the layer inputs IN[n][.] and one backward signal per output GK[k][n][.]; a parameter P = (layer i, unit a, slot b) has
//   J_nk[P] = GK[k][n][gcol(P)] * IN[n][icol(P)],   gcol = offG[i] + a,  icol = offIN[i] + b   (bias: the stored 1).
// The (gcol, icol) pairs of all P are tabulated once per call (k_glm_table).
//
// COV_FULL.  Rows r = n * o + k.  One block owns GLM_RP = 64 rows and ALL columns: for every tile of 64 columns Q it runs the GEMM
// T[r][Q] = sum_P J[r][P] Sigma[P][Q] over all P on v_mfma_f64_16x16x4_f64, chunks of GLM_KC = 32 values of P staged through LDS
// (the A chunk formed from the table and the two per-row arrays, the Sigma chunk copied), each wave 16 rows x 64 columns; the
// epilogue multiplies the accumulator tile by J[(n, l)][Q] for l >= k, sums over the 16 columns a lane group holds with a fixed
// butterfly and adds the result to cov[n][k][l] -- the same lane for the same row at every column tile, in column order: no
// atomics, no dependence on the grid.  After the last column tile the lane copies cov[n][k][l] to cov[n][l][k].
// COV_DIAG.  One wave per (n, k <= l): sum_P J_nk[P] sigma[P] J_nl[P], lanes strided over P, fixed butterfly.
#include "qn_curv_rows.h"
#include "qn_host_args.h"

namespace {

constexpr int GLM_MAX_P = 16384;      // COV_FULL: Sigma is p x p doubles per member
constexpr int GLM_RT = 4096;          // query rows per tile (bounds the workspace)
constexpr int GLM_RP = 64;            // rows (n, k) per block
constexpr int GLM_KC = 32;            // values of P per LDS chunk
constexpr int GLM_AS = GLM_KC + 2;    // A chunk [RP][AS]: lane (q, cl) reads row cl, column 4 s + q; 68 dwords per row puts the 32 lanes
                                      // of a ds_read_b64 group on 64 distinct banks
constexpr int GLM_BS = 64 + 16;       // Sigma chunk [KC][BS]: lane (q, cl) reads row 4 s + q, column 16 ct + cl; 160 dwords per row

__global__ __launch_bounds__(256) void k_glm_table(CurvArgs g, int2* __restrict__ tab) {
    const int64_t P = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (P >= g.p) return;
    for (int i = 0; i < g.L; ++i) {
        const int64_t nw = (int64_t)g.dims[i] * g.dims[i + 1];
        if (P >= g.offW[i] && P < g.offW[i] + nw) {
            const int64_t r = P - g.offW[i];
            tab[P] = make_int2(g.offG[i] + (int)(r / g.dims[i]), g.offIN[i] + (int)(r % g.dims[i]));
            return;
        }
        if (g.hb && P >= g.offB[i] && P < g.offB[i] + g.dims[i + 1]) {
            tab[P] = make_int2(g.offG[i] + (int)(P - g.offB[i]), g.offIN[i] + g.dims[i]);
            return;
        }
    }
}

// grid (row panels of the tile, members).  IN [members][RT][EI], GK [members][o][RT][D]; Sigma [members][p][p];
// cov [members][N][o][o]; the tile holds query rows n0 .. n0 + nrows - 1.
__global__ __launch_bounds__(256) void k_glm_full(CurvArgs g, const int2* __restrict__ tab, const double* __restrict__ IN,
                                                  const double* __restrict__ GK, const double* __restrict__ Sigma, int n0,
                                                  int nrows, int N, double* __restrict__ cov) {
    __shared__ double As[GLM_RP * GLM_AS];
    __shared__ double Bs[GLM_KC * GLM_BS];
    __shared__ int rowN[GLM_RP], rowK[GLM_RP];            // query row within the tile (-1: past the end) and output of a panel row
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, q = lane >> 4, cl = lane & 15;
    const int mb = blockIdx.y, o = g.o;
    const int64_t P = g.p;
    const int r0 = blockIdx.x * GLM_RP;
    const double* INb = IN + (size_t)mb * g.RT * g.EI;
    const double* GKb = GK + (size_t)mb * o * g.RT * g.D;
    const size_t kstride = (size_t)g.RT * g.D;
    const double* Sb = Sigma + (size_t)mb * P * P;
    double* covb = cov + (size_t)mb * N * o * o;
    if (tid < GLM_RP) {
        const int r = r0 + tid;
        const bool live = r < nrows * o;
        rowN[tid] = live ? r / o : -1;
        rowK[tid] = live ? r % o : 0;
    }
    __syncthreads();
    // the rows this lane's accumulator registers belong to: panel row 16 wv + q + 4 r
    int myN[4], myK[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        myN[r] = rowN[16 * wv + q + 4 * r];
        myK[r] = rowK[16 * wv + q + 4 * r];
    }
    const int nqt = (int)((P + 63) / 64);
    for (int qt = 0; qt < nqt; ++qt) {
        const int64_t Q0 = (int64_t)qt * 64;
        dv4 acc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = (dv4){0.0, 0.0, 0.0, 0.0};
        for (int64_t P0 = 0; P0 < P; P0 += GLM_KC) {
            __syncthreads();
            // A chunk: wave wv forms its own 16 rows; two rows per pass, lanes along P
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int rr = 16 * wv + 2 * it + (lane >> 5), kk = lane & 31;
                const int64_t Pc = P0 + kk;
                const int n = rowN[rr];
                double v = 0.0;
                if (n >= 0 && Pc < P) {
                    const int2 t = tab[Pc];
                    v = GKb[rowK[rr] * kstride + (size_t)n * g.D + t.x] * INb[(size_t)n * g.EI + t.y];
                }
                As[rr * GLM_AS + kk] = v;
            }
            // Sigma chunk: rows P0 .. P0 + 31, columns Q0 .. Q0 + 63
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int kk = 4 * it + wv;
                const int64_t Pc = P0 + kk, Qc = Q0 + lane;
                Bs[kk * GLM_BS + lane] = (Pc < P && Qc < P) ? Sb[Pc * P + Qc] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < GLM_KC / 4; ++s) {
                const double a = As[(16 * wv + cl) * GLM_AS + 4 * s + q];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma64(a, Bs[(4 * s + q) * GLM_BS + 16 * ct + cl], acc[ct]);
            }
        }
        // epilogue: cov[n][k][l] += sum over this tile's columns of T[(n, k)][Q] J[(n, l)][Q], l >= k
        int2 tq[4];
        bool ql[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int64_t Qc = Q0 + 16 * ct + cl;
            ql[ct] = Qc < P;
            tq[ct] = ql[ct] ? tab[Qc] : make_int2(0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = max(myN[r], 0);               // every lane runs the same loop (the butterfly needs all 64); only the store is
            const bool rlive = myN[r] >= 0;             // predicated
            const double* inr = INb + (size_t)n * g.EI;
            double tin[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) tin[ct] = ql[ct] ? acc[ct][r] * inr[tq[ct].y] : 0.0;
            for (int l = 0; l < o; ++l) {
                const double* gl = GKb + l * kstride + (size_t)n * g.D;
                double v = 0.0;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) v = fma(tin[ct], ql[ct] ? gl[tq[ct].x] : 0.0, v);
                v += __shfl_xor(v, 1);
                v += __shfl_xor(v, 2);
                v += __shfl_xor(v, 4);
                v += __shfl_xor(v, 8);
                if (cl == 0 && rlive && l >= myK[r]) {
                    double* c = covb + ((size_t)(n0 + n) * o + myK[r]) * o + l;
                    const double tot = qt == 0 ? v : *c + v;
                    *c = tot;
                    if (qt == nqt - 1 && l != myK[r]) covb[((size_t)(n0 + n) * o + l) * o + myK[r]] = tot;
                }
            }
        }
    }
}

// grid (items of the tile / 4, members), one wave per item (n, pair k <= l); sig [members][p]
__global__ __launch_bounds__(256) void k_glm_diag(CurvArgs g, const int2* __restrict__ tab, const double* __restrict__ IN,
                                                  const double* __restrict__ GK, const double* __restrict__ sig, int n0, int nrows,
                                                  int N, double* __restrict__ cov) {
    const int lane = threadIdx.x & 63, o = g.o, npair = o * (o + 1) / 2;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (int64_t)nrows * npair) return;          // whole waves leave together
    const int n = (int)(item / npair);
    int pr = (int)(item % npair), k = 0;
    while (pr >= o - k) { pr -= o - k; ++k; }
    const int l = k + pr;
    const int mb = blockIdx.y;
    const int64_t P = g.p;
    const size_t kstride = (size_t)g.RT * g.D;
    const double* inr = IN + ((size_t)mb * g.RT + n) * g.EI;
    const double* gk = GK + (size_t)mb * o * kstride + k * kstride + (size_t)n * g.D;
    const double* gl = GK + (size_t)mb * o * kstride + l * kstride + (size_t)n * g.D;
    const double* sb = sig + (size_t)mb * P;
    double v = 0.0;
    for (int64_t Pc = lane; Pc < P; Pc += 64) {
        const int2 t = tab[Pc];
        const double iv = inr[t.y];
        v = fma(gk[t.x] * iv * sb[Pc], gl[t.x] * iv, v);
    }
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    if (lane == 0) {
        double* cb = cov + ((size_t)mb * N + n0 + n) * o * o;
        cb[k * o + l] = v;
        cb[l * o + k] = v;
    }
}

bool glm_args(const qn_desc* d, int cov_kind, int B, int N, CurvArgs* g, const char* who) {
    if (!qn_check_mlp_desc(d, who, "the linearised predictive")) return false;
    if (cov_kind != QN_GLM_COV_FULL && cov_kind != QN_GLM_COV_DIAG) {
        qn_set_error("%s: cov_kind must be QN_GLM_COV_FULL (0) or QN_GLM_COV_DIAG (1), got %d", who, cov_kind);
        return false;
    }
    if (cov_kind == QN_GLM_COV_FULL && d->p > GLM_MAX_P) {
        qn_set_error("%s: a full covariance is refused for p = %lld > %d parameters (%.1f GB per member); use QN_GLM_COV_DIAG",
                     who, (long long)d->p, GLM_MAX_P, (double)d->p * (double)d->p * 8e-9);
        return false;
    }
    if (!qn_check_members(B, who)) return false;
    if (N <= 0) {
        qn_set_error("%s: need N >= 1 query rows", who);
        return false;
    }
    curv_fill_dims(d, g);
    g->RT = std::min(GLM_RT, (N + 3) / 4 * 4);
    return true;
}

struct GlmLayout { size_t tab, in, gk, total; };

GlmLayout glm_layout(const CurvArgs& g, int B) {
    GlmLayout l;
    qn_ws_carver c;
    l.tab = c.take((size_t)g.p * sizeof(int2));
    l.in = c.take_doubles((size_t)B * g.RT * g.EI);
    l.gk = c.take_doubles((size_t)B * g.o * g.RT * g.D);
    l.total = c.total;
    return l;
}

}  // namespace

extern "C" size_t qn_glm_workspace_bytes(const qn_desc* d, int cov_kind, int B, int N) {
    CurvArgs g;
    if (!glm_args(d, cov_kind, B, N, &g, "qn_glm_workspace_bytes")) return 0;
    return glm_layout(g, B).total;
}

extern "C" int qn_mlp_glm_predict(const qn_desc* d, int cov_kind, const double* W, const double* X, const double* Sigma, int B,
                                  int N, double* mean_out, double* cov_out, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    CurvArgs g;
    if (!glm_args(d, cov_kind, B, N, &g, "qn_mlp_glm_predict")) return QN_EINVAL;
    if (!W || !X || !Sigma || !mean_out || !cov_out) {
        qn_set_error("qn_mlp_glm_predict: need non-NULL W, X, Sigma, mean_out, cov_out");
        return QN_EINVAL;
    }
    const GlmLayout l = glm_layout(g, B);
    if (!qn_check_workspace(workspace, workspace_bytes, l.total, "qn_mlp_glm_predict")) return QN_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int2* tab = qn_ws_at<int2>(workspace, l.tab);
    double* IN = qn_ws_at(workspace, l.in);
    double* GK = qn_ws_at(workspace, l.gk);
    hipLaunchKernelGGL(k_glm_table, dim3((unsigned)((g.p + 255) / 256)), dim3(256), 0, st, g, tab);
    QN_HIP_CHECK(hipGetLastError());
    const int npair = g.o * (g.o + 1) / 2;
    for (int n0 = 0; n0 < N; n0 += g.RT) {
        const int nrows = std::min(g.RT, N - n0);
        hipLaunchKernelGGL(k_jac_rows, dim3((g.RT + 255) / 256, B), dim3(256), 0, st, g, W, X, (const int32_t*)nullptr,
                           (int64_t)0, n0, nrows, IN, GK, mean_out, (int64_t)N);
        QN_HIP_CHECK(hipGetLastError());
        if (cov_kind == QN_GLM_COV_FULL) {
            const int panels = (int)(((int64_t)nrows * g.o + GLM_RP - 1) / GLM_RP);
            hipLaunchKernelGGL(k_glm_full, dim3(panels, B), dim3(256), 0, st, g, tab, IN, GK, Sigma, n0, nrows, N, cov_out);
        } else {
            const int64_t items = (int64_t)nrows * npair;
            hipLaunchKernelGGL(k_glm_diag, dim3((unsigned)((items + 3) / 4), B), dim3(256), 0, st, g, tab, IN, GK, Sigma, n0,
                               nrows, N, cov_out);
        }
        QN_HIP_CHECK(hipGetLastError());
    }
    return QN_OK;
}
