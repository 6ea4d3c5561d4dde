// Curvature of the data term of a batched MLP (the Laplace approximation, reference quinn/solvers/nn_laplace.py:76-122,
// quinn/nns/nnwrap.py:153-229), float64 only:
//   QN_CURV_HESS_FULL  out[b] = d2/dW2 sum_n |r_bn|^2 / 2                    [B, p, p], both triangles, exactly symmetric
//   QN_CURV_EF_DIAG    out[b][j] = (1/Nb) sum_n (d/dW_j |r_bn|^2 / 2)^2        [B, p]
//   QN_CURV_GGN_FULL   out[b] = sum_n sum_k J_nk^T J_nk,  J_nk = d f_k(x_n)/dW   [B, p, p], both triangles, exactly symmetric
//   QN_CURV_GGN_DIAG   out[b][j] = sum_n sum_k J_nk[j]^2  (a sum, not a mean)    [B, p]
//
// Notation (Linear layer i = 0..L-1, L = nlayers): in_i = input of layer i (in_0 = x), ~in_i = [in_i; 1] (bias slot if any),
// z_i = W_i in_i + b_i, in_{i+1} = act(z_i), f = z_{L-1}, r = f - y.  Backward: g_{L-1} = r, u_i = W_{i+1}^T g_{i+1},
// g_i = act'(z_i) o u_i; d(|r|^2/2)/dW_i[a][b] = g_i[a] ~in_i[b].
//
// FULL.  A weight W_i[a][b] moves every downstream quantity exactly ~in_i[b] times as much as the bias b_i[a] does, so only the
// unit directions dz_i = e_a (one per unit of every layer: D = sum of the layer widths) need tangents.  Along direction (i, a):
//   forward   dz_i = e_a,  din_{k+1} = act'(z_k) o dz_k,  dz_{k+1} = W_{k+1} din_{k+1}
//   backward  dg_{L-1} = dz_{L-1},  dg_k = act''(z_k) o dz_k o u_k + act'(z_k) o (W_{k+1}^T dg_{k+1})      (k >= i)
//   H[(i,a,b),(m,c,d)] = sum_n ~in_i[b] ( dg_m[c] ~in_m[d] + g_m[c] d~in_m[d] )    for m >= i  (d~in_i = 0, bias slot 0)
// and the blocks m < i by symmetry.  Per direction and column layer m that is a GEMM over the data rows whose A operand
// ~in_i[b][n] is shared by all directions of layer i and whose B operand is formed on the fly from four per-row vectors; it
// runs on v_mfma_f64_16x16x4_f64.  Only the entries with row parameter <= column parameter are assembled; a last kernel
// copies them to the lower triangle, so the result is symmetric bit for bit.
//
// GGN.  With g^k the backward pass started from the output unit vector e_k (k_jac_rows, qn_curv_rows.h),
//   G[(i,a,b),(m,c,d)] = sum_n ~in_i[b] (sum_k g^k_i[a] g^k_m[c]) ~in_m[d]:
// the FULL assembly with a B operand formed from the per-output signals (no tangents); its diagonal is the DIAG GEMM on
// sum_k (g^k o g^k) without the division.
//
// DIAG.  D_W = (g o g)^T (~in o ~in) / Nb per layer: the weight-gradient GEMM on squared operands, also on the f64 MFMA.
//
// Rows are processed in tiles of RT (workspace-bounded); a member's tiles are added into `out` one after another in a fixed
// order, members one after another: no atomics, two calls give the same bits.  Rows past the end of a tile are zero in every
// per-row array (so they add exact zeros).
#include "qn_curv_rows.h"
#include "qn_host_args.h"

namespace {

constexpr int CURV_MAX_P = 16384;          // FULL: p x p doubles per member (2.1 GB at the cap)
constexpr size_t CURV_TANGENT_BUDGET = size_t(1) << 29;   // bytes of tangents per row tile
constexpr int CURV_RT_MAX = 1024;
constexpr int CURV_RT_GGN = 4096;          // GGN kinds: no tangents, the row tile is bounded by o * RT * D doubles only

// ---- per data row of the tile: forward and backward, stored row-major ([n][column])
//   IN [RT][EI]: ~in_i;  G [RT][D]: g_i;  SP [RT][D]: act'(z_i);  S2U [RT][D]: act''(z_i) u_i
__global__ __launch_bounds__(256) void k_curv_rows(CurvArgs g, const double* __restrict__ W, const double* __restrict__ X,
                                                   const double* __restrict__ Y, const int32_t* __restrict__ rows, int n0,
                                                   int nrows, double* __restrict__ IN, double* __restrict__ G,
                                                   double* __restrict__ SP, double* __restrict__ S2U) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= g.RT) return;
    double* in = IN + (size_t)n * g.EI;
    double* gr = G + (size_t)n * g.D;
    double* sp = SP + (size_t)n * g.D;
    double* s2 = S2U + (size_t)n * g.D;
    if (n >= nrows) {
        for (int j = 0; j < g.EI; ++j) in[j] = 0.0;
        for (int j = 0; j < g.D; ++j) { gr[j] = 0.0; sp[j] = 0.0; s2[j] = 0.0; }
        return;
    }
    const int64_t row = rows ? rows[n0 + n] : (int64_t)(n0 + n);
    double* f = gr + g.offG[g.L - 1];
    curv_row_forward<true>(g, W, X, row, in, sp, s2, f);
    for (int j = 0; j < g.o; ++j) f[j] = f[j] - Y[row * g.o + j];
    curv_row_backward<true>(g, W, in, gr, s2);
}

// ---- tangents of the directions of layer i, one thread per (direction a = blockIdx.y, row n):
//   ZG [D][RT][D]: dz_k, overwritten in place by dg_k (k >= i);   AD [D][RT][D]: din_{k+1} = act'(z_k) dz_k at column offG[k]
__global__ __launch_bounds__(64) void k_curv_tangent(CurvArgs g, const double* __restrict__ W, int i,
                                                     const double* __restrict__ SP, const double* __restrict__ S2U,
                                                     double* __restrict__ ZG, double* __restrict__ AD) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= g.RT) return;
    const int a = blockIdx.y;
    const size_t t = (size_t)g.offG[i] + a;
    double* zg = ZG + (t * g.RT + n) * g.D;
    double* ad = AD + (t * g.RT + n) * g.D;
    const double* sp = SP + (size_t)n * g.D;
    const double* s2 = S2U + (size_t)n * g.D;
    for (int c = 0; c < g.dims[i + 1]; ++c) zg[g.offG[i] + c] = c == a ? 1.0 : 0.0;
    for (int k = i; k + 1 < g.L; ++k) {
        const int hi = g.dims[k + 1], ho = g.dims[k + 2];
        const int ok = g.offG[k], on = g.offG[k + 1];
        for (int c = 0; c < hi; ++c) ad[ok + c] = sp[ok + c] * zg[ok + c];
        const double* Wn = W + g.offW[k + 1];
        int j = 0;
        for (; j + 4 <= ho; j += 4) {
            double s0 = 0.0, s1 = 0.0, s2v = 0.0, s3 = 0.0;
            for (int c = 0; c < hi; ++c) {
                const double v = ad[ok + c];
                s0 = fma(Wn[(int64_t)(j + 0) * hi + c], v, s0);
                s1 = fma(Wn[(int64_t)(j + 1) * hi + c], v, s1);
                s2v = fma(Wn[(int64_t)(j + 2) * hi + c], v, s2v);
                s3 = fma(Wn[(int64_t)(j + 3) * hi + c], v, s3);
            }
            zg[on + j] = s0; zg[on + j + 1] = s1; zg[on + j + 2] = s2v; zg[on + j + 3] = s3;
        }
        for (; j < ho; ++j) {
            double s = 0.0;
            for (int c = 0; c < hi; ++c) s = fma(Wn[(int64_t)j * hi + c], ad[ok + c], s);
            zg[on + j] = s;
        }
    }
    for (int k = g.L - 2; k >= i; --k) {
        const int hi = g.dims[k + 1], ho = g.dims[k + 2];
        const int ok = g.offG[k], on = g.offG[k + 1];
        const double* Wn = W + g.offW[k + 1];
        int c = 0;
        for (; c + 4 <= hi; c += 4) {
            double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
            for (int j = 0; j < ho; ++j) {
                const double e = zg[on + j];
                const double* w = Wn + (int64_t)j * hi + c;
                v0 = fma(w[0], e, v0); v1 = fma(w[1], e, v1); v2 = fma(w[2], e, v2); v3 = fma(w[3], e, v3);
            }
            zg[ok + c + 0] = fma(s2[ok + c + 0], zg[ok + c + 0], sp[ok + c + 0] * v0);
            zg[ok + c + 1] = fma(s2[ok + c + 1], zg[ok + c + 1], sp[ok + c + 1] * v1);
            zg[ok + c + 2] = fma(s2[ok + c + 2], zg[ok + c + 2], sp[ok + c + 2] * v2);
            zg[ok + c + 3] = fma(s2[ok + c + 3], zg[ok + c + 3], sp[ok + c + 3] * v3);
        }
        for (; c < hi; ++c) {
            double v = 0.0;
            for (int j = 0; j < ho; ++j) v = fma(Wn[(int64_t)j * hi + c], zg[on + j], v);
            zg[ok + c] = fma(s2[ok + c], zg[ok + c], sp[ok + c] * v);
        }
    }
}

// ---- FULL assembly of the block (row layer i, column layer m >= i) over the rows of one tile.
// One wave = direction a x (64 b) x (4 c) x (16 d): 4 x 4 accumulator tiles of v_mfma_f64_16x16x4_f64, K = rows, 4 per step.
// Operand maps (one f64 per lane, q = lane >> 4, cl = lane & 15): A[row cl][k q] = ~in_i[b0 + 16 mt + cl] of row n0 + q;
// B[k q][col cl] = dg_m[c] ~in_m[d0 + cl] + g_m[c] d~in_m[d0 + cl] of that row;  C/D reg r = row q + 4 r, col cl.
// GGN: the same GEMM with B[k q][col cl] = (sum_k g^k_i[a] g^k_m[c]) ~in_m[d0 + cl]: the sum over the outputs is folded into the
// operand, so K stays the rows; G is then GK [o][RT][D] of k_jac_rows and ZG / AD are not read.
template <bool GGN>
__global__ __launch_bounds__(256) void k_curv_full(CurvArgs g, int i, int m, const double* __restrict__ IN,
                                                   const double* __restrict__ G, const double* __restrict__ ZG,
                                                   const double* __restrict__ AD, double* __restrict__ out, int accumulate) {
    const int lane = threadIdx.x & 63, q = lane >> 4, cl = lane & 15;
    const int ei = g.dims[i] + g.hb, em = g.dims[m] + g.hb, hm = g.dims[m + 1];
    const int nbch = (ei + 63) / 64, ncg = (hm + 3) / 4, ndt = (em + 15) / 16;
    int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int items = g.dims[i + 1] * nbch * ncg * ndt;
    if (w >= items) return;
    const int dt = w % ndt; w /= ndt;
    const int cg = w % ncg; w /= ncg;
    const int bch = w % nbch;
    const int a = w / nbch;
    const int b0 = bch * 64, c0 = cg * 4, d0 = dt * 16;
    const int mtn = min(4, (ei - b0 + 15) / 16), ncn = min(4, hm - c0);
    const size_t t = (size_t)g.offG[i] + a;
    const int dcol = d0 + cl;
    const bool dlive = dcol < em, alive = m > i && dcol < g.dims[m];
    const int bl[4] = {min(b0 + cl, ei - 1), min(b0 + 16 + cl, ei - 1), min(b0 + 32 + cl, ei - 1), min(b0 + 48 + cl, ei - 1)};
    const int cidx[4] = {g.offG[m] + c0, g.offG[m] + min(c0 + 1, hm - 1), g.offG[m] + min(c0 + 2, hm - 1),
                         g.offG[m] + min(c0 + 3, hm - 1)};
    dv4 acc[4][4];
#pragma unroll
    for (int cc = 0; cc < 4; ++cc)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[cc][mt] = (dv4){0.0, 0.0, 0.0, 0.0};
    for (int n0 = 0; n0 < g.RT; n0 += 4) {
        const int n = n0 + q;
        const double* inr = IN + (size_t)n * g.EI;
        const double* gr = G + (size_t)n * g.D;
        const double* zr = GGN ? nullptr : ZG + (t * g.RT + n) * g.D;
        double A[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) A[mt] = inr[g.offIN[i] + bl[mt]];
        const double dv = dlive ? inr[g.offIN[m] + dcol] : 0.0;
        const double adv = !GGN && alive ? AD[(t * g.RT + n) * g.D + g.offG[m - 1] + dcol] : 0.0;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            if (cc < ncn) {
                double Bv;
                if (GGN) {
                    double s = 0.0;
                    for (int k = 0; k < g.o; ++k) {
                        const double* gk = gr + (size_t)k * g.RT * g.D;
                        s = fma(gk[g.offG[i] + a], gk[cidx[cc]], s);
                    }
                    Bv = s * dv;
                } else {
                    Bv = fma(zr[cidx[cc]], dv, gr[cidx[cc]] * adv);
                }
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    if (mt < mtn) acc[cc][mt] = mfma64(A[mt], Bv, acc[cc][mt]);
            }
        }
    }
    const int64_t P = g.p;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        if (cc >= ncn) continue;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            if (mt >= mtn) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = b0 + 16 * mt + q + 4 * r;
                if (b >= ei || !dlive) continue;
                const int64_t rp = param_index(g, i, a, b), cp = param_index(g, m, c0 + cc, dcol);
                if (m == i && rp > cp) continue;
                double* o = out + rp * P + cp;
                *o = accumulate ? *o + acc[cc][mt][r] : acc[cc][mt][r];
            }
        }
    }
}

// ---- lower triangle := upper triangle, 32 x 32 tiles through LDS (only tiles on or below the diagonal)
__global__ __launch_bounds__(256) void k_curv_mirror(double* __restrict__ H, int64_t p) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t R0 = (int64_t)blockIdx.y * 32, C0 = (int64_t)blockIdx.x * 32;    // destination tile rows R0.., cols C0..
    if (C0 > R0) return;
    for (int k = ty; k < 32; k += 8) {                // source: rows C0 + k, cols R0 + tx (upper triangle)
        const int64_t r = C0 + k, c = R0 + tx;
        tile[k][tx] = (r < p && c < p) ? H[r * p + c] : 0.0;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int64_t r = R0 + k, c = C0 + tx;
        if (r < p && c < p && r > c) H[r * p + c] = tile[tx][k];
    }
}

// ---- DIAG of layer i over the rows of one tile: one wave = 64 units a x 16 input slots b, K = rows.
// A[row cl][k q] = g_i[a0 + 16 mt + cl]^2, B[k q][col cl] = ~in_i[b0 + cl]^2; the last tile divides the total by Nb.
// GGN: A = sum_k g^k_i[.]^2 from GK [o][RT][D], and no division (a sum over the rows).
template <bool GGN>
__global__ __launch_bounds__(256) void k_curv_diag(CurvArgs g, int i, const double* __restrict__ IN, const double* __restrict__ G,
                                                   double* __restrict__ out, int accumulate, double div) {
    const int lane = threadIdx.x & 63, q = lane >> 4, cl = lane & 15;
    const int ho = g.dims[i + 1], ei = g.dims[i] + g.hb;
    const int nat = (ho + 63) / 64, nbt = (ei + 15) / 16;
    int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nat * nbt) return;
    const int bt = w % nbt, at = w / nbt;
    const int a0 = at * 64, b = bt * 16 + cl;
    const int mtn = min(4, (ho - a0 + 15) / 16);
    const int al[4] = {min(a0 + cl, ho - 1), min(a0 + 16 + cl, ho - 1), min(a0 + 32 + cl, ho - 1), min(a0 + 48 + cl, ho - 1)};
    const int bc = min(b, ei - 1);
    dv4 acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = (dv4){0.0, 0.0, 0.0, 0.0};
    for (int n0 = 0; n0 < g.RT; n0 += 4) {
        const int n = n0 + q;
        const double v = IN[(size_t)n * g.EI + g.offIN[i] + bc];
        const double Bv = v * v;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            if (mt < mtn) {
                double u2;
                if (GGN) {
                    u2 = 0.0;
                    for (int k = 0; k < g.o; ++k) {
                        const double u = G[((size_t)k * g.RT + n) * g.D + g.offG[i] + al[mt]];
                        u2 = fma(u, u, u2);
                    }
                } else {
                    const double u = G[(size_t)n * g.D + g.offG[i] + al[mt]];
                    u2 = u * u;
                }
                acc[mt] = mfma64(u2, Bv, acc[mt]);
            }
        }
    }
    if (b >= ei) return;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        if (mt >= mtn) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + 16 * mt + q + 4 * r;
            if (a >= ho) continue;
            double* o = out + param_index(g, i, a, b);
            double v = accumulate ? *o + acc[mt][r] : acc[mt][r];
            if (div > 0.0) v = v / div;
            *o = v;
        }
    }
}

bool is_full(int kind) { return kind == QN_CURV_HESS_FULL || kind == QN_CURV_GGN_FULL; }
bool is_ggn(int kind) { return kind == QN_CURV_GGN_FULL || kind == QN_CURV_GGN_DIAG; }

bool fill_args(const qn_desc* d, int kind, int Nb, CurvArgs* g, const char* who) {
    if (!qn_check_mlp_desc(d, who, "the curvature kernels")) return false;
    if (kind != QN_CURV_HESS_FULL && kind != QN_CURV_EF_DIAG && kind != QN_CURV_GGN_FULL && kind != QN_CURV_GGN_DIAG) {
        qn_set_error("%s: kind must be QN_CURV_HESS_FULL (0), QN_CURV_EF_DIAG (1), QN_CURV_GGN_FULL (2) or QN_CURV_GGN_DIAG (3), "
                     "got %d", who, kind);
        return false;
    }
    if (is_full(kind) && d->p > CURV_MAX_P) {
        qn_set_error("%s: the full %s is refused for p = %lld > %d parameters (%.1f GB per member); use %s", who,
                     kind == QN_CURV_HESS_FULL ? "Hessian" : "Gauss-Newton matrix", (long long)d->p, CURV_MAX_P,
                     (double)d->p * (double)d->p * 8e-9, kind == QN_CURV_HESS_FULL ? "QN_CURV_EF_DIAG" : "QN_CURV_GGN_DIAG");
        return false;
    }
    if (Nb <= 0) {
        qn_set_error("%s: need Nb >= 1 rows", who);
        return false;
    }
    curv_fill_dims(d, g);
    const int dd = g->D;
    const int nb4 = (Nb + 3) / 4 * 4;
    int rt;
    if (kind == QN_CURV_HESS_FULL) {
        const size_t per_row = 2 * (size_t)dd * dd * sizeof(double);
        rt = (int)std::min<size_t>((size_t)CURV_RT_MAX, std::max<size_t>(4, CURV_TANGENT_BUDGET / per_row / 4 * 4));
    } else {
        rt = is_ggn(kind) ? CURV_RT_GGN : 4096;
    }
    g->RT = std::min(rt, nb4);
    return true;
}

struct CurvLayout { size_t in, gr, sp, s2, zg, ad, total; };

CurvLayout layout(const CurvArgs& g, int kind) {
    CurvLayout l;
    qn_ws_carver c;
    l.in = c.take_doubles((size_t)g.RT * g.EI);
    l.gr = c.take_doubles((size_t)g.RT * g.D * (is_ggn(kind) ? g.o : 1));      // GGN: GK [o][RT][D]
    l.sp = is_ggn(kind) ? 0 : c.take_doubles((size_t)g.RT * g.D);
    l.s2 = is_ggn(kind) ? 0 : c.take_doubles((size_t)g.RT * g.D);
    l.zg = kind == QN_CURV_HESS_FULL ? c.take_doubles((size_t)g.D * g.RT * g.D) : 0;
    l.ad = kind == QN_CURV_HESS_FULL ? c.take_doubles((size_t)g.D * g.RT * g.D) : 0;
    l.total = c.total;
    return l;
}

}  // namespace

extern "C" size_t qn_curv_workspace_bytes(const qn_desc* d, int kind, int B, int Nb) {
    CurvArgs g;
    if (B <= 0 || !fill_args(d, kind, Nb, &g, "qn_curv_workspace_bytes")) return 0;
    return layout(g, kind).total;
}

extern "C" int qn_mlp_curv(const qn_desc* d, int kind, const double* W, const double* X, const double* Y,
                           const int32_t* row_idx, int B, int N, int Nb, double* out, void* workspace,
                           size_t workspace_bytes, void* stream) {
    CurvArgs g;
    if (!fill_args(d, kind, Nb, &g, "qn_mlp_curv")) return QN_EINVAL;
    if (B <= 0 || N <= 0 || !W || !X || (!Y && !is_ggn(kind)) || !out) {
        qn_set_error("qn_mlp_curv: need B >= 1, N >= 1 and non-NULL W, X, Y (HESS_FULL / EF_DIAG), out");
        return QN_EINVAL;
    }
    if (!qn_check_row_idx(row_idx, N, Nb, "qn_mlp_curv")) return QN_EINVAL;
    const CurvLayout l = layout(g, kind);
    if (!qn_check_workspace(workspace, workspace_bytes, l.total, "qn_mlp_curv")) return QN_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* IN = qn_ws_at(workspace, l.in);
    double* G = qn_ws_at(workspace, l.gr);
    double* SP = qn_ws_at(workspace, l.sp);
    double* S2U = qn_ws_at(workspace, l.s2);
    double* ZG = kind == QN_CURV_HESS_FULL ? qn_ws_at(workspace, l.zg) : nullptr;
    double* AD = kind == QN_CURV_HESS_FULL ? qn_ws_at(workspace, l.ad) : nullptr;
    const int64_t P = g.p;
    const int ntiles = (Nb + g.RT - 1) / g.RT;
    for (int b = 0; b < B; ++b) {
        const double* Wb = W + (int64_t)b * P;
        const int32_t* rows = row_idx ? row_idx + (int64_t)b * Nb : nullptr;
        double* ob = out + (is_full(kind) ? (int64_t)b * P * P : (int64_t)b * P);
        for (int tI = 0; tI < ntiles; ++tI) {
            const int n0 = tI * g.RT, nrows = std::min(g.RT, Nb - n0);
            if (is_ggn(kind))
                hipLaunchKernelGGL(k_jac_rows, dim3((g.RT + 255) / 256, 1), dim3(256), 0, st, g, Wb, X, rows, (int64_t)0, n0,
                                   nrows, IN, G, (double*)nullptr, (int64_t)0);
            else
                hipLaunchKernelGGL(k_curv_rows, dim3((g.RT + 255) / 256), dim3(256), 0, st, g, Wb, X, Y, rows, n0, nrows, IN,
                                   G, SP, S2U);
            QN_HIP_CHECK(hipGetLastError());
            if (kind == QN_CURV_GGN_FULL) {
                for (int i = 0; i < g.L; ++i)
                    for (int m = i; m < g.L; ++m) {
                        const int ei = g.dims[i] + g.hb, em = g.dims[m] + g.hb;
                        const int64_t items = (int64_t)g.dims[i + 1] * ((ei + 63) / 64) * ((g.dims[m + 1] + 3) / 4) *
                                              ((em + 15) / 16);
                        hipLaunchKernelGGL(k_curv_full<true>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, g, i, m, IN,
                                           G, (const double*)nullptr, (const double*)nullptr, ob, tI > 0 ? 1 : 0);
                        QN_HIP_CHECK(hipGetLastError());
                    }
            } else if (kind == QN_CURV_GGN_DIAG) {
                for (int i = 0; i < g.L; ++i) {
                    const int ei = g.dims[i] + g.hb;
                    const int items = ((g.dims[i + 1] + 63) / 64) * ((ei + 15) / 16);
                    hipLaunchKernelGGL(k_curv_diag<true>, dim3((items + 3) / 4), dim3(256), 0, st, g, i, IN, G, ob,
                                       tI > 0 ? 1 : 0, 0.0);
                    QN_HIP_CHECK(hipGetLastError());
                }
            } else if (kind == QN_CURV_HESS_FULL) {
                for (int i = 0; i < g.L; ++i) {
                    hipLaunchKernelGGL(k_curv_tangent, dim3((g.RT + 63) / 64, g.dims[i + 1]), dim3(64), 0, st, g, Wb, i, SP,
                                       S2U, ZG, AD);
                    QN_HIP_CHECK(hipGetLastError());
                }
                for (int i = 0; i < g.L; ++i)
                    for (int m = i; m < g.L; ++m) {
                        const int ei = g.dims[i] + g.hb, em = g.dims[m] + g.hb;
                        const int64_t items = (int64_t)g.dims[i + 1] * ((ei + 63) / 64) * ((g.dims[m + 1] + 3) / 4) *
                                              ((em + 15) / 16);
                        hipLaunchKernelGGL(k_curv_full<false>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, g, i, m, IN, G,
                                           ZG, AD, ob, tI > 0 ? 1 : 0);
                        QN_HIP_CHECK(hipGetLastError());
                    }
            } else {
                for (int i = 0; i < g.L; ++i) {
                    const int ei = g.dims[i] + g.hb;
                    const int items = ((g.dims[i + 1] + 63) / 64) * ((ei + 15) / 16);
                    hipLaunchKernelGGL(k_curv_diag<false>, dim3((items + 3) / 4), dim3(256), 0, st, g, i, IN, G, ob, tI > 0 ? 1 : 0,
                                       tI == ntiles - 1 ? (double)Nb : 0.0);
                    QN_HIP_CHECK(hipGetLastError());
                }
            }
        }
        if (is_full(kind)) {
            const unsigned nt = (unsigned)((P + 31) / 32);
            hipLaunchKernelGGL(k_curv_mirror, dim3(nt, nt), dim3(256), 0, st, ob, P);
            QN_HIP_CHECK(hipGetLastError());
        }
    }
    return QN_OK;
}
