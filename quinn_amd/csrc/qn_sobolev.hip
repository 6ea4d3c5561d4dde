// Input Jacobian of a batched MLP and the derivative-informed ("Sobolev") loss with its weight gradient, float64:
//   J[b][n][k][j] = d f_k(x_n) / d x_j at W[b]                                           (qn_mlp_input_jac)
//   sse[b] = sum_n |f - y|^2,  gsse[b] = sum_n sum_kj (J_kj - G_kj)^2,
//   gradW[b] = wv d sse / dW + wg d gsse / dW                                            (qn_mlp_sobolev_fwdbwd)
// the loss of the reference's GradLoss (quinn/nns/losses.py:84-145).  The weight gradient of gsse is a reverse pass over a
// forward-mode tangent pass.
//
// Notation (Linear layer l = 0..L-1): a_0 = x, z_l = W_l a_l + b_l, a_{l+1} = act(z_l), f = z_{L-1}; input direction j:
//   forward   da_0^j = e_j,  dz_l^j = W_l da_l^j,  da_{l+1}^j = act'(z_l) o dz_l^j,  J[:, j] = dz_{L-1}^j
//   reverse   zb_{L-1} = 2 wv (f - y),  dzb_{L-1}^j = 2 wg (J[:, j] - G[:, j]);  per layer from the top down
//             Wb_l += zb_l a_l^T + sum_j dzb_l^j (da_l^j)^T,  bb_l += zb_l,  ab_l = W_l^T zb_l,  dab_l^j = W_l^T dzb_l^j,
//             zb_{l-1} = act'(z_{l-1}) o ab_l + sum_j act''(z_{l-1}) o dz_{l-1}^j o dab_l^j,  dzb_{l-1}^j = act'(z_{l-1}) o dab_l^j.
//
// EXTENDED ROWS.  A data row n and its d tangents are S = 1 + d rows r = n S + s of one matrix: row s = 0 is [a_l; 1] (the 1
// multiplies the bias), rows s = 1 + j are [da_l^j; 0].  With W~_l = [W_l | b_l] the forward of a layer is ONE product
// A_l W~_l^T over the extended rows, the adjoint pass one product ZB_l W_l, and the weight AND bias gradient one product
// ZB_l^T A_l -- all on v_mfma_f64_16x16x4_f64, a wave holding 64 extended rows, so a weight tile is fetched once for a row's
// value and all its tangents.  Between the products one elementwise kernel per layer does everything that couples a value
// row with its tangent rows: forward a, act'(z) dz^j in one pass over z (k_sob_act); reverse zb, dzb^j in one pass, with
// act''(z) dz^j = -2 a da^j for tanh formed from what the forward stored (k_sob_bwd_act).  relu's act' is the select of the
// gradient kernels (qn_act_bwd), its act'' is 0.
//
// Rows go in tiles of RT data rows (RE = RT S extended rows, a multiple of 64), bounded by SOB_BUDGET bytes per member; all
// members of a call run in one launch (blockIdx.y).  Rows past the end of a tile are zero in every array and are seeded
// with zero, so they add exact zeros.  Weight-gradient partial sums over chunks of SOB_KC extended rows go to a slab and
// are added in chunk order, tiles in tile order, the two sums of squares block by block in a fixed order: no atomics, two
// calls give the same bits, and nothing depends on B.
#include "qn_curv_rows.h"
#include "qn_host_args.h"
#include <algorithm>

namespace {

constexpr size_t SOB_BUDGET = size_t(1) << 28;   // bytes of extended rows per member and row tile
constexpr int SOB_RT_MAX = 2048;                 // data rows per tile
constexpr int SOB_KC = 1024;                     // extended rows per weight-gradient chunk
constexpr int SOB_MAX_D = 16, SOB_MAX_O = 16;

struct SobArgs {
    int L, act, hb, d, o, S;
    int64_t p;
    int dims[QN_MAX_LAYERS + 1];
    int64_t offW[QN_MAX_LAYERS], offB[QN_MAX_LAYERS];
    int64_t offA[QN_MAX_LAYERS];   // doubles: start of A_l [RE][dims[l] + hb] inside a member's A block
    int RT, RE, hmax, nchunks;
};

// ---- A_0: extended input rows [x; 1], [e_j; 0] of the tile's data rows; zero past nrows.  grid (RT / 256, B)
__global__ __launch_bounds__(256) void k_sob_input(SobArgs g, const double* __restrict__ X, const int32_t* __restrict__ rows,
                                                   int Nb, int n0, int nrows, double* __restrict__ A, int64_t strideA) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= g.RT) return;
    const int b = blockIdx.y, e = g.d + g.hb;
    double* a = A + (int64_t)b * strideA + g.offA[0] + (int64_t)n * g.S * e;
    if (n >= nrows) {
        for (int i = 0; i < g.S * e; ++i) a[i] = 0.0;
        return;
    }
    const int64_t row = rows ? rows[(int64_t)b * Nb + n0 + n] : (int64_t)(n0 + n);
    for (int k = 0; k < g.d; ++k) a[k] = X[row * g.d + k];
    if (g.hb) a[g.d] = 1.0;
    for (int j = 0; j < g.d; ++j) {
        double* t = a + (int64_t)(1 + j) * e;
        for (int k = 0; k < e; ++k) t[k] = k == j ? 1.0 : 0.0;
    }
}

// ---- forward product of layer l over the extended rows: Z [RE][ho] = A_l [RE][e] W~_l^T, e = hin + hb.
// One wave = 64 extended rows x 32 units: 4 x 2 accumulator tiles, K = e in steps of 16.  Operand maps (one f64 per lane,
// q = lane >> 4, cl = lane & 15): A[row cl][k] and B[k][col cl] with k = k0 + 4 q + t for the t-th MFMA of a step, so a
// lane reads 4 consecutive doubles of its row of A_l and of W_l;  C/D reg i = row q + 4 i, col cl.
__global__ __launch_bounds__(256) void k_sob_fwd(SobArgs g, int l, const double* __restrict__ W, const double* __restrict__ A,
                                                 int64_t strideA, double* __restrict__ Z, int64_t strideZ) {
    const int lane = threadIdx.x & 63, q = lane >> 4, cl = lane & 15;
    const int hin = g.dims[l], ho = g.dims[l + 1], e = hin + g.hb;
    const int nrt = g.RE / 64, nct = (ho + 31) / 32;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nrt * nct) return;
    const int rt = w % nrt, ct = w / nrt, b = blockIdx.y;
    const int r0 = rt * 64, c0 = ct * 32;
    const int ntn = min(2, (ho - c0 + 15) / 16);
    const double* Wb = W + (int64_t)b * g.p;
    const double* Ar = A + (int64_t)b * strideA + g.offA[l] + (int64_t)(r0 + cl) * e;
    const int cc[2] = {min(c0 + cl, ho - 1), min(c0 + 16 + cl, ho - 1)};
    dv4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = (dv4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < e; k0 += 16) {
        double av[4][4], bv[2][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = k0 + 4 * q + t, kc = min(k, e - 1);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const double v = Ar[(int64_t)(16 * mt) * e + kc];
                av[mt][t] = k < e ? v : 0.0;
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const double v = k < hin ? Wb[g.offW[l] + (int64_t)cc[nt] * hin + k] : Wb[g.hb ? g.offB[l] + cc[nt] : 0];
                bv[nt][t] = k < e ? v : 0.0;
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                if (nt < ntn) {
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = mfma64(av[mt][t], bv[nt][t], acc[mt][nt]);
                }
    }
    double* Zb = Z + (int64_t)b * strideZ;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int col = c0 + 16 * nt + cl;
            if (nt >= ntn || col >= ho) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) Zb[(int64_t)(r0 + 16 * mt + q + 4 * i) * ho + col] = acc[mt][nt][i];
        }
}

// ---- activation of layer l over Z [RE][ho] in one pass: A_{l+1} [RE][ho + hb] value rows a = act(z) (and the bias 1),
// tangent rows act'(z) o dz^j (and 0).  One thread per (data row, column of A_{l+1}).  grid (RT (ho + hb) / 256, B)
__global__ __launch_bounds__(256) void k_sob_act(SobArgs g, int l, int nrows, const double* __restrict__ Z, int64_t strideZ,
                                                 double* __restrict__ A, int64_t strideA) {
    const int ho = g.dims[l + 1], e = ho + g.hb;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)g.RT * e) return;
    const int n = (int)(idx / e), c = (int)(idx % e), b = blockIdx.y;
    double* an = A + (int64_t)b * strideA + g.offA[l + 1] + (int64_t)n * g.S * e + c;
    if (c == ho) {                                 // bias slot
        an[0] = n < nrows ? 1.0 : 0.0;
        for (int s = 1; s < g.S; ++s) an[(int64_t)s * e] = 0.0;
        return;
    }
    const double* zn = Z + (int64_t)b * strideZ + (int64_t)n * g.S * ho + c;
    const double z = zn[0];
    if (g.act == QN_ACT_TANH) {
        const double a = qn_tanh_f64(z), d1 = 1.0 - a * a;
        an[0] = a;
        for (int s = 1; s < g.S; ++s) an[(int64_t)s * e] = d1 * zn[(int64_t)s * ho];
    } else if (g.act == QN_ACT_RELU) {
        const double a = qn_relu<double>(z);
        an[0] = a;
        for (int s = 1; s < g.S; ++s) an[(int64_t)s * e] = qn_act_bwd<double>(zn[(int64_t)s * ho], a, QN_ACT_RELU);
    } else {
        for (int s = 0; s < g.S; ++s) an[(int64_t)s * e] = zn[(int64_t)s * ho];
    }
}

// ---- predictions and Jacobian out of the last layer's Z [RE][o].  grid (RT / 256, B)
__global__ __launch_bounds__(256) void k_sob_out(SobArgs g, int Nb, int n0, int nrows, const double* __restrict__ Z,
                                                 int64_t strideZ, double* __restrict__ pred, double* __restrict__ jac) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= nrows) return;
    const int b = blockIdx.y, o = g.o, d = g.d;
    const double* zn = Z + (int64_t)b * strideZ + (int64_t)n * g.S * o;
    const int64_t r = (int64_t)b * Nb + n0 + n;
    if (pred)
        for (int k = 0; k < o; ++k) pred[r * o + k] = zn[k];
    for (int k = 0; k < o; ++k)
        for (int j = 0; j < d; ++j) jac[(r * o + k) * d + j] = zn[(int64_t)(1 + j) * o + k];
}

// ---- the two sums of squares of the tile and the seeds of the reverse pass, in place on Z [RE][o]:
// value rows := 2 wv (f - y), tangent rows := 2 wg (J[:, j] - G[:, j]); rows past nrows := 0.
// part [B][2][npart]: this block's sums at column tile_part0 + blockIdx.x.  grid (RT / 256, B)
__global__ __launch_bounds__(256) void k_sob_seed(SobArgs g, const double* __restrict__ Y, const double* __restrict__ G,
                                                  const int32_t* __restrict__ rows, int Nb, int n0, int nrows, double twv,
                                                  double twg, double* __restrict__ Z, int64_t strideZ,
                                                  double* __restrict__ part, int npart, int part0) {
    __shared__ double red[2][4];
    const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, o = g.o, d = g.d;
    double s = 0.0, gs = 0.0;
    if (n < g.RT) {
        double* zn = Z + (int64_t)b * strideZ + (int64_t)n * g.S * o;
        if (n < nrows) {
            const int64_t row = rows ? rows[(int64_t)b * Nb + n0 + n] : (int64_t)(n0 + n);
            for (int k = 0; k < o; ++k) {
                const double r = Y ? zn[k] - Y[row * o + k] : 0.0;
                s = fma(r, r, s);
                zn[k] = twv * r;
            }
            for (int j = 0; j < d; ++j)
                for (int k = 0; k < o; ++k) {
                    const double ev = G ? zn[(int64_t)(1 + j) * o + k] - G[(row * o + k) * d + j] : 0.0;
                    gs = fma(ev, ev, gs);
                    zn[(int64_t)(1 + j) * o + k] = twg * ev;
                }
        } else {
            for (int i = 0; i < g.S * o; ++i) zn[i] = 0.0;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off, 64);
        gs += __shfl_down(gs, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s;
        red[1][threadIdx.x >> 6] = gs;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double* r = red[threadIdx.x];
        part[((int64_t)b * 2 + threadIdx.x) * npart + part0 + blockIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
    }
}

__global__ __launch_bounds__(64) void k_sob_sums(const double* __restrict__ part, int npart, int B, double* __restrict__ sse,
                                                 double* __restrict__ gsse) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= 2 * B) return;
    double* out = (i & 1) ? gsse : sse;
    if (!out) return;
    double s = 0.0;
    for (int k = 0; k < npart; ++k) s += part[(int64_t)i * npart + k];
    out[i >> 1] = s;
}

// ---- adjoint product of layer l >= 1 over the extended rows: AB [RE][hin] = ZB_l [RE][ho] W_l.
// One wave = 64 extended rows x 32 inputs, K = ho in steps of 16; A[row cl][c], B[c][col cl] = W_l[c][k0 + cl], c = c0 + 4 q + t.
__global__ __launch_bounds__(256) void k_sob_da(SobArgs g, int l, const double* __restrict__ W, const double* __restrict__ ZB,
                                                double* __restrict__ AB, int64_t strideZ) {
    const int lane = threadIdx.x & 63, q = lane >> 4, cl = lane & 15;
    const int hin = g.dims[l], ho = g.dims[l + 1];
    const int nrt = g.RE / 64, nct = (hin + 31) / 32;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nrt * nct) return;
    const int rt = w % nrt, ct = w / nrt, b = blockIdx.y;
    const int r0 = rt * 64, k0 = ct * 32;
    const int ntn = min(2, (hin - k0 + 15) / 16);
    const double* Wl = W + (int64_t)b * g.p + g.offW[l];
    const double* Zr = ZB + (int64_t)b * strideZ + (int64_t)(r0 + cl) * ho;
    const int kk[2] = {min(k0 + cl, hin - 1), min(k0 + 16 + cl, hin - 1)};
    dv4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = (dv4){0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < ho; c0 += 16) {
        double av[4][4], bv[2][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = c0 + 4 * q + t, cc = min(c, ho - 1);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const double v = Zr[(int64_t)(16 * mt) * ho + cc];
                av[mt][t] = c < ho ? v : 0.0;
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const double v = Wl[(int64_t)cc * hin + kk[nt]];
                bv[nt][t] = c < ho ? v : 0.0;
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                if (nt < ntn) {
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = mfma64(av[mt][t], bv[nt][t], acc[mt][nt]);
                }
    }
    double* Ab = AB + (int64_t)b * strideZ;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int col = k0 + 16 * nt + cl;
            if (nt >= ntn || col >= hin) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) Ab[(int64_t)(r0 + 16 * mt + q + 4 * i) * hin + col] = acc[mt][nt][i];
        }
}

// ---- reverse of the activation of layer l - 1 in one pass, in place on AB [RE][h] (h = dims[l]), reading A_l [RE][h + hb]:
//   value row  zb = act'(z) ab + sum_j act''(z) dz^j dab^j  (tanh: act'' dz^j = -2 a da^j);  tangent rows dzb^j = act'(z) dab^j.
// One thread per (data row, unit).  grid (RT h / 256, B)
__global__ __launch_bounds__(256) void k_sob_bwd_act(SobArgs g, int l, const double* __restrict__ A, int64_t strideA,
                                                     double* __restrict__ AB, int64_t strideZ) {
    const int h = g.dims[l], e = h + g.hb;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)g.RT * h) return;
    const int n = (int)(idx / h), c = (int)(idx % h), b = blockIdx.y;
    const double* an = A + (int64_t)b * strideA + g.offA[l] + (int64_t)n * g.S * e + c;
    double* gn = AB + (int64_t)b * strideZ + (int64_t)n * g.S * h + c;
    const double a = an[0];
    if (g.act == QN_ACT_TANH) {
        const double d1 = 1.0 - a * a, m2a = -2.0 * a;
        double zb = d1 * gn[0];
        for (int s = 1; s < g.S; ++s) {
            const double dab = gn[(int64_t)s * h];
            zb = fma(m2a * an[(int64_t)s * e], dab, zb);
            gn[(int64_t)s * h] = d1 * dab;
        }
        gn[0] = zb;
    } else {
        for (int s = 0; s < g.S; ++s) gn[(int64_t)s * h] = qn_act_bwd<double>(gn[(int64_t)s * h], a, QN_ACT_RELU);
    }
}

// ---- weight and bias gradient of layer l over one chunk of SOB_KC extended rows: slab[chunk][W~_l] = ZB_l^T A_l.
// One wave = 64 units x 32 input slots, K = extended rows in steps of 16; A[row cl][r] = ZB[r][c0 + cl],
// B[r][col cl] = A_l[r][k0 + cl], r = r0 + 4 q + t.  slab [B][nchunks][p]
__global__ __launch_bounds__(256) void k_sob_dw(SobArgs g, int l, const double* __restrict__ ZB, int64_t strideZ,
                                                const double* __restrict__ A, int64_t strideA, double* __restrict__ slab) {
    const int lane = threadIdx.x & 63, q = lane >> 4, cl = lane & 15;
    const int hin = g.dims[l], ho = g.dims[l + 1], e = hin + g.hb;
    const int nmt = (ho + 63) / 64, nnt = (e + 31) / 32;
    int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nmt * nnt * g.nchunks) return;
    const int kt = w % nnt; w /= nnt;
    const int ct = w % nmt;
    const int ch = w / nmt, b = blockIdx.y;
    const int c0 = ct * 64, k0 = kt * 32;
    const int mtn = min(4, (ho - c0 + 15) / 16), ntn = min(2, (e - k0 + 15) / 16);
    const int rbeg = ch * SOB_KC, rend = min(g.RE, rbeg + SOB_KC);
    const double* Zb = ZB + (int64_t)b * strideZ;
    const double* Ab = A + (int64_t)b * strideA + g.offA[l];
    const int cc[4] = {min(c0 + cl, ho - 1), min(c0 + 16 + cl, ho - 1), min(c0 + 32 + cl, ho - 1), min(c0 + 48 + cl, ho - 1)};
    const int kk[2] = {min(k0 + cl, e - 1), min(k0 + 16 + cl, e - 1)};
    dv4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = (dv4){0.0, 0.0, 0.0, 0.0};
    for (int r0 = rbeg; r0 < rend; r0 += 16) {          // RE and SOB_KC are multiples of 16: no ragged step
        double av[4][4], bv[2][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t r = r0 + 4 * q + t;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) av[mt][t] = mt < mtn ? Zb[r * ho + cc[mt]] : 0.0;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) bv[nt][t] = nt < ntn ? Ab[r * e + kk[nt]] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                if (nt < ntn) {
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
                        if (mt < mtn) acc[mt][nt] = mfma64(av[mt][t], bv[nt][t], acc[mt][nt]);
                }
    }
    double* sl = slab + ((int64_t)b * g.nchunks + ch) * g.p;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int k = k0 + 16 * nt + cl;
            if (mt >= mtn || nt >= ntn || k >= e) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = c0 + 16 * mt + q + 4 * i;
                if (c >= ho) continue;
                sl[k < hin ? g.offW[l] + (int64_t)c * hin + k : g.offB[l] + c] = acc[mt][nt][i];
            }
        }
}

// ---- gradW[b][e] = (accumulate ? gradW[b][e] : 0) + slab[b][0][e] + slab[b][1][e] + ...   grid (p / 256, B)
__global__ __launch_bounds__(256) void k_sob_reduce(const double* __restrict__ slab, int nchunks, int64_t p, int accumulate,
                                                    double* __restrict__ gradW) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p) return;
    const int b = blockIdx.y;
    double* o = gradW + (int64_t)b * p + i;
    double s = accumulate ? *o : 0.0;
    for (int k = 0; k < nchunks; ++k) s += slab[((int64_t)b * nchunks + k) * p + i];
    *o = s;
}

struct SobLayout { size_t a, z0, z1, slab, part, total; int64_t strideA, strideZ; int ntiles, nblk; };

bool fill_args(const qn_desc* d, int Nb, int want_grad, SobArgs* g, const char* who) {
    if (!qn_check_mlp_desc(d, who, "the input-derivative kernels")) return false;
    const int din = d->dims[0], o = d->dims[d->nlayers];
    if (din > SOB_MAX_D || o > SOB_MAX_O) {
        qn_set_error("%s: d = %d inputs, o = %d outputs: the input-derivative kernels take d <= %d and o <= %d", who, din, o,
                     SOB_MAX_D, SOB_MAX_O);
        return false;
    }
    if (Nb <= 0) {
        qn_set_error("%s: need Nb >= 1 rows", who);
        return false;
    }
    g->L = d->nlayers;
    g->act = d->act;
    g->hb = d->has_bias;
    g->d = din;
    g->o = o;
    g->S = 1 + din;
    g->p = d->p;
    size_t per_row = 0;          // doubles per extended row: the layer inputs and two product buffers
    int hmax = 0;
    for (int i = 0; i <= d->nlayers; ++i) g->dims[i] = d->dims[i];
    for (int i = 0; i < d->nlayers; ++i) {
        g->offW[i] = d->offW[i];
        g->offB[i] = d->offB[i];
        per_row += d->dims[i] + d->has_bias;
        hmax = std::max(hmax, d->dims[i + 1]);
    }
    per_row += 2 * (size_t)hmax;
    g->hmax = hmax;
    const size_t fit = SOB_BUDGET / (per_row * g->S * sizeof(double)) / 64 * 64;
    const int rt = (int)std::min<size_t>(SOB_RT_MAX, std::max<size_t>(64, fit));
    g->RT = std::min(rt, (Nb + 63) / 64 * 64);
    g->RE = g->RT * g->S;
    g->nchunks = (g->RE + SOB_KC - 1) / SOB_KC;
    // A_l of every layer is kept for the reverse pass; the forward alone alternates between two blocks
    int emax = 0;
    for (int i = 0; i < g->L; ++i) emax = std::max(emax, g->dims[i] + g->hb);
    int64_t off = 0;
    for (int i = 0; i < g->L; ++i) {
        if (want_grad) {
            g->offA[i] = off;
            off += (int64_t)g->RE * (g->dims[i] + g->hb);
        } else {
            g->offA[i] = (int64_t)(i & 1) * g->RE * emax;
        }
    }
    return true;
}

SobLayout layout(const SobArgs& g, int B, int Nb, int want_grad) {
    SobLayout l;
    int emax = 0;
    int64_t esum = 0;
    for (int i = 0; i < g.L; ++i) {
        emax = std::max(emax, g.dims[i] + g.hb);
        esum += g.dims[i] + g.hb;
    }
    l.strideA = (int64_t)g.RE * (want_grad ? esum : (int64_t)std::min(g.L, 2) * emax);
    l.strideZ = (int64_t)g.RE * g.hmax;
    l.ntiles = (Nb + g.RT - 1) / g.RT;
    l.nblk = (g.RT + 255) / 256;
    qn_ws_carver c;
    l.a = c.take_doubles((size_t)B * l.strideA);
    l.z0 = c.take_doubles((size_t)B * l.strideZ);
    l.z1 = want_grad ? c.take_doubles((size_t)B * l.strideZ) : 0;
    l.slab = want_grad ? c.take_doubles((size_t)B * g.nchunks * g.p) : 0;
    l.part = c.take_doubles((size_t)B * 2 * l.ntiles * l.nblk);
    l.total = c.total;
    return l;
}

bool check_common(const char* who, const double* W, const double* X, const int32_t* row_idx, int B, int N, int Nb) {
    if (!qn_check_members(B, who)) return false;
    if (N <= 0 || !W || !X) {
        qn_set_error("%s: need N >= 1 and non-NULL W, X", who);
        return false;
    }
    return qn_check_row_idx(row_idx, N, Nb, who);
}

// the forward of one row tile: leaves the last layer's Z in Z0 (and, for the reverse pass, every A_l)
int forward_tile(const SobArgs& g, const SobLayout& l, const double* W, const double* X, const int32_t* row_idx, int B, int Nb,
                 int n0, int nrows, double* A, double* Z0, hipStream_t st) {
    hipLaunchKernelGGL(k_sob_input, dim3((g.RT + 255) / 256, B), dim3(256), 0, st, g, X, row_idx, Nb, n0, nrows, A, l.strideA);
    QN_HIP_CHECK(hipGetLastError());
    for (int i = 0; i < g.L; ++i) {
        const int ho = g.dims[i + 1];
        const int waves = (g.RE / 64) * ((ho + 31) / 32);
        hipLaunchKernelGGL(k_sob_fwd, dim3((waves + 3) / 4, B), dim3(256), 0, st, g, i, W, (const double*)A, l.strideA, Z0,
                           l.strideZ);
        QN_HIP_CHECK(hipGetLastError());
        if (i + 1 < g.L) {
            const int64_t items = (int64_t)g.RT * (ho + g.hb);
            hipLaunchKernelGGL(k_sob_act, dim3((unsigned)((items + 255) / 256), B), dim3(256), 0, st, g, i, nrows,
                               (const double*)Z0, l.strideZ, A, l.strideA);
            QN_HIP_CHECK(hipGetLastError());
        }
    }
    return QN_OK;
}

}  // namespace

extern "C" size_t qn_sobolev_workspace_bytes(const qn_desc* d, int B, int Nb, int want_grad) {
    SobArgs g;
    if (B <= 0) {
        qn_set_error("qn_sobolev_workspace_bytes: need B >= 1");
        return 0;
    }
    if (!fill_args(d, Nb, want_grad, &g, "qn_sobolev_workspace_bytes")) return 0;
    return layout(g, B, Nb, want_grad).total;
}

extern "C" int qn_mlp_input_jac(const qn_desc* d, const double* W, const double* X, const int32_t* row_idx, int B, int N, int Nb,
                                double* pred_out, double* jac_out, void* workspace, size_t workspace_bytes, void* stream) {
    SobArgs g;
    if (!fill_args(d, Nb, 0, &g, "qn_mlp_input_jac")) return QN_EINVAL;
    if (!check_common("qn_mlp_input_jac", W, X, row_idx, B, N, Nb)) return QN_EINVAL;
    if (!jac_out) {
        qn_set_error("qn_mlp_input_jac: jac_out is NULL");
        return QN_EINVAL;
    }
    const SobLayout l = layout(g, B, Nb, 0);
    if (!qn_check_workspace(workspace, workspace_bytes, l.total, "qn_mlp_input_jac")) return QN_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* A = qn_ws_at(workspace, l.a);
    double* Z0 = qn_ws_at(workspace, l.z0);
    for (int tI = 0; tI < l.ntiles; ++tI) {
        const int n0 = tI * g.RT, nrows = std::min(g.RT, Nb - n0);
        const int rc = forward_tile(g, l, W, X, row_idx, B, Nb, n0, nrows, A, Z0, st);
        if (rc != QN_OK) return rc;
        hipLaunchKernelGGL(k_sob_out, dim3((g.RT + 255) / 256, B), dim3(256), 0, st, g, Nb, n0, nrows, (const double*)Z0,
                           l.strideZ, pred_out, jac_out);
        QN_HIP_CHECK(hipGetLastError());
    }
    return QN_OK;
}

extern "C" int qn_mlp_sobolev_fwdbwd(const qn_desc* d, const double* W, const double* X, const double* Y, const double* G,
                                     const int32_t* row_idx, int B, int N, int Nb, double wv, double wg, double* sse_out,
                                     double* gsse_out, double* gradW_out, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    const int want_grad = gradW_out ? 1 : 0;
    SobArgs g;
    if (!fill_args(d, Nb, want_grad, &g, "qn_mlp_sobolev_fwdbwd")) return QN_EINVAL;
    if (!check_common("qn_mlp_sobolev_fwdbwd", W, X, row_idx, B, N, Nb)) return QN_EINVAL;
    if (!Y && (wv != 0.0 || sse_out)) {
        qn_set_error("qn_mlp_sobolev_fwdbwd: Y may be NULL only when wv == 0 and sse_out == NULL");
        return QN_EINVAL;
    }
    if (!G && (wg != 0.0 || gsse_out)) {
        qn_set_error("qn_mlp_sobolev_fwdbwd: G may be NULL only when wg == 0 and gsse_out == NULL");
        return QN_EINVAL;
    }
    const SobLayout l = layout(g, B, Nb, want_grad);
    if (!qn_check_workspace(workspace, workspace_bytes, l.total, "qn_mlp_sobolev_fwdbwd")) return QN_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* A = qn_ws_at(workspace, l.a);
    double* Z0 = qn_ws_at(workspace, l.z0);
    double* Z1 = qn_ws_at(workspace, l.z1);
    double* slab = qn_ws_at(workspace, l.slab);
    double* part = qn_ws_at(workspace, l.part);
    const int npart = l.ntiles * l.nblk;
    for (int tI = 0; tI < l.ntiles; ++tI) {
        const int n0 = tI * g.RT, nrows = std::min(g.RT, Nb - n0);
        const int rc = forward_tile(g, l, W, X, row_idx, B, Nb, n0, nrows, A, Z0, st);
        if (rc != QN_OK) return rc;
        hipLaunchKernelGGL(k_sob_seed, dim3(l.nblk, B), dim3(256), 0, st, g, Y, G, row_idx, Nb, n0, nrows, 2.0 * wv, 2.0 * wg, Z0,
                           l.strideZ, part, npart, tI * l.nblk);
        QN_HIP_CHECK(hipGetLastError());
        if (!want_grad) continue;
        double* zb = Z0;           // ZB_i
        double* other = Z1;
        for (int i = g.L - 1; i >= 0; --i) {
            const int hin = g.dims[i], ho = g.dims[i + 1], e = hin + g.hb;
            const int wdw = ((ho + 63) / 64) * ((e + 31) / 32) * g.nchunks;
            hipLaunchKernelGGL(k_sob_dw, dim3((wdw + 3) / 4, B), dim3(256), 0, st, g, i, (const double*)zb, l.strideZ,
                               (const double*)A, l.strideA, slab);
            QN_HIP_CHECK(hipGetLastError());
            if (i == 0) break;
            const int wda = (g.RE / 64) * ((hin + 31) / 32);
            hipLaunchKernelGGL(k_sob_da, dim3((wda + 3) / 4, B), dim3(256), 0, st, g, i, W, (const double*)zb, other, l.strideZ);
            QN_HIP_CHECK(hipGetLastError());
            if (g.act != QN_ACT_IDENTITY) {
                const int64_t items = (int64_t)g.RT * hin;
                hipLaunchKernelGGL(k_sob_bwd_act, dim3((unsigned)((items + 255) / 256), B), dim3(256), 0, st, g, i,
                                   (const double*)A, l.strideA, other, l.strideZ);
                QN_HIP_CHECK(hipGetLastError());
            }
            std::swap(zb, other);
        }
        hipLaunchKernelGGL(k_sob_reduce, dim3((unsigned)((g.p + 255) / 256), B), dim3(256), 0, st, (const double*)slab, g.nchunks,
                           g.p, tI > 0 ? 1 : 0, gradW_out);
        QN_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_sob_sums, dim3((2 * B + 63) / 64), dim3(64), 0, st, (const double*)part, npart, B, sse_out, gsse_out);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
