// Kronecker-factored Gauss-Newton of a batched MLP ('kron' Laplace), float64.  Notation of qn_curv_rows.h: ~in_i = [in_i; 1] of
// length e_i = h_i + has_bias is the input of Linear layer i, g^k_i the backward signal at z_i from output unit vector e_k.
//   factors    A_i = sum_n ~in_i ~in_i^T [e_i, e_i],   S_i = sum_n sum_k g^k_i g^k_i^T [h_{i+1}, h_{i+1}]     (plain sums over the rows)
//   the layer-i diagonal block of sum_n sum_k J_nk^T J_nk is approximated by (S_i (x) A_i) / Nb, row index (unit a, slot b)
//   posterior  with S_i = U_S L_S U_S^T, A_i = U_A L_A U_A^T (the caller's eigendecompositions; eigenvectors are COLUMNS) the
//              precision of pair (a, c) is diagonal in the rotated basis; the caller passes its reciprocal Dinv and Dih = sqrt(Dinv)
//   "kron order" of a length-p vector: layer i, unit a, slot c < e_i at offK[i] + a e_i + c  (offK[i] = offW[i]; not the flat
//              order when there are biases: param_index maps (i, a, c) to flat order)
//
// FACTORS (qn_mlp_kron_factors).  k_jac_rows leaves IN [B][RT][EI] and GK [B][o][RT][D] of a row tile.  k_kron_syrk: one wave owns
// one 64 x 64 tile on or below the diagonal of one factor and one chunk of KRON_RC rows of the tile; K = the rows (times the
// outputs for S), four per v_mfma_f64_16x16x4_f64: A[row cl][k q] = X[n + q][r0 + 16 mt + cl], B[k q][col cl] =
// X[n + q][c0 + 16 ct + cl], C/D reg r = row q + 4 r, col cl (q = lane >> 4, cl = lane & 15), the maps of qn_glm.hip.  The
// wave stores its tile as a partial; k_kron_reduce adds the chunks of an entry a >= b in chunk order, adds the earlier row
// tiles' total and writes it to [a][b] and [b][a]: both triangles, equal bit for bit, no atomics, and nothing depends on B.
//
// GLM (qn_mlp_kron_glm_predict).  cov[n][k][l] = sum_i sum_{a,c} Dinv_i[a][c] gh^k_a gh^l_a ah_c^2, gh^k = U_S^T g^k_i,
// ah = U_A^T ~in_i.  Per tile of query rows: k_jac_rows, then k_kron_rotate (row-block x eigenbasis GEMMs on the MFMA) leaves
// AH2 = (IN U_A)^2 and GH = GK U_S; k_kron_glm: one wave owns 16 query rows and for every layer and every 64 units a forms
// T[n][a] = sum_c AH2[n][c] Dinv[a][c] on the MFMA, multiplies the accumulator tile by gh^k_a gh^l_a (l >= k), sums the 16
// columns a lane group holds with a fixed butterfly and adds the result to cov[n][k][l] -- the same lane for the same row every
// time, in layer and unit order; after the last one the lane copies cov[n][k][l] to cov[n][l][k].  T never leaves the registers.
//
// SAMPLE (qn_kron_sample).  Layer block of draw m (member j = js[m]) = mean + U_S (Z o Dih) U_A^T.  One block per (draw, layer,
// 16 input slots b'): T1[a][b'] = sum_c Z[a][c] Dih[a][c] U_A[b'][c] for all units a into LDS, then
// Y[a'][b'] = sum_a U_S[a'][a] T1[a][b'] and W_out = mean + Y at param_index(i, a', b'); both products on the MFMA.
#include <algorithm>

#include "qn_curv_rows.h"
#include "qn_host_args.h"

namespace {

constexpr int KRON_MAX_W = 512;       // widest layer taken: the sampler keeps a [width][16] panel in 64 KB of LDS
constexpr int KRON_RT = 2048;         // rows per tile of the factor accumulation
constexpr int KRON_RC = 512;          // rows per partial (chunk) within a tile
constexpr int KRON_GLM_RT = 1024;     // query rows per tile of the predictive

struct KronArgs {
    int64_t offA[QN_MAX_LAYERS], offS[QN_MAX_LAYERS], offK[QN_MAX_LAYERS];
    int64_t lenA, lenS;
    int itemStart[2 * QN_MAX_LAYERS + 1];   // syrk tiles: slot 2 i = A_i, 2 i + 1 = S_i
    int colStart[QN_MAX_LAYERS + 1];        // sampler: panels of 16 input slots per layer
};

void kron_fill(const CurvArgs& g, KronArgs* k) {
    int64_t a = 0, s = 0;
    int items = 0, cols = 0;
    for (int i = 0; i < g.L; ++i) {
        const int e = g.dims[i] + g.hb, h = g.dims[i + 1];
        k->offA[i] = a;
        k->offS[i] = s;
        k->offK[i] = g.offW[i];
        a += (int64_t)e * e;
        s += (int64_t)h * h;
        const int ta = (e + 63) / 64, ts = (h + 63) / 64;
        k->itemStart[2 * i] = items;
        items += ta * (ta + 1) / 2;
        k->itemStart[2 * i + 1] = items;
        items += ts * (ts + 1) / 2;
        k->colStart[i] = cols;
        cols += (e + 15) / 16;
    }
    k->itemStart[2 * g.L] = items;
    k->colStart[g.L] = cols;
    k->lenA = a;
    k->lenS = s;
}

// ---- one wave = one lower-triangle 64 x 64 tile of one factor x one row chunk.  grid (ceil(items * nchunks / 4), members)
// part [members][nchunks][lenA + lenS]: A factors, then S factors; only entries row >= col of a tile are written
__global__ __launch_bounds__(256) void k_kron_syrk(CurvArgs g, KronArgs kr, const double* __restrict__ IN,
                                                   const double* __restrict__ GK, int nchunks, double* __restrict__ part) {
    const int lane = threadIdx.x & 63, q = lane >> 4, cl = lane & 15;
    const int nitems = kr.itemStart[2 * g.L];
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nitems * nchunks) return;                    // whole waves leave together
    const int chunk = w / nitems, item = w % nitems;
    int slot = 0;
    while (item >= kr.itemStart[slot + 1]) ++slot;
    const int i = slot >> 1, isS = slot & 1;
    int t = item - kr.itemStart[slot], ti = 0;
    while (t > ti) { t -= ti + 1; ++ti; }
    const int tj = t;                                     // tile row ti >= tile column tj
    const int mb = blockIdx.y;
    const int dim = isS ? g.dims[i + 1] : g.dims[i] + g.hb;
    const int width = isS ? g.D : g.EI, coff = isS ? g.offG[i] : g.offIN[i];
    const int nk = isS ? g.o : 1;
    const size_t kstride = (size_t)g.RT * g.D;
    const double* src = isS ? GK + (size_t)mb * g.o * kstride : IN + (size_t)mb * g.RT * g.EI;
    const int r0 = ti * 64, c0 = tj * 64;
    const int mtn = min(4, (dim - r0 + 15) / 16), ctn = min(4, (dim - c0 + 15) / 16);
    int rc[4], cc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        rc[m] = coff + min(r0 + 16 * m + cl, dim - 1);
        cc[m] = coff + min(c0 + 16 * m + cl, dim - 1);
    }
    dv4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[mt][ct] = (dv4){0.0, 0.0, 0.0, 0.0};
    const int nb = chunk * KRON_RC, ne = min(g.RT, nb + KRON_RC);          // RT and RC are multiples of 4
    for (int k = 0; k < nk; ++k) {
        const double* sk = src + k * kstride;
        for (int n0 = nb; n0 < ne; n0 += 4) {
            const double* row = sk + (size_t)(n0 + q) * width;
            double a[4], b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                a[m] = row[rc[m]];
                b[m] = row[cc[m]];
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    if (mt < mtn && ct < ctn) acc[mt][ct] = mfma64(a[mt], b[ct], acc[mt][ct]);
        }
    }
    double* pb = part + ((size_t)mb * nchunks + chunk) * (size_t)(kr.lenA + kr.lenS) + (isS ? kr.lenA + kr.offS[i] : kr.offA[i]);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = r0 + 16 * mt + q + 4 * r, col = c0 + 16 * ct + cl;
                if (mt < mtn && ct < ctn && rr < dim && col <= rr) pb[(size_t)rr * dim + col] = acc[mt][ct][r];
            }
}

// ---- entry [a][b], a >= b, of every factor: chunks in order, plus the total of the earlier row tiles; both triangles written
__global__ __launch_bounds__(256) void k_kron_reduce(CurvArgs g, KronArgs kr, const double* __restrict__ part, int nchunks,
                                                     int accumulate, double* __restrict__ Aout, double* __restrict__ Sout) {
    const int64_t len = kr.lenA + kr.lenS;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= len) return;
    const int mb = blockIdx.y;
    const bool isS = idx >= kr.lenA;
    const int64_t loc = isS ? idx - kr.lenA : idx;
    int i = g.L - 1;
    while (i > 0 && loc < (isS ? kr.offS[i] : kr.offA[i])) --i;
    const int dim = isS ? g.dims[i + 1] : g.dims[i] + g.hb;
    const int64_t r = loc - (isS ? kr.offS[i] : kr.offA[i]);
    const int a = (int)(r / dim), b = (int)(r % dim);
    if (b > a) return;
    const double* pb = part + (size_t)mb * nchunks * len + idx;
    double v = pb[0];
    for (int c = 1; c < nchunks; ++c) v += pb[(size_t)c * len];
    double* ob = (isS ? Sout + (size_t)mb * kr.lenS + kr.offS[i] : Aout + (size_t)mb * kr.lenA + kr.offA[i]);
    if (accumulate) v = ob[(size_t)a * dim + b] + v;
    ob[(size_t)a * dim + b] = v;
    ob[(size_t)b * dim + a] = v;
}

// ---- dst[r][off + c] = sum_b src[r][off + b] U[b][c]  (squared if `square`), r < R (a multiple of 16), b, c < dim; rows of
// `width` doubles.  One wave = 16 rows x 64 columns, K = b: A[row cl][k q] = src[r0 + cl][off + 4 s + q], B[k q][col cl] =
// U[4 s + q][c0 + 16 ct + cl].  grid (ceil(R / 16 * ceil(dim / 64) / 4), members)
__global__ __launch_bounds__(256) void k_kron_rotate(const double* __restrict__ src, double* __restrict__ dst, size_t mstride,
                                                     int R, int width, int off, int dim, const double* __restrict__ U,
                                                     size_t ustride, int square) {
    const int lane = threadIdx.x & 63, q = lane >> 4, cl = lane & 15;
    const int ncg = (dim + 63) / 64;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (R / 16) * ncg) return;
    const int cg = w % ncg, r0 = (w / ncg) * 16, c0 = cg * 64;
    const int ctn = min(4, (dim - c0 + 15) / 16);
    const double* sb = src + blockIdx.y * mstride + (size_t)(r0 + cl) * width + off;
    const double* Ub = U + blockIdx.y * ustride;
    int col[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) col[ct] = min(c0 + 16 * ct + cl, dim - 1);
    dv4 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = (dv4){0.0, 0.0, 0.0, 0.0};
    for (int s = 0; 4 * s < dim; ++s) {
        const int kc = 4 * s + q;
        const bool kv = kc < dim;
        const int kk = min(kc, dim - 1);
        const double a = kv ? sb[kk] : 0.0;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
            if (ct < ctn) acc[ct] = mfma64(a, kv ? Ub[(size_t)kk * dim + col[ct]] : 0.0, acc[ct]);
    }
    double* db = dst + blockIdx.y * mstride + off;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = c0 + 16 * ct + cl;
            if (ct < ctn && c < dim) {
                const double v = acc[ct][r];
                db[(size_t)(r0 + q + 4 * r) * width + c] = square ? v * v : v;
            }
        }
}

// ---- grid (ceil(RT / 64), members), one wave per 16 query rows of the tile.  AH2 [members][RT][EI], GH [members][o][RT][D],
// Dinv [members][p] kron order, cov [members][N][o][o]; the tile holds query rows n0 .. n0 + nrows - 1
__global__ __launch_bounds__(256) void k_kron_glm(CurvArgs g, KronArgs kr, const double* __restrict__ AH2,
                                                  const double* __restrict__ GH, const double* __restrict__ Dinv, int n0,
                                                  int nrows, int N, double* __restrict__ cov) {
    const int lane = threadIdx.x & 63, q = lane >> 4, cl = lane & 15;
    const int rw = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;           // first row of this wave within the tile
    if (rw >= nrows) return;                                             // whole waves leave together
    const int mb = blockIdx.y, o = g.o;
    const size_t kstride = (size_t)g.RT * g.D;
    const double* ah = AH2 + ((size_t)mb * g.RT + rw + cl) * g.EI;       // the row this lane feeds to the A operand (< RT)
    const double* GHb = GH + (size_t)mb * o * kstride;
    const double* Db = Dinv + (size_t)mb * g.p;
    double* covb = cov + (size_t)mb * N * o * o;
    for (int i = 0; i < g.L; ++i) {
        const int e = g.dims[i] + g.hb, h = g.dims[i + 1];
        const double* Di = Db + kr.offK[i];
        for (int a0 = 0; a0 < h; a0 += 64) {
            const int ctn = min(4, (h - a0 + 15) / 16);
            const bool first = i == 0 && a0 == 0, last = i == g.L - 1 && a0 + 64 >= h;
            int col[4];
            bool cv[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                cv[ct] = ct < ctn && a0 + 16 * ct + cl < h;
                col[ct] = min(a0 + 16 * ct + cl, h - 1);
            }
            dv4 acc[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[ct] = (dv4){0.0, 0.0, 0.0, 0.0};
            for (int s = 0; 4 * s < e; ++s) {
                const int kc = 4 * s + q;
                const bool kv = kc < e;
                const int kk = min(kc, e - 1);
                const double a = kv ? ah[g.offIN[i] + kk] : 0.0;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    if (ct < ctn) acc[ct] = mfma64(a, kv ? Di[(size_t)col[ct] * e + kk] : 0.0, acc[ct]);
            }
            // epilogue: cov[n][k][l] += sum over these units of T[n][a] gh^k_a gh^l_a, l >= k.  Every lane runs the same loops
            // (the butterfly needs all 64); only the store is predicated
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = rw + q + 4 * r;                             // < RT: a row of the arrays, zero past nrows
                const bool live = n < nrows;
                const double* gn = GHb + (size_t)n * g.D + g.offG[i];
                for (int k = 0; k < o; ++k) {
                    double tg[4];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) tg[ct] = cv[ct] ? acc[ct][r] * gn[k * kstride + col[ct]] : 0.0;
                    for (int l = k; l < o; ++l) {
                        double v = 0.0;
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct) v = fma(tg[ct], cv[ct] ? gn[l * kstride + col[ct]] : 0.0, v);
                        v += __shfl_xor(v, 1);
                        v += __shfl_xor(v, 2);
                        v += __shfl_xor(v, 4);
                        v += __shfl_xor(v, 8);
                        if (cl == 0 && live) {
                            double* c = covb + ((size_t)(n0 + n) * o + k) * o + l;
                            const double tot = first ? v : *c + v;
                            *c = tot;
                            if (last && l != k) covb[((size_t)(n0 + n) * o + l) * o + k] = tot;
                        }
                    }
                }
            }
        }
    }
}

// ---- grid (panels of 16 input slots over all layers, draws); dynamic LDS: [round16(widest layer)][16] doubles
__global__ __launch_bounds__(256) void k_kron_sample(CurvArgs g, KronArgs kr, const double* __restrict__ mean,
                                                     const double* __restrict__ UA, const double* __restrict__ US,
                                                     const double* __restrict__ Dih, const int32_t* __restrict__ js,
                                                     const double* __restrict__ Z, double* __restrict__ Wout) {
    extern __shared__ double T1s[];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, cl = lane & 15;
    int i = 0;
    while ((int)blockIdx.x >= kr.colStart[i + 1]) ++i;
    const int b0 = ((int)blockIdx.x - kr.colStart[i]) * 16;
    const int e = g.dims[i] + g.hb, h = g.dims[i + 1];
    const int m = blockIdx.y, j = js[m];
    const int64_t P = g.p;
    const double* Zm = Z + (size_t)m * P;
    const double* Dj = Dih + (size_t)j * P + kr.offK[i];
    const double* UAj = UA + (size_t)j * kr.lenA + kr.offA[i];
    const double* USj = US + (size_t)j * kr.lenS + kr.offS[i];
    const int nat = (h + 15) / 16;
    const int brow = min(b0 + cl, e - 1);
    // T1[a][b'] = sum_c Z[a][c] Dih[a][c] U_A[b'][c]: A[row cl][k q] = (Z o Dih)[a0 + cl][4 s + q], B[k q][col cl] = U_A[b0 + cl][4 s + q]
    for (int at = wv; at < nat; at += 4) {
        const int arow = min(at * 16 + cl, h - 1);
        dv4 acc = (dv4){0.0, 0.0, 0.0, 0.0};
        for (int s = 0; 4 * s < e; ++s) {
            const int kc = 4 * s + q;
            const bool kv = kc < e;
            const int kk = min(kc, e - 1);
            const double a = kv ? Zm[param_index(g, i, arow, kk)] * Dj[(size_t)arow * e + kk] : 0.0;
            const double b = kv ? UAj[(size_t)brow * e + kk] : 0.0;
            acc = mfma64(a, b, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) T1s[(at * 16 + q + 4 * r) * 16 + cl] = acc[r];      // rows >= h are never read
    }
    __syncthreads();
    // Y[a'][b'] = sum_a U_S[a'][a] T1[a][b']: A[row cl][k q] = U_S[a0 + cl][4 s + q], B[k q][col cl] = T1[4 s + q][cl]
    for (int at = wv; at < nat; at += 4) {
        const int arow = min(at * 16 + cl, h - 1);
        dv4 acc = (dv4){0.0, 0.0, 0.0, 0.0};
        for (int s = 0; 4 * s < h; ++s) {
            const int kc = 4 * s + q;
            const bool kv = kc < h;
            const double a = kv ? USj[(size_t)arow * h + kc] : 0.0;
            const double b = kv ? T1s[kc * 16 + cl] : 0.0;
            acc = mfma64(a, b, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = at * 16 + q + 4 * r, b = b0 + cl;
            if (a < h && b < e) {
                const int64_t idx = param_index(g, i, a, b);
                Wout[(size_t)m * P + idx] = mean[(size_t)j * P + idx] + acc[r];
            }
        }
    }
}

bool kron_args(const qn_desc* d, CurvArgs* g, KronArgs* kr, const char* who) {
    if (!qn_check_mlp_desc(d, who, "the Kronecker-factored kernels")) return false;
    for (int i = 0; i <= d->nlayers; ++i)
        if (d->dims[i] > KRON_MAX_W) {
            qn_set_error("%s: layer width %d is not supported; the Kronecker-factored kernels take widths up to %d", who,
                         d->dims[i], KRON_MAX_W);
            return false;
        }
    curv_fill_dims(d, g);
    g->RT = 0;
    kron_fill(*g, kr);
    return true;
}

struct KronLayout { size_t in, gk, part, ah, gh, total; };

KronLayout factor_layout(const CurvArgs& g, const KronArgs& kr, int B, int nchunks) {
    KronLayout l = {};
    qn_ws_carver c;
    l.in = c.take_doubles((size_t)B * g.RT * g.EI);
    l.gk = c.take_doubles((size_t)B * g.o * g.RT * g.D);
    l.part = c.take_doubles((size_t)B * nchunks * (size_t)(kr.lenA + kr.lenS));
    l.total = c.total;
    return l;
}

KronLayout glm_layout(const CurvArgs& g, int B) {
    KronLayout l = {};
    qn_ws_carver c;
    l.in = c.take_doubles((size_t)B * g.RT * g.EI);
    l.gk = c.take_doubles((size_t)B * g.o * g.RT * g.D);
    l.ah = c.take_doubles((size_t)B * g.RT * g.EI);
    l.gh = c.take_doubles((size_t)B * g.o * g.RT * g.D);
    l.total = c.total;
    return l;
}

bool factor_sizes(const qn_desc* d, int B, int Nb, CurvArgs* g, KronArgs* kr, int* nchunks, const char* who) {
    if (!kron_args(d, g, kr, who)) return false;
    if (!qn_check_members(B, who)) return false;
    if (Nb <= 0) {
        qn_set_error("%s: need Nb >= 1 rows", who);
        return false;
    }
    g->RT = std::min(KRON_RT, (Nb + 3) / 4 * 4);
    *nchunks = (g->RT + KRON_RC - 1) / KRON_RC;
    return true;
}

bool glm_sizes(const qn_desc* d, int B, int N, CurvArgs* g, KronArgs* kr, const char* who) {
    if (!kron_args(d, g, kr, who)) return false;
    if (!qn_check_members(B, who)) return false;
    if (N <= 0) {
        qn_set_error("%s: need N >= 1 query rows", who);
        return false;
    }
    g->RT = std::min(KRON_GLM_RT, (N + 15) / 16 * 16);
    return true;
}

}  // namespace

extern "C" int qn_kron_layout(const qn_desc* d, int64_t* offA, int64_t* offS, int64_t* offK, int64_t* lenA, int64_t* lenS) {
    CurvArgs g;
    KronArgs kr;
    if (!kron_args(d, &g, &kr, "qn_kron_layout")) return QN_EINVAL;
    for (int i = 0; i < g.L; ++i) {
        if (offA) offA[i] = kr.offA[i];
        if (offS) offS[i] = kr.offS[i];
        if (offK) offK[i] = kr.offK[i];
    }
    if (lenA) *lenA = kr.lenA;
    if (lenS) *lenS = kr.lenS;
    return QN_OK;
}

extern "C" size_t qn_kron_workspace_bytes(const qn_desc* d, int B, int Nb) {
    CurvArgs g;
    KronArgs kr;
    int nchunks;
    if (!factor_sizes(d, B, Nb, &g, &kr, &nchunks, "qn_kron_workspace_bytes")) return 0;
    return factor_layout(g, kr, B, nchunks).total;
}

extern "C" int qn_mlp_kron_factors(const qn_desc* d, const double* W, const double* X, const int32_t* row_idx, int B, int N,
                                   int Nb, double* A_out, double* S_out, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    CurvArgs g;
    KronArgs kr;
    int nchunks;
    if (!factor_sizes(d, B, Nb, &g, &kr, &nchunks, "qn_mlp_kron_factors")) return QN_EINVAL;
    if (N <= 0 || !W || !X || !A_out || !S_out) {
        qn_set_error("qn_mlp_kron_factors: need N >= 1 and non-NULL W, X, A_out, S_out");
        return QN_EINVAL;
    }
    if (!qn_check_row_idx(row_idx, N, Nb, "qn_mlp_kron_factors")) return QN_EINVAL;
    const KronLayout l = factor_layout(g, kr, B, nchunks);
    if (!qn_check_workspace(workspace, workspace_bytes, l.total, "qn_mlp_kron_factors")) return QN_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* IN = qn_ws_at(workspace, l.in);
    double* GK = qn_ws_at(workspace, l.gk);
    double* part = qn_ws_at(workspace, l.part);
    const int nitems = kr.itemStart[2 * g.L];
    const int64_t len = kr.lenA + kr.lenS;
    for (int n0 = 0; n0 < Nb; n0 += g.RT) {
        const int nrows = std::min(g.RT, Nb - n0);
        hipLaunchKernelGGL(k_jac_rows, dim3((g.RT + 255) / 256, B), dim3(256), 0, st, g, W, X, row_idx, (int64_t)Nb, n0, nrows,
                           IN, GK, (double*)nullptr, (int64_t)0);
        QN_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_kron_syrk, dim3((nitems * nchunks + 3) / 4, B), dim3(256), 0, st, g, kr, IN, GK, nchunks, part);
        QN_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_kron_reduce, dim3((unsigned)((len + 255) / 256), B), dim3(256), 0, st, g, kr, part, nchunks,
                           n0 > 0 ? 1 : 0, A_out, S_out);
        QN_HIP_CHECK(hipGetLastError());
    }
    return QN_OK;
}

extern "C" size_t qn_kron_glm_workspace_bytes(const qn_desc* d, int B, int N) {
    CurvArgs g;
    KronArgs kr;
    if (!glm_sizes(d, B, N, &g, &kr, "qn_kron_glm_workspace_bytes")) return 0;
    return glm_layout(g, B).total;
}

extern "C" int qn_mlp_kron_glm_predict(const qn_desc* d, const double* W, const double* X, const double* UA, const double* US,
                                       const double* Dinv, int B, int N, double* mean_out, double* cov_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    CurvArgs g;
    KronArgs kr;
    if (!glm_sizes(d, B, N, &g, &kr, "qn_mlp_kron_glm_predict")) return QN_EINVAL;
    if (!W || !X || !UA || !US || !Dinv || !mean_out || !cov_out) {
        qn_set_error("qn_mlp_kron_glm_predict: need non-NULL W, X, UA, US, Dinv, mean_out, cov_out");
        return QN_EINVAL;
    }
    const KronLayout l = glm_layout(g, B);
    if (!qn_check_workspace(workspace, workspace_bytes, l.total, "qn_mlp_kron_glm_predict")) return QN_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* IN = qn_ws_at(workspace, l.in);
    double* GK = qn_ws_at(workspace, l.gk);
    double* AH = qn_ws_at(workspace, l.ah);
    double* GH = qn_ws_at(workspace, l.gh);
    const size_t inStride = (size_t)g.RT * g.EI, gkStride = (size_t)g.o * g.RT * g.D;
    for (int n0 = 0; n0 < N; n0 += g.RT) {
        const int nrows = std::min(g.RT, N - n0);
        hipLaunchKernelGGL(k_jac_rows, dim3((g.RT + 255) / 256, B), dim3(256), 0, st, g, W, X, (const int32_t*)nullptr,
                           (int64_t)0, n0, nrows, IN, GK, mean_out, (int64_t)N);
        QN_HIP_CHECK(hipGetLastError());
        for (int i = 0; i < g.L; ++i) {
            const int e = g.dims[i] + g.hb, h = g.dims[i + 1];
            const int wa = (g.RT / 16) * ((e + 63) / 64), wsn = (g.o * g.RT / 16) * ((h + 63) / 64);
            hipLaunchKernelGGL(k_kron_rotate, dim3((wa + 3) / 4, B), dim3(256), 0, st, IN, AH, inStride, g.RT, g.EI, g.offIN[i],
                               e, UA + kr.offA[i], (size_t)kr.lenA, 1);
            QN_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_kron_rotate, dim3((wsn + 3) / 4, B), dim3(256), 0, st, GK, GH, gkStride, g.o * g.RT, g.D,
                               g.offG[i], h, US + kr.offS[i], (size_t)kr.lenS, 0);
            QN_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_kron_glm, dim3((g.RT + 63) / 64, B), dim3(256), 0, st, g, kr, AH, GH, Dinv, n0, nrows, N, cov_out);
        QN_HIP_CHECK(hipGetLastError());
    }
    return QN_OK;
}

extern "C" int qn_kron_sample(const qn_desc* d, const double* mean, const double* UA, const double* US, const double* Dih,
                              const int32_t* js, const double* Z, double* W_out, int M, void* stream) {
    CurvArgs g;
    KronArgs kr;
    if (!kron_args(d, &g, &kr, "qn_kron_sample")) return QN_EINVAL;
    if (!mean || !UA || !US || !Dih || !js || !Z || !W_out || M <= 0 || M > 65535) {
        qn_set_error("qn_kron_sample: need non-NULL mean, UA, US, Dih, js, Z, W_out and 1 <= M <= 65535 draws (M=%d)", M);
        return QN_EINVAL;
    }
    int hmax = 0;
    for (int i = 0; i < g.L; ++i) hmax = std::max(hmax, g.dims[i + 1]);
    const size_t lds = (size_t)((hmax + 15) / 16 * 16) * 16 * sizeof(double);          // <= 64 KB at KRON_MAX_W
    hipLaunchKernelGGL(k_kron_sample, dim3(kr.colStart[g.L], M), dim3(256), lds, static_cast<hipStream_t>(stream), g, kr, mean,
                       UA, US, Dih, js, Z, W_out);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
