// SWAG (Stochastic Weight Averaging Gaussian, reference quinn/solvers/nn_swag.py), float64 state:
//   qn_swag_step    one SGD step of B members, fused with the running-moment / deviation update of swag_calc
//                   (nn_swag.py:86-123):   w <- w - lr[b] * (G * gscale)
//                                          m1 <- (n m1 + w) / (n + 1),  m2 <- (n m2 + w^2) / (n + 1),  D[b][slot] <- w - m1
//   qn_swag_sample  M posterior draws theta_s = mean_{js[s]} + corr_s (nn_swag.py:125-145) with
//                   corr = sqrt(.5) (sqrt(diag) z1) + sqrt(.5) (D z2) / sqrt(K - 1)   (lowrank)   or   sqrt(diag) z1
//                   and, with drift, the reference's in-place update mean_{js[s]} <- theta_s in sample order.
//
// Bit-exactness: every expression is evaluated in the reference's (numpy's) order with one rounding per operation.  FP
// contraction is off for the whole file (hipcc would fuse n * m1 + w into an fma); `/` and sqrt are the IEEE-correct
// float64 operations (no fast-math, no reciprocal approximations).  The only sum whose order differs from numpy's is the
// K-term D z2 of the sampler (BLAS sums in its own order).  No atomics: each output element has exactly one writer.
#include <algorithm>
#include <cmath>

#include "qn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SBLK = 256;

// the update of one parameter; numpy's order of operations (np.power(w, 2) is w * w)
struct SwagElem {
    double nd, n1, lr;
    __device__ __forceinline__ void init(double w, double& m1, double& m2) const {
        m1 = w;
        m2 = w * w;
    }
    __device__ __forceinline__ double sgd(double w, double g) const { return w - lr * g; }
    __device__ __forceinline__ double collect(double w, double& m1, double& m2) const {
        m1 = (nd * m1 + w) / n1;
        m2 = (nd * m2 + w * w) / n1;
        return w - m1;
    }
};

template <typename T> struct Vec2;
template <> struct Vec2<double> { using type = double2; };
template <> struct Vec2<float> { using type = float2; };

template <int MODE, typename T>
__device__ __forceinline__ void swag_one(const SwagElem& e, double gscale, double* W, const T* G, double* m1, double* m2,
                                         double* Drow, int64_t k, int64_t i) {
    double w = W[k];
    if (MODE == QN_SWAG_INIT) {
        double a, b;
        e.init(w, a, b);
        m1[k] = a;
        m2[k] = b;
        return;
    }
    w = e.sgd(w, (double)G[k] * gscale);
    W[k] = w;
    if (MODE == QN_SWAG_SGD_COLLECT) {
        double a = m1[k], b = m2[k];
        const double dv = e.collect(w, a, b);
        m1[k] = a;
        m2[k] = b;
        if (Drow) Drow[i] = dv;
    }
}

// grid (x: parameter blocks, y: member).  VEC: every base pointer is 16-B aligned (8-B for float G), so within a row the
// pairs starting at an even flat offset load as double2 / float2; a row of odd start has one head element, a row of odd
// remaining length one tail element, both done by lanes of block x = 0.  D rows (offset (b K + slot) p) can have the
// other parity: their pair is then written as two scalars.
template <int MODE, typename T, bool VEC>
__global__ __launch_bounds__(SBLK) void k_swag_step(double* __restrict__ W, const T* __restrict__ G,
                                                    const double* __restrict__ lr, double gscale, double* __restrict__ m1,
                                                    double* __restrict__ m2, double* __restrict__ D, int K, int slot,
                                                    double nd, int64_t p) {
    const int b = blockIdx.y;
    SwagElem e;
    e.nd = nd;
    e.n1 = nd + 1.0;
    e.lr = MODE == QN_SWAG_INIT ? 0.0 : lr[b];
    const int64_t off = (int64_t)b * p;
    double* Drow = (MODE == QN_SWAG_SGD_COLLECT && D) ? D + ((int64_t)b * K + slot) * p : nullptr;
    const int64_t tid = (int64_t)blockIdx.x * SBLK + threadIdx.x, stride = (int64_t)gridDim.x * SBLK;
    if (!VEC) {
        for (int64_t i = tid; i < p; i += stride) swag_one<MODE, T>(e, gscale, W, G, m1, m2, Drow, off + i, i);
        return;
    }
    const int64_t h = off & 1;                           // head element before the first aligned pair
    const int64_t npairs = (p - h) >> 1;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 && h) swag_one<MODE, T>(e, gscale, W, G, m1, m2, Drow, off, 0);
        if (threadIdx.x == 1 && h + 2 * npairs < p) swag_one<MODE, T>(e, gscale, W, G, m1, m2, Drow, off + p - 1, p - 1);
    }
    const bool dvec = Drow && ((((int64_t)b * K + slot) * p + h) & 1) == 0;
    using T2 = typename Vec2<T>::type;
    for (int64_t q = tid; q < npairs; q += stride) {
        const int64_t i = h + 2 * q, k = off + i;
        double2 w = *reinterpret_cast<const double2*>(W + k);
        if (MODE == QN_SWAG_INIT) {
            double2 a, c;
            e.init(w.x, a.x, c.x);
            e.init(w.y, a.y, c.y);
            *reinterpret_cast<double2*>(m1 + k) = a;
            *reinterpret_cast<double2*>(m2 + k) = c;
            continue;
        }
        const T2 g = *reinterpret_cast<const T2*>(G + k);
        w.x = e.sgd(w.x, (double)g.x * gscale);
        w.y = e.sgd(w.y, (double)g.y * gscale);
        *reinterpret_cast<double2*>(W + k) = w;
        if (MODE == QN_SWAG_SGD_COLLECT) {
            double2 a = *reinterpret_cast<const double2*>(m1 + k), c = *reinterpret_cast<const double2*>(m2 + k);
            double2 dv;
            dv.x = e.collect(w.x, a.x, c.x);
            dv.y = e.collect(w.y, a.y, c.y);
            *reinterpret_cast<double2*>(m1 + k) = a;
            *reinterpret_cast<double2*>(m2 + k) = c;
            if (dvec) {
                *reinterpret_cast<double2*>(Drow + i) = dv;
            } else if (Drow) {
                Drow[i] = dv.x;
                Drow[i + 1] = dv.y;
            }
        }
    }
}

__device__ __forceinline__ double swag_corr(const double* __restrict__ diag, const double* __restrict__ Dj,
                                            const double* __restrict__ z1s, const double* __restrict__ z2s, int K,
                                            int64_t p, int64_t i, double s5, double sk) {
    const double c = sqrt(diag[i]) * z1s[i];
    if (!Dj) return c;
    double dz = 0.0;
    for (int k = 0; k < K; ++k) dz = dz + Dj[(int64_t)k * p + i] * z2s[k];
    return s5 * c + (s5 * dz) / sk;
}

// drift: one thread per parameter walks the samples in order, so mean_j carries every earlier draw of member j
__global__ __launch_bounds__(SBLK) void k_swag_sample_drift(double* __restrict__ mean, const double* __restrict__ diag,
                                                            const double* __restrict__ D, int K,
                                                            const int32_t* __restrict__ js, const double* __restrict__ z1,
                                                            const double* __restrict__ z2, int M, int B, int64_t p,
                                                            double s5, double sk, double* __restrict__ theta) {
    const int64_t i = (int64_t)blockIdx.x * SBLK + threadIdx.x;
    if (i >= p) return;
    for (int s = 0; s < M; ++s) {
        const int j = js[s];
        if (j < 0 || j >= B) {                           // the host checks the indices; never read outside the arrays
            theta[(int64_t)s * p + i] = __builtin_nan("");
            continue;
        }
        const int64_t jo = (int64_t)j * p;
        const double c = swag_corr(diag + jo, D ? D + jo * K : nullptr, z1 + (int64_t)s * p, z2 ? z2 + (int64_t)s * K : nullptr,
                                   K, p, i, s5, sk);
        const double t = mean[jo + i] + c;
        mean[jo + i] = t;
        theta[(int64_t)s * p + i] = t;
    }
}

// no drift: every draw is centred on the collected mean; samples are independent (grid y strides over them)
__global__ __launch_bounds__(SBLK) void k_swag_sample(const double* __restrict__ mean, const double* __restrict__ diag,
                                                      const double* __restrict__ D, int K, const int32_t* __restrict__ js,
                                                      const double* __restrict__ z1, const double* __restrict__ z2, int M,
                                                      int B, int64_t p, double s5, double sk, double* __restrict__ theta) {
    for (int s = blockIdx.y; s < M; s += gridDim.y) {
        const int j = js[s];
        for (int64_t i = (int64_t)blockIdx.x * SBLK + threadIdx.x; i < p; i += (int64_t)gridDim.x * SBLK) {
            if (j < 0 || j >= B) {
                theta[(int64_t)s * p + i] = __builtin_nan("");
                continue;
            }
            const int64_t jo = (int64_t)j * p;
            const double c = swag_corr(diag + jo, D ? D + jo * K : nullptr, z1 + (int64_t)s * p,
                                       z2 ? z2 + (int64_t)s * K : nullptr, K, p, i, s5, sk);
            theta[(int64_t)s * p + i] = mean[jo + i] + c;
        }
    }
}

bool aligned(const void* ptr, uintptr_t a) { return ptr == nullptr || (reinterpret_cast<uintptr_t>(ptr) % a) == 0; }

template <int MODE, typename T>
void launch_step(dim3 grid, hipStream_t st, bool vec, double* W, const T* G, const double* lr, double gscale, double* m1,
                 double* m2, double* D, int K, int slot, double nd, int64_t p) {
    if (vec)
        hipLaunchKernelGGL((k_swag_step<MODE, T, true>), grid, dim3(SBLK), 0, st, W, G, lr, gscale, m1, m2, D, K, slot, nd, p);
    else
        hipLaunchKernelGGL((k_swag_step<MODE, T, false>), grid, dim3(SBLK), 0, st, W, G, lr, gscale, m1, m2, D, K, slot, nd, p);
}

}  // namespace

extern "C" int qn_swag_step(int mode, double* W, const void* G, int gdtype, const double* lr, double gscale, double* m1,
                            double* m2, double* D, int K, int slot, int64_t n, int B, int64_t p, void* stream) {
    if (mode != QN_SWAG_INIT && mode != QN_SWAG_SGD && mode != QN_SWAG_SGD_COLLECT) {
        qn_set_error("qn_swag_step: mode %d (QN_SWAG_INIT, QN_SWAG_SGD or QN_SWAG_SGD_COLLECT)", mode);
        return QN_EINVAL;
    }
    if (!W || B <= 0 || B > 65535 || p <= 0) {
        qn_set_error("qn_swag_step: need W and 1 <= B <= 65535, p >= 1 (B=%d p=%lld)", B, (long long)p);
        return QN_EINVAL;
    }
    if (mode != QN_SWAG_SGD && (!m1 || !m2)) {
        qn_set_error("qn_swag_step: mode %d needs m1 and m2", mode);
        return QN_EINVAL;
    }
    if (mode != QN_SWAG_INIT && (!G || !lr || (gdtype != QN_F64 && gdtype != QN_F32))) {
        qn_set_error("qn_swag_step: an SGD step needs G, lr and a G dtype of QN_F64 or QN_F32 (got %d)", gdtype);
        return QN_EINVAL;
    }
    if (mode == QN_SWAG_SGD_COLLECT && (n < 1 || n > (int64_t(1) << 52))) {
        qn_set_error("qn_swag_step: collection count n = %lld (need 1 <= n <= 2^52)", (long long)n);
        return QN_EINVAL;
    }
    if (mode == QN_SWAG_SGD_COLLECT && D && (K < 1 || slot < 0 || slot >= K)) {
        qn_set_error("qn_swag_step: ring slot %d outside [0, K=%d)", slot, K);
        return QN_EINVAL;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool f32 = mode != QN_SWAG_INIT && gdtype == QN_F32;
    const bool vec = aligned(W, 16) && aligned(m1, 16) && aligned(m2, 16) && aligned(D, 16) && aligned(G, f32 ? 8 : 16);
    const int64_t per_row = vec ? (p + 1) / 2 : p;
    int64_t nx = (per_row + SBLK - 1) / SBLK;
    const int64_t cap = std::max<int64_t>(1, 8192 / B);   // ~8k blocks in all; the rest is grid-strided
    if (nx > cap) nx = cap;
    dim3 grid((unsigned)nx, (unsigned)B);
    const double nd = (double)n;
    (void)hipGetLastError();
    if (mode == QN_SWAG_INIT)
        launch_step<QN_SWAG_INIT, double>(grid, st, vec, W, nullptr, nullptr, 0.0, m1, m2, nullptr, 0, 0, 0.0, p);
    else if (mode == QN_SWAG_SGD && !f32)
        launch_step<QN_SWAG_SGD, double>(grid, st, vec, W, (const double*)G, lr, gscale, m1, m2, nullptr, 0, 0, 0.0, p);
    else if (mode == QN_SWAG_SGD)
        launch_step<QN_SWAG_SGD, float>(grid, st, vec, W, (const float*)G, lr, gscale, m1, m2, nullptr, 0, 0, 0.0, p);
    else if (!f32)
        launch_step<QN_SWAG_SGD_COLLECT, double>(grid, st, vec, W, (const double*)G, lr, gscale, m1, m2, D, K, slot, nd, p);
    else
        launch_step<QN_SWAG_SGD_COLLECT, float>(grid, st, vec, W, (const float*)G, lr, gscale, m1, m2, D, K, slot, nd, p);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}

extern "C" int qn_swag_sample(double* mean, const double* diag, const double* D, int K, const int32_t* js,
                              const double* z1, const double* z2, int M, int B, int64_t p, int drift, double* theta,
                              void* stream) {
    if (!mean || !diag || !js || !z1 || !theta || M <= 0 || B <= 0 || p <= 0 || (drift != 0 && drift != 1)) {
        qn_set_error("qn_swag_sample: need mean, diag, js, z1, theta, M >= 1, B >= 1, p >= 1, drift 0 or 1 "
                     "(M=%d B=%d p=%lld drift=%d)", M, B, (long long)p, drift);
        return QN_EINVAL;
    }
    if (D && (K < 2 || !z2)) {
        qn_set_error("qn_swag_sample: the low-rank term needs K >= 2 (it divides by sqrt(K - 1)) and z2 (K=%d)", K);
        return QN_EINVAL;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double s5 = std::sqrt(0.5), sk = D ? std::sqrt((double)(K - 1)) : 1.0;
    const int64_t nx = (p + SBLK - 1) / SBLK;
    (void)hipGetLastError();
    if (drift) {
        if (nx > 0x7fffffff) {
            qn_set_error("qn_swag_sample: p = %lld too large", (long long)p);
            return QN_EINVAL;
        }
        hipLaunchKernelGGL(k_swag_sample_drift, dim3((unsigned)nx), dim3(SBLK), 0, st, mean, diag, D, K, js, z1, z2, M, B,
                           p, s5, sk, theta);
    } else {
        const unsigned gx = (unsigned)std::min<int64_t>(nx, 1024), gy = (unsigned)std::min(M, 65535);
        hipLaunchKernelGGL(k_swag_sample, dim3(gx, gy), dim3(SBLK), 0, st, mean, diag, D, K, js, z1, z2, M, B, p, s5, sk,
                           theta);
    }
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
