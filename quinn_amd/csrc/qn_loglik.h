// The member log density of the scoring kernels (qn_score.hip, qn_psis.hip): ll = log N(y; f, s^2) with its roundings carried
// along, so that both files form the same bits from the same inputs.  Internal linkage.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr double LOG_2PI_HI = 1.8378770664093453, LOG_2PI_LO = 1.0549287138283958e-16;      // log(2 pi) = HI + LO

// s = a + b rounded and the rounding's exact error (Knuth)
__device__ __forceinline__ double two_sum(double a, double b, double* err) {
    const double s = a + b, bb = s - a;
    *err = (a - (s - bb)) + (b - bb);
    return s;
}

// log(2 pi s^2) = g + gc for s^2 = s2h + s2l (|s2l| far below s2h): gc collects the roundings, so that what is left is the
// error of log() itself.  inv = 1 / s2h.
struct LogNorm {
    double s2h, s2l, inv, g, gc;
};
__device__ __forceinline__ LogNorm log_norm(double s2h, double s2l) {
    LogNorm n;
    n.s2h = s2h;
    n.s2l = s2l;
    n.inv = 1.0 / s2h;
    double ge;
    n.g = two_sum(LOG_2PI_HI, log(s2h), &ge);
    n.gc = ge + LOG_2PI_LO + s2l * n.inv;
    return n;
}

// ll = -0.5 ((y - f)^2 / s^2 + log(2 pi s^2)) with the roundings of the residual, its square, the quotient and the sum
// carried along: the quadratic and the log term can cancel (s^2 < 1 / (2 pi)), and ll is then far smaller than either, so
// their own float64 roundings would be large relative to ll.  A residual whose square overflows gives -inf.
__device__ __forceinline__ double log_lik(double y, double f, const LogNorm& n) {
    double rl, ae;
    const double r = two_sum(y, -f, &rl);
    const double p = r * r, qh = p * n.inv;
    const double pe = fma(r, r, -p) + 2.0 * r * rl;
    const double qc = (fma(-qh, n.s2h, p) + pe - qh * n.s2l) * n.inv;
    const double a = two_sum(qh, n.g, &ae);
    const double c = fabs(qh) < 1e300 ? ae + qc + n.gc : 0.0;
    return -0.5 * (a + c);
}

}  // namespace
