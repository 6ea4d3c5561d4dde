// Replica exchange (parallel tempering) for the device HMC / MALA engines:
//   qn_pt_swap : one exchange round between neighbouring rungs of every ladder
// The tempered step itself is elsewhere: qn_hmc_begin_t / qn_hmc_leap_t, the leapfrog with the force beta_c * d logpost, in
// qn_hmc_leap.hip; qn_hmc_accept_t, qn_hmc_accept with beta_c in the MH ratio, in qn_mcmc.hip next to the kernel it shares.
// Chains are ladder-major: chain c is rung c % R of ladder c / R, 1 = beta_0 > ... > beta_{R-1}.  Round `round` pairs
// (c, c + 1) for c % R in {e, e + 2, ...}, e = round & 1 (deterministic even-odd scheme); the pair exchanges its states with
// probability min(1, exp((beta_c - beta_{c+1}) (lp_{c+1} - lp_c))), lp the UNTEMPERED log-posteriors.
// Like k_accept the swap kernel is a latency chain, not a bandwidth problem: every workgroup of a pair takes the decision
// itself from slot `par` of the double-buffered scalars (nobody writes that slot in this launch), the element loads of both rows
// are issued before the decision is known, and workgroup 0 of every chain writes slot 1 - par (of rid: slot 1 - rpar; the accept
// kernel does not know rid, so only exchange rounds flip its parity).  Plain vector loads and stores,
// no atomics, no fences.
#include "qn_mcmc_shared.h"

namespace {

struct SwapArgs {
    int R, round, nrounds, C, chain0, nmcmc, par, rpar;
    int64_t p;
    uint64_t seed;
};
constexpr int SBLK = 256;
constexpr int SPT = 2;                    // pairs of elements per thread and pass
constexpr int SPARTS_MAX = 64;

// The two rows of a pair are exchanged IN PLACE: a thread reads its element pairs of both rows into registers (16-byte accesses
// declared 8-byte aligned: a row starts at an odd multiple of 8 bytes for odd c * p) and writes them back crosswise, so no
// element is read after it was written.  The work of a pair is split over its two chains' workgroups: those of the lower chain
// exchange the states (cur, and rewrite the two stored rows of step t), those of the upper chain the cached gradients.
__global__ __launch_bounds__(SBLK) void k_pt_swap(SwapArgs a, double* cur, double* gcur, double* cur_lp, double* best_lp,
                                                  double* lps, double* chain, const double* __restrict__ beta, int32_t* rid,
                                                  int32_t* __restrict__ rep, int64_t* __restrict__ swap_acc,
                                                  int64_t* __restrict__ swap_try, int64_t* step_ptr) {
    const int b = blockIdx.y, part = blockIdx.x;
    const int r = b % a.R, e = a.round & 1;               // (chain0 % R == 0: the rung of the local index is the global one)
    const bool lower = r >= e && ((r - e) & 1) == 0 && r + 1 < a.R;
    const bool upper = r - 1 >= e && ((r - 1 - e) & 1) == 0;          // (then r - e is odd: not `lower`; r < R always)
    const bool paired = lower || upper;
    if (!paired && part != 0) return;
    const int lo = lower ? b : b - 1;                     // the pair's lower chain (meaningless when unpaired)
    const int64_t npair = (a.p + 1) / 2;
    double* rowl = (lower ? cur : gcur) + (int64_t)lo * a.p;
    double* rowh = rowl + a.p;
    d2u lv[SPT], hv[SPT];
    auto load = [&](int64_t pair0) {
#pragma unroll
        for (int h = 0; h < SPT; ++h) {
            const int64_t pair = pair0 + (int64_t)h * SBLK, el = 2 * pair;
            const bool in = paired && pair < npair, both = el + 1 < a.p;
            const d2u zero = {0.0, 0.0};
            lv[h] = in ? ld2(rowl + el, both) : zero;
            hv[h] = in ? ld2(rowh + el, both) : zero;
        }
    };
    // ---- issue: the thread's first pairs of both rows, then the scalars of the pair
    int64_t pair0 = (int64_t)part * (SPT * SBLK) + threadIdx.x;
    load(pair0);
    const int64_t t = step_ptr[a.par];
    const int so = a.par * a.C, sn = (1 - a.par) * a.C;
    const double lpl = paired ? cur_lp[so + lo] : 0.0, lph = paired ? cur_lp[so + lo + 1] : 0.0;
    const double bl = paired ? beta[lo] : 0.0, bh = paired ? beta[lo + 1] : 0.0;
    // ---- the decision (the same numbers in the same order in every workgroup of the pair)
    bool swap = false;
    if (paired) {
        const double d = (bl - bh) * (lph - lpl);
        Philox ph;
        ph.gen(a.seed, 2 * (uint64_t)t + 1, ctr_of(a.chain0 + lo, 6, 0));
        const double u = u01(ph.c[0], ph.c[1]);
        const bool fin = fabs(lpl) < INFINITY && fabs(lph) < INFINITY;       // a NaN or infinite log-posterior never moves
        swap = fin && u < exp(d);                                            // (NaN -> no swap)
    }
    const bool tin = t >= 0 && t <= a.nmcmc;
    if (swap) {
        // the stored row of step t is the state step t + 1 starts from: rewritten with the exchanged states
        double* crl = (lower && chain && tin) ? chain + ((int64_t)lo * (a.nmcmc + 1) + t) * a.p : nullptr;
        double* crh = crl ? crl + (int64_t)(a.nmcmc + 1) * a.p : nullptr;
        const int64_t stride = (int64_t)gridDim.x * (SPT * SBLK);
        while (pair0 < npair) {
#pragma unroll
            for (int h = 0; h < SPT; ++h) {
                const int64_t pair = pair0 + (int64_t)h * SBLK, el = 2 * pair;
                if (pair >= npair) break;
                const bool both = el + 1 < a.p;
                st2(rowl + el, hv[h].x, hv[h].y, both);
                st2(rowh + el, lv[h].x, lv[h].y, both);
                if (crl) {
                    st2(crl + el, hv[h].x, hv[h].y, both);
                    st2(crh + el, lv[h].x, lv[h].y, both);
                }
            }
            pair0 += stride;
            if (pair0 < npair) load(pair0);                                  // (p > 2 * SPT * SPARTS_MAX * SBLK: further passes)
        }
    }
    if (part == 0 && threadIdx.x == 0) {
        const int src = swap ? (lower ? b + 1 : b - 1) : b;                  // the slot whose replica this chain holds now
        const double nlp = cur_lp[so + src];
        const int32_t nr = rid[a.rpar * a.C + src];             // rid has a parity of its own: no accept call carries it over
        cur_lp[sn + b] = nlp;
        best_lp[sn + b] = best_lp[so + b];                                   // the MAP stays with the chain slot
        rid[(1 - a.rpar) * a.C + b] = nr;
        if (rep) rep[(int64_t)b * (a.nrounds + 1) + a.round + 1] = nr;
        if (swap && tin) lps[(int64_t)b * (a.nmcmc + 1) + t] = nlp;
        if (lower) {
            swap_try[b] += 1;
            if (swap) swap_acc[b] += 1;
        }
        if (b == 0) step_ptr[1 - a.par] = t;                                 // no step was taken: the caller only flips its parity
    }
}

int swap_parts(int64_t p) {
    const int64_t n = ((p + 1) / 2 + SPT * SBLK - 1) / (SPT * SBLK);
    return n > SPARTS_MAX ? SPARTS_MAX : (n < 1 ? 1 : (int)n);
}

}  // namespace

extern "C" int qn_pt_swap(double* cur, double* grad_cur, double* cur_lp, double* best_lp, double* lps, double* chain,
                          const double* beta, int32_t* rid, int32_t* rep, int64_t* swap_acc, int64_t* swap_try,
                          int64_t* step_ptr, int R, int round, int nrounds, int C, int chain0, int64_t p, int nmcmc,
                          uint64_t seed, int parity, int rid_parity, void* stream) {
    if (R < 2) {
        qn_set_error("qn_pt_swap: a ladder has R >= 2 rungs (R = %d)", R);
        return QN_EINVAL;
    }
    if (C <= 0 || C > 65535 || C % R != 0 || chain0 < 0 || chain0 % R != 0) {
        qn_set_error("qn_pt_swap: C = %d chains from chain0 = %d are not whole ladders of R = %d rungs (1 <= C <= 65535)", C,
                     chain0, R);
        return QN_EINVAL;
    }
    if (p <= 0 || nmcmc < 1 || round < 0 || nrounds < 1 || round >= nrounds || (parity != 0 && parity != 1) ||
        (rid_parity != 0 && rid_parity != 1)) {
        qn_set_error("qn_pt_swap: bad size (p >= 1, nmcmc >= 1, 0 <= round < nrounds, parity and rid_parity 0 or 1)");
        return QN_EINVAL;
    }
    if (!cur || !grad_cur || !cur_lp || !best_lp || !lps || !beta || !rid || !swap_acc || !swap_try || !step_ptr) {
        qn_set_error("qn_pt_swap: a required pointer is NULL (only chain and rep are optional)");
        return QN_EINVAL;
    }
    SwapArgs a;
    a.R = R; a.round = round; a.nrounds = nrounds; a.C = C; a.chain0 = chain0; a.nmcmc = nmcmc; a.par = parity; a.rpar = rid_parity; a.p = p;
    a.seed = seed;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_pt_swap, dim3(swap_parts(p), C), dim3(SBLK), 0, static_cast<hipStream_t>(stream), a, cur, grad_cur,
                       cur_lp, best_lp, lps, chain, beta, rid, rep, swap_acc, swap_try, step_ptr);
    QN_HIP_CHECK(hipGetLastError());
    return QN_OK;
}
