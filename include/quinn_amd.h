/* quinn_amd.h -- C ABI of the MI355X (gfx950) hot path for QUiNN.
 *
 * The reference (sandialabs/quinn) is pure Python and has no FFI layer; its operator
 * boundaries for this path are Python callables.  Each entry point below replaces the
 * inner loop behind one of them and is what a ctypes binding in the reference would call
 * (INTEGRATION.md shows the stubs).  Citations are file:line relative to the reference.
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is a BORROWED DEVICE pointer
 *     (HIP), never allocated or freed across this boundary;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is
 *     enqueued on it, no call synchronises the device;
 *   - return value: QN_OK (0) or a negative QN_E* code; qn_last_error() gives the text
 *     of the calling thread's last failure;
 *   - dtype: QN_F64 (the reference's arithmetic, quinn/nns/tchutils.py:9) or QN_F32.
 *
 * Flat parameter layout of one weight vector (quinn/nns/nnwrap.py:70-77, i.e.
 * module.parameters() order of quinn/nns/mlp.py:55-84):
 *   [ W_0 (h_1 x d, row-major), b_0 (h_1), W_1 (h_2 x h_1), b_1, ..., W_L (o x h_L), b_L ]
 */
#ifndef QUINN_AMD_H
#define QUINN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { QN_F64 = 0, QN_F32 = 1 };
enum { QN_ACT_IDENTITY = 0, QN_ACT_TANH = 1, QN_ACT_RELU = 2 };
enum { QN_OK = 0, QN_EINVAL = -1, QN_EWORKSPACE = -2, QN_EHIP = -3, QN_EUNSUPPORTED = -4 };
/* kernel families, for qn_mlp_desc_set_path (tests / profiling) */
enum { QN_PATH_AUTO = 0, QN_PATH_GENERIC = 1, QN_PATH_FUSED = 2, QN_PATH_FUSED_DP = 3 };

typedef struct qn_desc qn_desc;

/* Architecture descriptor of a quinn-style MLP: dims = {d, h_1, ..., h_L, o} (ndims >= 2),
 * one activation between consecutive Linear layers, none after the last
 * (quinn/nns/mlp.py:46-84: 'tanh' | 'relu' | identity). */
int qn_mlp_desc_create(const int* dims, int ndims, int act, int has_bias, qn_desc** out);
/* Descriptor of a quinn residual network (quinn/nns/rnet.py:16-165):
 *   out = act(Wpre x + bpre)                       if layer_pre, else out = x (indim == rdim)
 *   for i in 0..nsteps-1:  W_i = sum_k coef[i*npar+k] * ww_k,  b_i likewise from bb_k (if has_bias)
 *       out = mlp ? act(W_i out + b_i) : out + (1/nsteps) * act(W_i out + b_i)
 *   pred = Wpost out + bpost                       if layer_post, else pred = out (outdim == rdim)
 * nsteps = nlayers + 1 of the reference; coef[i][k] is the weight-parameterisation function
 * (rnet.py:217-380) evaluated at t = i / nsteps: t^k for Const/Lin/Quad/Cubic/Poly, a one-hot at
 * int(t * npar) for NonPar.  act = tanh (nonlin=True) or identity.  Flat layout = the module's
 * parameters() order: weight_pre, bias_pre, weight_post, bias_post, ww_0.., bb_0.. (rnet.py:90-120).
 * The descriptor is used with the same qn_mlp_* entry points as an MLP's. */
int qn_rnet_desc_create(int indim, int rdim, int outdim, int nsteps, int npar, const double* coef, int act,
                        int has_bias, int layer_pre, int layer_post, int mlp, qn_desc** out);
/* uses[i*npar+k] = 0: parameter tensor k does not enter step i at all (NonPar, rnet.py:349-377, picks ONE tensor per step:
 * `pars[int(t * npar)]`); such a tensor is skipped -- its value, even Inf or NaN, has no effect on the step and its
 * gradient receives nothing from it -- where a tensor with uses = 1 and coefficient 0 (the t^k of Lin / Quad / Cubic / Poly at
 * t = 0, which the reference multiplies out) contributes 0 * value.  Default: every entry 1.  n = nsteps * npar; an entry
 * marked unused must have coefficient 0. */
int qn_rnet_desc_set_uses(qn_desc* desc, const unsigned char* uses, int n);
int qn_mlp_desc_destroy(qn_desc* desc);
/* p = number of entries of one flat weight vector. */
int64_t qn_mlp_num_params(const qn_desc* desc);

/* Bytes of scratch the two calls below need for B weight vectors x Nb rows each.  The workspace is the caller's: it needs
 * no initialisation and keeps no state between calls (the fused forward kernels sum a chain's SSE by a last-arriver
 * protocol on a tagged word of it that treats any other content as "fresh" and resets itself), but it must not be shared by
 * calls that can run concurrently (two streams: two workspaces). */
size_t qn_workspace_bytes(const qn_desc* desc, int B, int Nb, int want_grad, int dtype);

/* Which kernel family the next call with these sizes would run (QN_PATH_GENERIC/FUSED). */
int qn_mlp_path(const qn_desc* desc, int B, int Nb, int want_grad, int dtype);
/* Which ARITHMETIC the next call with these sizes would form the hidden-layer products in: QN_ARITH_PLAIN -- the arithmetic
 * of `dtype` throughout; QN_ARITH_I8_FUSED -- sliced exact int8 products in the one-launch kernels of 64-wide networks
 * (qn_fused_i8.hip / qn_fused_bwd_i8.hip; also a narrower network's zero-padded 64-wide twin); QN_ARITH_I8_WIDE -- the
 * int8-slice kernels of 128 / 256-wide networks (qn_wide_i8.hip; tanh also qn_dw_i8.hip); QN_ARITH_I8_LAYERS -- the layer-wise
 * int8-slice forward of other tanh networks whose widths are multiples of 64.  (The reference has one arithmetic, torch
 * float64: quinn/nns/tchutils.py:9; tests use this query to prove which kernels a parity case exercised.) */
enum { QN_ARITH_PLAIN = 0, QN_ARITH_I8_FUSED = 1, QN_ARITH_I8_WIDE = 2, QN_ARITH_I8_LAYERS = 3 };
int qn_mlp_arith(const qn_desc* desc, int B, int Nb, int want_grad, int dtype);
/* Force a kernel family for the calls made with THIS descriptor (QN_PATH_AUTO restores dispatch by shape).  Returns
 * the previous setting.  There is no process-wide state: two operators in one process do not see each other's
 * choice.  QN_PATH_GENERIC is the layer-wise family at the EXACT layer widths; under QN_PATH_AUTO hidden widths that
 * are no multiples of 64 run on a zero-padded twin of the network (padded units stay exactly 0, results equal the
 * unpadded network's).  QN_PATH_FUSED_DP is QN_PATH_FUSED restricted to the kernels that use the float64 matrix
 * instructions: it excludes the forward kernel that forms the 64-wide hidden layers as sliced exact int8 products
 * (same results to ~1e-14 relative; kept selectable as the second implementation the tests compare it with).  Under
 * QN_PATH_AUTO the float64 networks with hidden widths all 128 or all 256 (one output, <= 8 inputs) take the layer-wise
 * family with their hidden layers -- forward, activation gradient and, for tanh, weight gradient -- as sliced exact int8
 * products (~1e-13 relative; relu / identity: one activation scale per data row and layer, and every weight and bias below
 * 2^20, inputs below 2^100); QN_PATH_GENERIC is the all-float64 reference of that family as well.
 * Shapes of the one-launch (QN_PATH_FUSED) kernels: uniform hidden width 16 / 32 / 64 (any width <= 64 through the twin), up to
 * 4 (64-wide: 3) hidden layers in a gradient call; forward and gradient: up to 16 inputs and 16 outputs (gradient of three
 * 64-wide hidden layers: not more than 4 inputs together with more than 4 outputs).  Everything else runs layer-wise.
 * Accuracy of the int8-slice kernels: operands are rounded to 2^-47 of (1 x the weight row's maximum), the products are
 * exact -- a norm-wise bound, 47-bit against float64's 53; rows whose activations are all below ~2^-5 and chains with a
 * hidden-matrix weight >= 2^20 (or not finite) are computed in plain float64 instead.
 * Not-finite values, every family: SSE, predictions and gradient carry the NaN / +Inf / -Inf pattern of the reference's
 * torch ops on the same inputs (relu(NaN) = NaN, relu backward is a select, tanh saturates an infinite input); a gradient
 * entry that is +-Inf there may be NaN here.  Chains of a zero-padded twin with an unbounded weight or input are recomputed
 * from the original weights (slow). */
int qn_mlp_desc_set_path(qn_desc* desc, int path);

/* The fused kernels give every chain ceil(512 / B) (gradient: 256 / B) workgroups, each summing its share of the data rows;
 * the per-chain SSE / gradient adds those shares left to right, so its last bits depend on B.  batch > 0: split as a launch
 * of max(B, batch) chains would -- a set of chains run as several smaller launches (the chain groups of the device samplers,
 * quinn_amd/mcmc/device_amcmc.py: one group's accept kernel overlaps the other's forward) then reproduces the one-launch
 * results bit for bit.  0 (default): by the launch's own B.  Returns the previous value. */
int qn_mlp_desc_set_plan_batch(qn_desc* desc, int batch);

/* sse_out[b] = sum_{n,o} (Y[r(b,n),o] - f_{W[b]}(X[r(b,n),:])[o])^2 for b < B.
 * Replaces the per-weight-vector loop over NN_MCMC.logpost -> NNWrap.calc_loss ->
 * NegLogPost.forward -> MLP.forward (quinn/solvers/nn_mcmc.py:45-71,
 * quinn/nns/nnwrap.py:109-126, quinn/nns/losses.py:197-198, quinn/nns/mlp.py:92-101), the
 * per-sample loop of BNet.sample_elbo (quinn/vi/bnet.py:202-205) and the forward of one
 * ensemble member's loss in nnfit (quinn/nns/nnfit.py:133-140); with pred_out also
 * nn_p / Learner.predict (quinn/nns/nnwrap.py:330-347, quinn/ens/learner.py:75-93).
 *   W        [B, p]   dtype, row-major flat weight vectors (layout above)
 *   X        [N, d]   dtype, row-major shared dataset
 *   Y        [N, o]   dtype
 *   row_idx  [B, Nb]  int32 or NULL. NULL: Nb must equal N and r(b,n) = n (all vectors see
 *                     the whole dataset); else r(b,n) = row_idx[b*Nb+n] (per-member
 *                     minibatch / data subset, quinn/nns/nnfit.py:131, nn_ens.py:63-64)
 *   sse_out  [B]      float64 always
 *   pred_out [B, Nb, o] dtype or NULL
 * The scalar tails (log-posterior, NLL, MSE) are applied by the caller in float64. */
int qn_mlp_sse_fwd(const qn_desc* desc, int dtype, const void* W, const void* X, const void* Y,
                   const int32_t* row_idx, int B, int N, int Nb, double* sse_out, void* pred_out,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The forward call without its final summation kernel, for a consumer that sums a handful of numbers itself
 * (qn_mcmc_accept): sse_parts_out is [B, parts], parts = qn_mlp_sse_parts(desc, B, Nb, dtype) >= 1, and the plain
 * left-to-right sum of row b is exactly (bit for bit) what qn_mlp_sse_fwd writes to sse_out[b].  parts > 1 only where
 * the fused forward kernel runs unpadded (one partial per row split of a chain); otherwise parts = 1 and the call is
 * qn_mlp_sse_fwd without predictions.  (qn_mlp_sse_fwd itself sums the parts inside the forward kernel since round 3 -- the
 * last workgroup of a chain to finish, ~1.5 us; this entry point saves that as well.) */
int qn_mlp_sse_parts(const qn_desc* desc, int B, int Nb, int dtype);
int qn_mlp_sse_fwd_parts(const qn_desc* desc, int dtype, const void* W, const void* X, const void* Y,
                         const int32_t* row_idx, int B, int N, int Nb, double* sse_parts_out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* As above plus gradW_out[b, :] = d sse_out[b] / d W[b, :]  ([B, p] dtype).  Replaces
 * NN_MCMC.logpostgrad -> NNWrap.calc_lossgrad (quinn/solvers/nn_mcmc.py:73-98,
 * quinn/nns/nnwrap.py:128-150) and loss.backward() in nnfit (quinn/nns/nnfit.py:163-165). */
int qn_mlp_sse_fwdbwd(const qn_desc* desc, int dtype, const void* W, const void* X, const void* Y,
                      const int32_t* row_idx, int B, int N, int Nb, double* sse_out, void* pred_out,
                      void* gradW_out, void* workspace, size_t workspace_bytes, void* stream);

/* Mean-field Gaussian VI, sampling + KL terms (quinn/vi/bnet.py:142-163,
 * quinn/rvar/rvs.py:96-127, 159-173; sigma = exp(rho), bnet.py:80):
 *   W_out[s,i]  = mu[i] + exp(rho[i]) * eps[s,i]                          [S, p] dtype
 *   logq_out[s] = sum_i( -log sqrt(2 pi) - rho[i] - (w-mu)^2 / (2 sigma^2) )   float64
 *   logp_out[s] = sum_i log( pi N(w;0,sigma1) + (1-pi) N(w;0,sigma2) )          float64
 * mu, rho: [p] float64 (the variational parameters stay float64); eps: [S, p] float64. */
int qn_vi_sample_kl(const double* mu, const double* rho, const double* eps, int S, int64_t p,
                    double pi, double sigma1, double sigma2, int dtype, void* W_out,
                    double* logq_out, double* logp_out, void* stream);

/* Chain rule of viloss = (mean_s logq - mean_s logp) * kl_scale + NLL  (bnet.py:229-232)
 * to (mu, rho), given gW[s,:] = d NLL / d W[s,:] * gw_scale taken from qn_mlp_sse_fwdbwd
 * (gw_scale = 0.5 / (S * o * sigma_d^2) turns dSSE into dNLL, bnet.py:215):
 *   dmu[i]  = sum_s gW[s,i]*gw_scale - kl_scale/S * sum_s gp(w_si)
 *   drho[i] = sum_s gW[s,i]*gw_scale*sigma_i*eps_si - kl_scale*(1 + 1/S sum_s gp(w_si)*sigma_i*eps_si)
 * with gp = d/dw log prior density.  dmu, drho: [p] float64. */
int qn_vi_grad(const double* mu, const double* rho, const double* eps, const void* gW, int S,
               int64_t p, double pi, double sigma1, double sigma2, double gw_scale, double kl_scale,
               int dtype, double* dmu_out, double* drho_out, void* stream);

/* One Adam step for B independent members at once (torch.optim.Adam defaults as used by
 * quinn/nns/nnfit.py:74-75, single-tensor update order):
 *   g = G*gscale + wd*W;  m += (g-m)*(1-b1);  v = v*b2 + (1-b2)*g*g;
 *   W -= lr[b]/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * W, m, v: [B, p] float64 master state; G: [B, p] dtype; lr: [B] float64 (device);
 * step t >= 1.  Members with lr[b] == 0 are left untouched. */
int qn_adam_batched(double* W, const void* G, double* m, double* v, const double* lr, int B,
                    int64_t p, int dtype, double gscale, double wd, double beta1, double beta2,
                    double eps, int step, void* stream);

/* Device-resident Metropolis-Hastings step (throughput engine of the adaptive Metropolis sampler,
 * quinn/mcmc/admcmc.py:38-74 + quinn/mcmc/mcmc.py:65-85), two kernels around the batched
 * log-posterior.  The step counter lives in device memory (keeping it there makes a run of steps a static
 * launch sequence / HIP graph).  It is DOUBLE-BUFFERED by the parity of the step, like the other per-chain
 * scalars qn_mcmc_accept maintains: the accept call of a step reads slot `parity` and writes slot 1 - parity, so
 * its workgroups (several per chain) never see a half-updated state and need no fence or atomic.  The proposal
 * kernels take a pointer to the CURRENT slot (`step_ptr` of qn_mcmc_propose* / qn_mcmc_apply_delta = base + parity).
 *
 * qn_mcmc_propose: out[c,:] = cur[c,:] + sd[c,:] * z + c1 * z0_c with z ~ N(0,I), z0_c ~ N(0,1)
 *   (the initial proposal covariance c1^2 + diag(sd^2) = 0.01 + diag(0.09|x0|), admcmc.py:65);
 *   with cur == NULL it writes the standard normals z themselves (input of a dense factor product).
 *   Random numbers: Philox4x32-10 keyed by (seed, step, GLOBAL chain id = chain0 + c, purpose, index): a
 *   chain's draws do not depend on how the chains are split over launches or ranks (every qn_mcmc_* call
 *   takes chain0, the global id of its first chain). */
int qn_mcmc_propose(const double* cur, const double* sd, double c1, int C, int chain0, int64_t p, uint64_t seed,
                    const int64_t* step_ptr, double* out, void* stream);

/* qn_mcmc_accept: for every chain c: log-posterior of the proposal from its SSE (sse_prop [C, nparts]: summed left to
 *   right, nparts = 1 for a plain [C] vector; see qn_mlp_sse_fwd_parts),
 *   lp = -(0.5 sse/sigma^2 + (n_rows/2) log 2pi + n_rows log sigma); mh = exp(lp - cur_lp[c]);
 *   accept iff u_c < mh (mcmc.py:72-75); updates cur, cur_lp, best / best_lp (MAP, mcmc.py:79-81),
 *   nacc, writes chain[c, step+1, :] (optional), lps[c, step+1], alphas[c, step+1]; then advances the
 *   counter.  cur_lp, best_lp, kcur: [2, C] and step_ptr: [2] -- slot `parity` (0 / 1) is read, slot 1 - parity
 *   written; the caller alternates parity from step to step (slot 0 holds the initial state for parity 0).
 *   With hist != NULL it also maintains what the adapted proposal is drawn from
 *   (qn_mcmc_propose_hist): hist [C, kcap, pstride] FLOAT16 = the DISTINCT states visited, as (x - x0[c]) * hscale[c]
 *   (x0 [C, p] float64: the chain's reference point -- the start, or wherever the caller re-bases the rows to; hscale [C]
 *   float64 or NULL = 1: a power of two that keeps the rows in float16's range, values are clamped to +-65504; half the bytes
 *   of float32 rows for the kernel that streams the whole history, and its products on the float16 matrix cores; rounding
 *   2^-11 of |x - x0|) (row 0 = the start, a new row per accepted move), mult [C, kcap] their multiplicities in the
 *   chain so far, kcur [2, C] the index of the current state's row, sumx [C, p] the sum of mult x (x - x0) over the
 *   states the chain has LEFT (a stay is added when the chain leaves the state -- no per-step pass over the vector; the sum
 *   of (x_i - x0) over all samples so far is sumx + mult[c, kcur[c]] x (cur[c] - x0[c])).  kcur[c] >= kcap means the history
 *   is full: rows, multiplicities and the sum are no longer maintained (the caller compresses before that happens). */
int qn_mcmc_accept(const double* prop, const double* sse_prop, double sigma, int n_rows, int C, int chain0, int64_t p,
                   int nmcmc, uint64_t seed, double* cur, double* cur_lp, double* best, double* best_lp,
                   double* chain, double* lps, double* alphas, int64_t* nacc, const double* x0, void* hist,
                   const double* hscale, int32_t* mult, int32_t* kcur, double* sumx, int kcap, int64_t pstride,
                   int64_t* step_ptr, int parity, int nparts, void* stream);

/* qn_mcmc_accept_propose: qn_mcmc_accept that also writes the NEXT step's proposal from the state it has just decided
 * (one launch and one pass over the state fewer per step): next_mode 0 = nothing more; 1 = prop_next = cur' + sd z +
 * c1 z0 (qn_mcmc_propose); 2 = prop_next = cur' + delta[c, t_next, :] + s_iso z (qn_mcmc_apply_delta).  Same random
 * numbers (streams of step + 1) and the same arithmetic as the separate kernels: results are bit-identical.
 * prop_next may be the buffer `prop`. */
int qn_mcmc_accept_propose(const double* prop, const double* sse_prop, double sigma, int n_rows, int C, int chain0,
                           int64_t p, int nmcmc, uint64_t seed, double* cur, double* cur_lp, double* best, double* best_lp,
                           double* chain, double* lps, double* alphas, int64_t* nacc, const double* x0, void* hist,
                           const double* hscale, int32_t* mult, int32_t* kcur, double* sumx, int kcap, int64_t pstride,
                           int64_t* step_ptr, int next_mode, const double* sd, double c1, const double* delta, int t_next, double s_iso,
                           double* prop_next, int parity, int nparts, void* stream);

/* qn_mcmc_propose_hist: the ADAPTED proposal of adaptive Metropolis (admcmc.py:52-70), drawn in sample
 *   space.  After an adaptation at step i the reference proposes from N(x, c (cov_i + 1e-8 I)) with
 *   cov_i the unbiased sample covariance of x_0..x_i and c = gamma 2.4^2 / p.  With the K distinct
 *   states x_k of that history, multiplicities w_k, mean m and n = i + 1,
 *       out[c,:] = cur[c,:] + s_lr * sum_k wsnap[c,k] u_k (hist[c,k,:] / hscale[c] - msnap[c,:]) + s_iso * v,
 *   u_k, v_j iid N(0,1), wsnap = sqrt(w), s_lr = sqrt(c/(n-1)), s_iso = sqrt(c 1e-8), has exactly that
 *   covariance: a K x p GEMV over the stored states instead of a p x p factor (cfg2: K ~ 10^2..10^3
 *   rows of 34 KB per chain and step instead of 290-580 MB).  ksnap [C] = K per chain, msnap [C, p] =
 *   mean of (x - x0) at the adaptation, both frozen until the next adaptation.  hist: float16 rows (x_k - x0) * hscale
 *   (qn_mcmc_accept); the coefficients wsnap u_k are rounded to float16 as well (the matrix cores' operand type; both the
 *   single-step and the block kernel use the rounded values, products accumulate in float32 / float64).  pstride even, >= p
 *   (a multiple of 4 for qn_mcmc_propose_hist_block). */
int qn_mcmc_propose_hist(const double* cur, const void* hist, const float* wsnap, const int32_t* ksnap,
                         const double* msnap, const double* hscale, double s_lr, double s_iso, int C, int chain0, int64_t p,
                         int64_t pstride, int kcap, uint64_t seed, const int64_t* step_ptr, double* out, void* stream);

/* The same draw for TB = qn_mcmc_hist_block_steps() (= 64) consecutive steps in one pass over the stored states:
 * the increment of step t depends only on the frozen snapshot and on that step's random numbers (keyed
 * by the absolute step, exactly as in qn_mcmc_propose_hist), not on the chain's state, so
 *   delta[c, t, :] = s_lr * sum_k wsnap[c,k] u_k^(step0+t) (hist[c,k,:] / hscale[c] - msnap[c,:])
 * for t = 0..TB-1 reads the history once: HBM traffic per step / TB, a (TB x K).(K x p) product per chain
 * (v_mfma_f32_32x32x16_f16: float16 operands, float32 accumulation).  step_ptr != NULL: step0 is read from the device step
 * counter when the kernels run (a static launch, capturable in a HIP graph).  coef: scratch of
 * qn_mcmc_hist_block_coef_bytes(C, kcap) bytes; delta: [C, TB, p] float64.
 * order (optional, [C] int32): a permutation of the chains giving the dispatch order of the history product -- pass the
 * chains sorted by ksnap, longest first (the work per chain is proportional to ksnap[c]); results do not depend on it.
 * qn_mcmc_apply_delta: out[c,:] = cur[c,:] + delta[c, t, :] + s_iso * v (the proposal of step step0 + t; v on the
 * stream of the CURRENT step *step_ptr, as in qn_mcmc_propose_hist; s_iso is unused by the block call). */
int qn_mcmc_hist_block_steps(void);
size_t qn_mcmc_hist_block_coef_bytes(int C, int kcap);
int qn_mcmc_propose_hist_block(const void* hist, const float* wsnap, const int32_t* ksnap, const double* msnap,
                               const double* hscale, double s_lr, double s_iso, int C, int chain0, int64_t p, int64_t pstride,
                               int kcap, uint64_t seed, int64_t step0, const int64_t* step_ptr, void* coef, double* delta,
                               const int32_t* order, void* stream);
int qn_mcmc_apply_delta(const double* cur, const double* delta, int t, double s_iso, int C, int chain0, int64_t p,
                        uint64_t seed, const int64_t* step_ptr, double* out, void* stream);

/* Device-resident Hamiltonian Monte Carlo step (throughput engine of quinn/mcmc/hmc.py:43-66 + the accept block of
 * quinn/mcmc/mcmc.py:65-85): three elementwise kernels around qn_mlp_sse_fwdbwd, no host synchronisation, every launch
 * static given the step parity (a pair of steps is capturable as one HIP graph).  All state is float64 [C, p]; the
 * gradient arrays hold d SSE / d W as qn_mlp_sse_fwdbwd writes it (d logpost = -0.5/sigma^2 * d SSE is applied here).
 *
 * qn_hmc_begin (hmc.py:43-51): momentum z ~ N(0, I) -- Philox4x32-10 keyed by (seed, step, GLOBAL chain id = chain0 + c,
 *   index), so a chain's draws do not depend on how chains are split over launches or ranks --,
 *   mom = z + (eps/2) d logpost(cur), q = cur + eps * mom, and the current kinetic energy as partial sums of z^2:
 *   kin_cur_parts [C, qn_hmc_parts(p)] (the accept call adds them left to right and halves the sum; the number of
 *   partials depends on p alone).  grad_cur is the gradient at the current state, kept from the accepted proposal.
 * qn_hmc_leap (hmc.py:53-60): given grad_q = d SSE / d W at q (dtype QN_F64 / QN_F32): inner step (last = 0)
 *   mom += eps * d logpost(q), q += eps * mom; last step (last = 1) mom += (eps/2) * d logpost(q) and kin_prop_parts
 *   [C, qn_hmc_parts(p)] = partial sums of mom^2 (the sign flip of hmc.py:64 does not change it).
 * qn_hmc_accept (mcmc.py:68-85): log-posterior of the proposal from sse_q [C] (the SSE the last gradient call returned:
 *   the reference spends an extra forward pass on it), mh = exp((U + K) - (U' + K')), accept iff u_c < mh; on accept
 *   cur <- q, grad_cur <- grad_q; MAP, chain / lps / alphas rows, nacc and the double-buffered scalars / step counter
 *   exactly as qn_mcmc_accept (cur_lp, best_lp: [2, C]; step_ptr: [2]; slot `parity` read, slot 1 - parity written). */
int qn_hmc_parts(int64_t p);
int qn_hmc_begin(const double* cur, const double* grad_cur, double sigma, double epsilon, int C, int chain0, int64_t p,
                 uint64_t seed, const int64_t* step_ptr, double* mom, double* q, double* kin_cur_parts, void* stream);
int qn_hmc_leap(const void* grad_q, int dtype, double sigma, double epsilon, int last, int C, int64_t p, double* mom,
                double* q, double* kin_prop_parts, void* stream);
int qn_hmc_accept(const double* q, const double* grad_q, const double* sse_q, const double* kin_cur_parts,
                  const double* kin_prop_parts, double sigma, int n_rows, int C, int chain0, int64_t p, int nmcmc,
                  uint64_t seed, double* cur, double* grad_cur, double* cur_lp, double* best, double* best_lp,
                  double* chain, double* lps, double* alphas, int64_t* nacc, int64_t* step_ptr, int parity, void* stream);

/* Device HMC / MALA with a per-chain step size eps [C] and a diagonal mass matrix, both DEVICE arrays, and their warm-up.
 * scale [C, p] > 0 is the square root of the inverse mass, M^-1 = diag(scale^2); NULL means 1.  The leapfrog runs in whitened
 * momenta u = scale * r (r the momentum), so u ~ N(0, I), the kinetic energy is |u|^2 / 2 and qn_hmc_accept is used unchanged:
 *     z ~ N(0, I);  u = z + (eps_c/2) s * g(cur);  q = cur + eps_c s * u
 *     L-1 times:    u += eps_c s * g(q);  q += eps_c s * u
 *     last:         u += (eps_c/2) s * g(q);          K_cur = sum z^2 / 2,  K_prop = sum u^2 / 2        (g = d logpost / d W)
 * qn_hmc_begin_s / qn_hmc_leap_s: qn_hmc_begin / qn_hmc_leap with the per-element factors (kick_c * s) and (eps_c * s) in
 *   place of the scalars -- same grid (qn_hmc_parts(p) workgroups per chain), same Philox keys (seed, 2 * step, global chain
 *   id), same fixed-order partial sums: with scale NULL or 1 and equal eps_c they give those calls' results bit for bit.
 * qn_hmc_adapt: one launch per warm-up step, after the accept call of that step.  Per chain it reads the step t just decided
 *   from slot `parity` of step_ptr [2] (the slot that accept call wrote) and its acceptance mh = alphas[c, t] (alphas
 *   [C, nmcmc + 1] as qn_hmc_accept fills it), a = min(1, mh) with NaN counted as 0, and advances the dual averaging of
 *   Hoffman & Gelman 2014 (algorithm 5; gamma = 0.05, t0 = 10, kappa = 0.75), m >= 1 the index of this step in the current run:
 *     Hbar = (1 - 1/(m+t0)) Hbar + (target_accept - a)/(m+t0);  logeps = mu - sqrt(m)/gamma * Hbar;
 *     logbar = m^-kappa logeps + (1 - m^-kappa) logbar;         eps[c] = exp(logeps)
 *   on da [C, 4] = (mu, Hbar, logbar, logeps); a run starts from (log(10 eps0), 0, 0, any).  freeze (the last warm-up step):
 *   eps[c] = exp(logbar) instead.  collect: Welford update of mean / m2 [C, p] with the state cur [C, p], n >= 1 the number
 *   of states collected including this one: d = x - mean; mean += d / n; m2 += d * (x - mean).  finish (a window end, n >= 2;
 *   after the update of the same call): scale = sqrt((n/(n+5)) * m2/(n-1) + 1e-3 * 5/(n+5)), mean = m2 = 0, and dual averaging
 *   restarts around the new step size: mu = log(10 eps[c]), Hbar = logbar = 0 (the caller's next m is 1).  finish and freeze
 *   exclude each other.  m, n and the flags are host-known: nothing is read back, no atomics; cur / mean / m2 / scale may be
 *   NULL when neither collect nor finish is set. */
int qn_hmc_begin_s(const double* cur, const double* grad_cur, double sigma, const double* eps, const double* scale, int C,
                   int chain0, int64_t p, uint64_t seed, const int64_t* step_ptr, double* mom, double* q,
                   double* kin_cur_parts, void* stream);
int qn_hmc_leap_s(const void* grad_q, int dtype, double sigma, const double* eps, const double* scale, int last, int C,
                  int64_t p, double* mom, double* q, double* kin_prop_parts, void* stream);
int qn_hmc_adapt(const double* cur, const double* alphas, int nmcmc, const int64_t* step_ptr, int parity, int C, int64_t p,
                 int m, double target_accept, int collect, int finish, int freeze, int n, double* da, double* eps,
                 double* mean, double* m2, double* scale, void* stream);

/* Replica exchange (parallel tempering) for the device HMC / MALA step (build-only; the reference has no such sampler;
 * quinn_amd.mcmc.tempering restates the contract in numpy).  The C chains of a launch are whole ladders of R rungs,
 * ladder-major: chain c is rung c % R of ladder c / R and samples pi^beta_c, beta [C] a DEVICE array with
 * 1 = beta_0 > ... > beta_{R-1} > 0 inside a ladder.  Every stored log-posterior (cur_lp, best_lp, lps, the MAP) stays in the
 * target's own, untempered units for every rung.
 *
 * qn_hmc_begin_t / qn_hmc_leap_t: qn_hmc_begin_s / qn_hmc_leap_s with the force beta_c * d logpost: gs_c = gs * beta_c
 *   (gs = -0.5 / sigma^2) is formed first and stands wherever those calls use gs; drifts are unchanged.  Same grid, element ->
 *   thread map, Philox keys and partial sums: with beta NULL (= 1) or all 1 the results are those calls' bit for bit.
 * qn_hmc_accept_t: qn_hmc_accept with mh = exp((-beta_c clp + K_cur / 2) - (-beta_c plp + K_prop / 2)), clp / plp the
 *   untempered log-posteriors; beta NULL or all 1: qn_hmc_accept bit for bit.
 * qn_pt_swap: one exchange round, launched after the accept call (and the adapt call, if any) of a step.  With e = round & 1
 *   the pairs are (c, c + 1) for c % R in {e, e + 2, ...}, c % R + 1 < R (deterministic even-odd scheme).  The step t just
 *   decided is read from slot `parity` of step_ptr [2]; per pair, from slot `parity` of cur_lp [2, C]:
 *     d = (beta_c - beta_{c+1}) * (lp_{c+1} - lp_c);   u = u01(words 0, 1) of Philox (seed, 2 t + 1, [chain0 + c : 24][6 : 4][0 : 36])
 *   and the pair swaps iff both lp are finite and u < exp(d) (NaN: no swap).  On a swap the rows c and c + 1 of cur and
 *   grad_cur [C, p] are exchanged in place, and chain[c, t, :], chain[c + 1, t, :] (chain [C, nmcmc + 1, p] or NULL) and
 *   lps[c, t], lps[c + 1, t] (lps [C, nmcmc + 1]) are rewritten to the exchanged values: the stored row of step t is the state
 *   step t + 1 starts from.  For EVERY chain, paired or not, slot 1 - parity receives cur_lp (exchanged or copied), best_lp
 *   (copied: the MAP `best` stays with the chain slot).  rid [2, C] int32, the replica sitting in each chain slot, is double-
 *   buffered by a parity of its OWN: slot rid_parity is read, slot 1 - rid_parity written (exchanged or copied), and the caller
 *   flips rid_parity once per exchange round -- the accept calls in between flip the step parity but carry no rid over, so the
 *   two parities differ whenever an odd number of steps lies between two rounds.  rep[c, round + 1] = that replica (rep [C, nrounds + 1] int32 or NULL; column 0 is the caller's).  swap_try[c] += 1
 *   for the lower chain of a pair and swap_acc[c] += 1 on a swap (both [C] int64).  step_ptr[1 - parity] = t: no step was
 *   taken, the caller only flips its parity (as after qn_sg_step(final)).  No atomics, no fences: two calls on equal inputs
 *   give equal bits.  QN_EINVAL with a message, before any pointer is touched: R < 2, C % R != 0, chain0 % R != 0, C outside
 *   1 .. 65535, p < 1, nmcmc < 1, round outside 0 .. nrounds - 1, a parity or rid_parity other than 0 / 1, a NULL pointer other than chain / rep. */
int qn_hmc_begin_t(const double* cur, const double* grad_cur, double sigma, const double* eps, const double* scale,
                   const double* beta, int C, int chain0, int64_t p, uint64_t seed, const int64_t* step_ptr, double* mom,
                   double* q, double* kin_cur_parts, void* stream);
int qn_hmc_leap_t(const void* grad_q, int dtype, double sigma, const double* eps, const double* scale, const double* beta,
                  int last, int C, int64_t p, double* mom, double* q, double* kin_prop_parts, void* stream);
int qn_hmc_accept_t(const double* q, const double* grad_q, const double* sse_q, const double* kin_cur_parts,
                    const double* kin_prop_parts, double sigma, int n_rows, int C, int chain0, int64_t p, int nmcmc,
                    uint64_t seed, double* cur, double* grad_cur, double* cur_lp, double* best, double* best_lp, double* chain,
                    double* lps, double* alphas, int64_t* nacc, int64_t* step_ptr, int parity, const double* beta,
                    void* stream);
int qn_pt_swap(double* cur, double* grad_cur, double* cur_lp, double* best_lp, double* lps, double* chain, const double* beta,
               int32_t* rid, int32_t* rep, int64_t* swap_acc, int64_t* swap_try, int64_t* step_ptr, int R, int round,
               int nrounds, int C, int chain0, int64_t p, int nmcmc, uint64_t seed, int parity, int rid_parity, void* stream);

/* Stochastic-gradient MCMC on the device (SGLD, SGHMC, optional cyclical step size; build-only, the reference has no such
 * sampler).  A step is qn_mlp_sse_fwdbwd on each chain's own n_batch rows followed by ONE qn_sg_step; nothing is read back.
 * Philox4x32-10 keyed by (seed, stream = inner step t, counter = [GLOBAL chain id = chain0 + c : 24][purpose : 4][index : 36]),
 * purpose 4 = minibatch rows (index = entry / 4), purpose 5 = step noise (index = element pair).
 *
 * qn_sg_rows: rows [C, Nb] int32 of inner step t = (step_ptr ? *step_ptr : 0) + step_off: entry j of chain c is
 *   __umulhi(r, N) in [0, N) with r = word (j & 3) of the block with index j >> 2 -- independent uniform draws WITH
 *   replacement, pure integer arithmetic (quinn_amd.mcmc.sgmcmc.minibatch_rows restates it bit for bit).
 * qn_sg_step: reads the inner step t from slot `parity` of step_ptr [2] and, for every chain,
 *     g   = (n_rows / n_batch) * grad / (2 sigma^2)         grad [C, p] = d SSE / d W of the minibatch, dtype QN_F64 / QN_F32
 *     eta = eta0                                            schedule 0 (constant)
 *           eta0 / 2 * (cos(pi (t mod K) / K) + 1)          schedule 1 (cyclic), K = cycle_len >= 2 inner steps per cycle
 *     on  = 1 (constant);  (t mod K) / K >= explore_frac (cyclic)
 *     v <- (1 - alpha) v - eta g + on sqrt(2 alpha eta temperature) z,  z ~ N(0, I);   theta <- theta + v
 *   theta, v: [C, p] float64, updated in place; alpha = 1 (SGLD) never touches v (NULL allowed); temperature = 0 or on = 0:
 *   no noise is drawn.  theta_op (optional, QN_F32 only): the new positions as float32 [C, p], what a float32 operator's
 *   next gradient call reads.  In the same launch:
 *   - t % thin == 0: lps[c, t / thin] = -((n_rows / n_batch) sse[c] / (2 sigma^2) + (n_rows / 2) log 2 pi + n_rows log sigma),
 *     the MINIBATCH estimate of the log-posterior of the incoming state theta_t (sse [C]: the SSE the gradient call returned);
 *     where it is >= best_lp, best [C, p] <- theta_t.  best_lp [2, C] is double-buffered like step_ptr (slot `parity` read,
 *     slot 1 - parity written).  lps [C, nstore + 1].
 *   - (t + 1) % thin == 0: chain[c, (t + 1) / thin, :] <- the new theta (chain [C, nstore + 1, p] or NULL; rows beyond nstore
 *     are never written).
 *   - rows (optional, [2, C, n_batch] int32): the rows of step t + 1 (qn_sg_rows' formula) go to half 1 - parity.
 *   - step_ptr[1 - parity] = t + 1.
 *   final != 0: only the log-posterior trace / best update of theta_t; nothing moves, step_ptr[1 - parity] = t. */
int qn_sg_rows(int32_t* rows, int C, int Nb, int N, int chain0, uint64_t seed, const int64_t* step_ptr, int64_t step_off,
               void* stream);
int qn_sg_step(double* theta, double* v, const void* grad, int dtype, const double* sse, double sigma, int n_rows, int n_batch,
               double eta0, double alpha, double temperature, int schedule, int64_t cycle_len, double explore_frac, int thin,
               int final, int C, int chain0, int64_t p, int nstore, uint64_t seed, void* theta_op, double* best, double* best_lp,
               double* chain, double* lps, int32_t* rows, int64_t* step_ptr, int parity, void* stream);

/* Fold an isotropic Gaussian weight prior N(0, priorsigma^2 I) into the outputs of a forward / gradient call (build-only; the
 * reference has no prior in NN_MCMC).  For every chain c < C, W [C, p] float64:
 *     grad[c, j]            <- grad[c, j] + (2 lam) * W[c, j]           grad [C, p] of dtype gdtype (QN_F64 / QN_F32) or NULL
 *     sse[c * sse_stride]   <- sse[c * sse_stride] + (lam * sum_j W[c, j]^2 + c0)      sse float64, or NULL
 * lam > 0 and c0 finite are host scalars.  With lam = sigma^2 / priorsigma^2 and c0 = sigma^2 p log(2 pi priorsigma^2) the
 * sampler kernels, which form log-posteriors and forces as gs * sse and gs * grad with gs = -0.5 / sigma^2, then see
 *     gs sse' = gs sse + log N(w; 0, priorsigma^2 I)   (normaliser included),       gs grad' = gs grad - w / priorsigma^2:
 * one launch behind every qn_mlp_sse_fwd / qn_mlp_sse_fwd_parts / qn_mlp_sse_fwdbwd call gives the accept, leapfrog, adapt,
 * swap and SG kernels the posterior with the prior (sse_stride = the number of parts after qn_mlp_sse_fwd_parts: column 0
 * receives the term, the accept kernel's left-to-right sum is unchanged).  A minibatch call multiplies lam and c0 by
 * n_batch / n_rows, which qn_sg_step's (n_rows / n_batch) undoes: the prior is exact, only the likelihood is estimated.
 * Arithmetic: every gradient entry is formed in float64 with one rounding per operation -- the product (2 lam) * w, then the
 *   sum, no contraction; a QN_F32 gradient is widened, updated in float64 and rounded once.  The sum of squares is added in a
 *   fixed order that depends on p alone -- not on C, the chain's place in the launch or the grid (workgroup 0 of every chain
 *   sums the whole row and is the only writer of the chain's sse entry; the other columns of a strided sse are not touched).
 *   No atomics, no fences: two calls on equal inputs give equal bits, and a chain's result is the same launched alone or among
 *   others.  Rows need 8-byte alignment only.  Non-finite weights propagate: an Inf or NaN in W[c] makes sse[c] +Inf or NaN and
 *   touches no other chain.
 * QN_EINVAL with a message, before any pointer is touched: W NULL; grad and sse both NULL; lam not > 0 or not finite; c0 not
 *   finite; C outside 1 .. 65535; p < 1; sse_stride < 1 with sse given; a gdtype other than the two with grad given. */
int qn_prior_fold(const double* W, double lam, double c0, void* grad, int gdtype, double* sse, int sse_stride, int C, int64_t p,
                  void* stream);

/* Hierarchical Gaussian weight prior for the device HMC / MALA engines (build-only; quinn_amd/mcmc/hyper.py restates both
 * calls in numpy).  Groups g < G, 1 <= G <= 32, are the contiguous segments [seg[g], seg[g + 1]) of the flat weight vector
 * (seg [G + 1] int64 ON THE DEVICE, seg[0] = 0, seg[G] = p, strictly increasing; the kernels clamp every bound to [0, p], so a
 * wrong array gives wrong numbers, never an access outside a row), n_g entries each, and
 *     w_j | tau_g ~ N(0, 1 / tau_g) for j in group g,     tau_g ~ Gamma(shape a0, rate b0).
 * In the units of the sampler kernels (gs = -0.5 / sigma^2), per chain c, with S_g = sum_{j in g} w_j^2:
 *     lam[c, g] = sigma^2 tau[c, g]
 *     c0[c]     = sigma^2 (sum_g n_g log(2 pi / tau[c, g]) - 2 log p(tau[c, :]))
 *     log p(tau) = sum_g (a0 log b0 - lgamma(a0) + (a0 - 1) log tau_g - b0 tau_g)
 * so that gs (sse + sum_g lam_g S_g + c0) + (likelihood constants) is the JOINT log density of (w, tau) given the data.
 *
 * qn_prior_fold_g: qn_prior_fold with lam [C, G] and c0 [C] read from device arrays.  For every chain c < C, W [C, p] float64:
 *     grad[c, j]           <- grad[c, j] + (2 lam[c, g(j)]) * W[c, j]          grad [C, p] of dtype gdtype (QN_F64 / QN_F32) or NULL
 *     sse[c * sse_stride]  <- sse[c * sse_stride] + (sum_g lam[c, g] S_g + c0[c])      sse float64, or NULL
 *   Arithmetic: that of qn_prior_fold -- the product (2 lam) * w, then the sum, in float64, one rounding each, no contraction; a
 *   QN_F32 gradient is widened, updated and rounded once; same grid and element -> thread map: with all lam[c, :] equal the
 *   gradient is qn_prior_fold's bit for bit.  The group of an element is not looked up in memory: the bounds and factors sit in
 *   LDS and every thread walks forward through them.  S_g is summed by workgroup 0 of the chain in an order that depends on
 *   (p, seg) alone; the terms lam_g S_g are added left to right, then c0; that workgroup is the only writer of the chain's sse
 *   entry (the other columns of a strided sse are not touched).  No atomics, no fences: equal inputs give equal bits, a chain's
 *   result is the same launched alone or among others, non-finite weights touch their own chain only.
 *   QN_EINVAL with a message, before any pointer is touched: W, lam, c0 or seg NULL; grad and sse both NULL; G outside 1 .. 32;
 *   C outside 1 .. 65535; p < 1 or p < G; sse_stride < 1 with sse given; a gdtype other than the two with grad given.
 *
 * qn_hyper_gibbs: one Gibbs round, launched after the accept call (and the adapt call, if any) of a step.  lam [2, C, G] and
 *   c0 [2, C] are double-buffered by a parity of their OWN (slot hyper_parity is read, slot 1 - hyper_parity written; the caller
 *   flips it once per round), the scalars cur_lp, best_lp [2, C] and step_ptr [2] by the step parity.  Per chain: the step t
 *   just decided is read from slot `parity` of step_ptr; S_g is computed from cur [C, p] (the sums of qn_prior_fold_g);
 *       tau'_g ~ Gamma(a0 + n_g / 2, rate b0 + S_g / 2),   lam'_g = sigma^2 tau'_g,   c0' as above;
 *       taus[c, round + 1, g] = lam'_g / sigma^2           (taus [C, nrounds + 1, G] float64 or NULL; column 0 is the caller's)
 *       grad_cur[c, j] += (2 (lam'_g(j) - lam_g(j))) * cur[c, j]
 *       cur_lp[1 - parity, c] = cur_lp[parity, c] + gs (sum_g (lam'_g - lam_g) S_g + (c0' - c0))
 *       best_lp[1 - parity, c] = best_lp[parity, c];   step_ptr[1 - parity] = t;   lps[c, t] = the new cur_lp (0 <= t <= nmcmc):
 *   the stored trace is that of the state step t + 1 starts from, as after qn_pt_swap.  The caller flips both parities.
 *   Gamma variates: Marsaglia & Tsang (2000) with the log test (no squeeze), float64 log / sqrt / cos.  Philox4x32-10 keyed
 *   (seed, 2 t + 1, [chain0 + c : 24][11 : 4][index : 36]), index = (g << 16) | (attempt << 4) | block: block 0 of an attempt
 *   gives the normal x = sqrt(-2 log u01(words 0, 1)) cos(2 pi u01(words 2, 3)), block 1 the uniform of the test (words 0, 1);
 *   with d = a - 1 / 3, c = 1 / sqrt(9 d), v = (1 + c x)^3 the attempt is accepted iff v > 0 and
 *   log u < 0.5 x^2 + d - d v + d log v, and the draw is d v / rate.  shape < 1: drawn at a = shape + 1 and multiplied by
 *   u^(1 / shape), u = u01(words 0, 1) of index (g << 16) | (64 << 4).  The loop is BOUNDED at 64 attempts; after them the draw
 *   is shape / rate.  A chain with a non-finite S_g (or whose new lam or c0 would not be positive / finite) keeps its tau, lam,
 *   c0, grad_cur, cur_lp and lps[c, t] (copied to the new slots; its taus column repeats the previous one); no other chain is
 *   touched.  Every workgroup of a chain takes the whole decision itself from the slots nobody writes in the launch: no
 *   atomics, no fences, no arrival counters; equal inputs give equal bits and nothing depends on C or the chain's place.
 *   QN_EINVAL with a message, before any pointer is touched: a0, b0 or sigma not > 0 or not finite; G outside 1 .. 32; C outside
 *   1 .. 65535; p < 1 or p < G; chain0 < 0; nmcmc < 1; round outside 0 .. nrounds - 1; a parity other than 0 / 1; a NULL pointer
 *   other than taus. */
int qn_prior_fold_g(const double* W, const double* lam, const double* c0, const int64_t* seg, int G, void* grad, int gdtype,
                    double* sse, int sse_stride, int C, int64_t p, void* stream);
int qn_hyper_gibbs(const double* cur, double* grad_cur, double* cur_lp, double* best_lp, double* lps, double* lam, double* c0,
                   const int64_t* seg, double* taus, int64_t* step_ptr, double sigma, double a0, double b0, int G, int round,
                   int nrounds, int C, int chain0, int64_t p, int nmcmc, uint64_t seed, int parity, int hyper_parity,
                   void* stream);

/* Conjugate hyper-prior on the noise level of the Gaussian likelihood for the device HMC / MALA engines (build-only;
 * quinn_amd/mcmc/noise.py restates both calls in numpy).  One noise variance s2_c per chain, shared by all n = N * o entries
 * of y (N rows, o outputs):
 *     y_k | w, s2 ~ N(M_w(x)_k, s2),     1 / s2 ~ Gamma(shape a0, rate b0),
 *     1 / s2 | w, y ~ Gamma(a0 + n / 2, rate b0 + SSE(w) / 2)          (SSE: the data sum of squares alone, without a prior).
 * The weight prior is NOT scaled by s2.  Every sampler kernel keeps the nominal noise level sigma0 it is called with
 * (gs = -h, h = 0.5 / sigma0^2, and the accept kernel's lik_const = (N / 2) log 2 pi + N log sigma0); per chain c
 *     kappa[c] = sigma0^2 / s2_c
 *     d0[c]    = sigma0^2 (n log(2 pi s2_c) - 2 log p(s2_c) - N log(2 pi sigma0^2))
 *     log p(s2) = a0 log b0 - lgamma(a0) + (a0 + 1) log(1 / s2) - b0 / s2           (the density of s2, Jacobian included)
 * so that -(h sse' + lik_const) with sse' = kappa sse + P + d0, P = sum_g lam_g S_g + c0 the weight prior's term in the units
 * of qn_prior_fold_g (absent without a prior), is the JOINT log density of (w, s2[, tau]) given the data; the normaliser covers
 * all N * o entries (the kernels' constant counts N, d0 removes it).  At fixed s2 the accept ratio is the conditional's.
 *
 * qn_noise_fold: the fold above in ONE launch; it stands where qn_prior_fold / qn_prior_fold_g stand.  For every chain c < C,
 *   W [C, p] float64, kappa [C], d0 [C] float64 on the device, and the weight prior as lam [C, G], c0 [C], seg [G + 1] of
 *   qn_prior_fold_g with 0 <= G <= 32 (G = 0: no weight prior, the three pointers are not read; a scalar prior is G = 1):
 *     grad[c, j]           <- kappa[c] * grad[c, j] + (2 lam[c, g(j)]) * W[c, j]     grad [C, p] of dtype gdtype (QN_F64 / QN_F32) or NULL
 *     sse[c * sse_stride]  <- (kappa[c] * sse[c * sse_stride] + P) + d0[c]           sse float64, or NULL
 *   Arithmetic: float64, no contraction, one rounding per operation -- the product kappa * g, the product (2 lam) * w, the sum
 *   (G = 0: the first product alone); a QN_F32 gradient is widened, updated and rounded once.  Grid, element -> thread map and
 *   the forward walk through the groups in LDS are qn_prior_fold_g's.  Workgroup 0 of a chain is the only writer of its sse
 *   entry (the other columns of a strided sse are not touched): kappa * sse, plus P -- formed exactly as qn_prior_fold_g forms
 *   it: the terms lam_g S_g added left to right, then c0 -- plus d0.  With kappa = 1, d0 = 0 and G >= 1 both outputs equal
 *   qn_prior_fold_g's bit for bit.  No atomics, no fences: equal inputs give equal bits, a chain's result is the same launched
 *   alone or among others, non-finite weights touch their own chain only.
 *   QN_EINVAL with a message, before any pointer is touched: W, kappa or d0 NULL; G outside 0 .. 32; lam, c0 or seg NULL with
 *   G >= 1; grad and sse both NULL; C outside 1 .. 65535; p < 1 or p < G; sse_stride < 1 with sse given; a gdtype other than the
 *   two with grad given.
 *
 * qn_noise_gibbs: one Gibbs round, launched after the accept call, the adapt call and qn_hyper_gibbs (if any) of a step.
 *   kappa [2, C] and d0 [2, C] are double-buffered by a parity of their OWN (slot noise_parity is read, slot 1 - noise_parity
 *   written; the caller flips it once per round), cur_lp, best_lp [2, C] and step_ptr [2] by the step parity.  lam [C, G] and
 *   c0 [C] are the slot of the weight prior that is current after those calls (read only; G = 0: not read).  Per chain, with
 *   the step t just decided read from slot `parity` of step_ptr and S_g computed from cur [C, p] (the sums of qn_prior_fold_g):
 *       F = (-cur_lp[parity, c] - lik_const) / h;   sse = ((F - d0) - P) / kappa          (the fold inverted, in this order)
 *       1 / s2' ~ Gamma(a0 + n / 2, rate b0 + sse / 2);   kappa' = sigma0^2 / s2', d0' as above;   r = kappa' / kappa
 *       sig[c, round + 1] = sqrt(s2')                 (sig [C, nrounds + 1] float64 or NULL; column 0 is the caller's)
 *       sse_rec[c] = sse                              (sse_rec [C] float64 or NULL: the recovered SSE, written for every chain,
 *                                                      kept or not -- for diagnostics and tests, nothing reads it)
 *       grad_cur[c, j] <- grad_cur + (r - 1) * (grad_cur - (2 lam_g(j)) * cur[c, j])          (G = 0: grad_cur + (r - 1) * grad_cur)
 *       cur_lp[1 - parity, c] = cur_lp[parity, c] - h * ((kappa' - kappa) * sse + (d0' - d0))
 *       best_lp[1 - parity, c] = best_lp[parity, c];   step_ptr[1 - parity] = t;   lps[c, t] = the new cur_lp (0 <= t <= nmcmc):
 *   the stored trace is that of the state step t + 1 starts from, as after qn_hyper_gibbs.  The caller flips both parities.
 *   n_rows = N and n = N * o are host-known.  The Gamma variate is qn_hyper_gibbs's (Marsaglia & Tsang, the log test, at most
 *   64 attempts, then shape / rate) with Philox keyed (seed, 2 t + 1, [chain0 + c : 24][12 : 4][index : 36]),
 *   index = (attempt << 4) | block.  A chain whose recovered sse is not finite or is negative, or whose s2', kappa' or d0' is
 *   not positive / finite, keeps kappa, d0, grad_cur, cur_lp and lps[c, t] (copied to the new slots; its sig column repeats
 *   the previous one); no other chain is touched.  Every workgroup of a chain takes the whole decision itself from the slots
 *   nobody writes in the launch: no atomics, no fences, no arrival counters; equal inputs give equal bits and nothing depends
 *   on C or the chain's place.
 *   QN_EINVAL with a message, before any pointer is touched: a0, b0 or sigma not > 0 or not finite; G outside 0 .. 32; C outside
 *   1 .. 65535; p < 1 or p < G; chain0 < 0; nmcmc < 1; n_rows < 1 or n < n_rows; round outside 0 .. nrounds - 1; a parity other
 *   than 0 / 1; a NULL pointer other than sig and sse_rec (and lam, c0, seg with G = 0). */
int qn_noise_fold(const double* W, const double* kappa, const double* d0, const double* lam, const double* c0,
                  const int64_t* seg, int G, void* grad, int gdtype, double* sse, int sse_stride, int C, int64_t p, void* stream);
int qn_noise_gibbs(const double* cur, double* grad_cur, double* cur_lp, double* best_lp, double* lps, double* kappa, double* d0,
                   const double* lam, const double* c0, const int64_t* seg, double* sig, double* sse_rec, int64_t* step_ptr,
                   double sigma, double a0, double b0, int n_rows, int64_t n, int G, int round, int nrounds, int C, int chain0, int64_t p,
                   int nmcmc, uint64_t seed, int parity, int noise_parity, void* stream);

/* Elliptical slice sampling on the device (Murray, Adams & MacKay 2010; build-only, the reference has no such sampler) for
 * the target L(w) N(w; 0, priorsigma^2 I), log L = gs sse + const, gs = -0.5 / sigma^2: no step size, no warm-up, only forward
 * calls.  The chains' steps are ASYNCHRONOUS: every chain has its own step t and shrink count j, and a launch of qn_ess_iter
 * either shrinks a chain's bracket or, its pending proposal accepted, starts the chain's next step in the same launch.  A run
 * is qn_ess_begin, then (qn_mlp_sse_fwd_parts on prop, qn_ess_iter) until every chain has made nmcmc steps; qn_prior_fold is
 * NOT launched (the ellipse carries the prior, the slice test sees the likelihood).  quinn_amd/mcmc/ess.py restates the rule.
 * Philox4x32-10 keyed by (seed, stream = the chain's step t, counter = [GLOBAL chain id = chain0 + c : 24][purpose : 4]
 * [index : 36]): purpose 7 = the ellipse partner (index = column pair; the float32-transcendental normals of the HMC momenta,
 * ~1e-6 relative accuracy), purpose 8 = the angle uniforms (index 0: start of the step; index j + 1: shrink j + 1).
 * Per-chain state, double-buffered by the launch parity the caller alternates (slot `parity` is read, slot 1 - parity
 * written -- copied for done chains and unchanged entries; slot 0 holds the state after qn_ess_begin):
 *     es [2, C, 6] float64 = (theta, tmin, tmax, logy, sse_cur, lp_cur)      ei [2, C, 4] int64 = (t, j, ntrunc, nevals)
 *     best_lp [2, C]      sq_parts [2, C, qn_hmc_parts(p)]: partial sums of squares of the pending proposal (fixed order, a
 *     function of p alone; the next launch adds them left to right for the log-prior)
 * and cur, nu, prop [C, p] float64, updated in place (an element belongs to one thread).  prop_op (optional, dtype QN_F32
 * only): every new proposal also as float32 [C, p], what a float32 operator's next forward reads.
 *
 * qn_ess_begin: start of step 0 of every chain from cur and sse_cur [C]:
 *     nu = priorsigma z;  theta = 2 pi u1;  logy = gs sse_cur + log u2;  tmin = theta - 2 pi;  tmax = theta;  j = 0;
 *     prop = cur cos(theta) + nu sin(theta)                   (u1, u2: words (0, 1) and (2, 3) of the purpose-8 block, index 0)
 *   writes nu, prop, prop_op, slot 0 of sq_parts, es (sse_cur and lp_cur [C] copied from the arguments) and ei (zeros).
 * qn_ess_iter: with sse_prop [C, nparts] (summed left to right) the SSE of the pending proposals, for every chain with t < nmcmc:
 *   - accept iff sse_prop is finite and gs sse_prop > logy (NaN: no): cur <- prop, sse_cur <- sse_prop,
 *       lp_cur = (gs sse_prop - (n_rows / 2) log 2 pi - n_rows log sigma) + (-0.5 |prop|^2 / priorsigma^2 - (p / 2) log(2 pi priorsigma^2)),
 *     chain[c, t + 1, :] <- prop (chain [C, nmcmc + 1, p] or NULL), lps[c, t + 1] = lp_cur, nev[c, t + 1] = j + 1 (int32
 *     [C, nmcmc + 1]), best [C, p] <- prop where lp_cur >= best_lp, t += 1; if t < nmcmc the next step starts as in qn_ess_begin;
 *   - else, j + 1 < max_shrink: theta < 0 ? tmin = theta : tmax = theta; theta = tmin + u (tmax - tmin) (u: words (0, 1) of
 *     the purpose-8 block, index j + 1); j += 1; prop = cur cos(theta) + nu sin(theta);
 *   - else (truncation): the chain stays: chain[c, t + 1, :] <- cur, lps[c, t + 1] = lp_cur, nev[c, t + 1] = max_shrink,
 *     ntrunc += 1, t += 1, and the next step starts;
 *   nevals += 1 in every case.  A chain with t == nmcmc is done: none of its arrays is read or written, its scalars are copied.
 * cos / sin of the angle are float64.  No atomics, no fences: equal inputs give equal bits, and a chain's result does not
 * depend on C, on its place in the launch, or on what the other chains do.
 * QN_EINVAL with a message, before any pointer is touched: C outside 1 .. 65535; chain0 < 0; p < 1; nmcmc, max_shrink, nparts
 *   or n_rows < 1; priorsigma or sigma not > 0 or not finite; a parity other than 0 / 1; a dtype other than the two; prop_op with
 *   QN_F64; a NULL pointer other than chain / prop_op. */
int qn_ess_begin(const double* cur, const double* sse_cur, const double* lp_cur, double sigma, double priorsigma, int C,
                 int chain0, int64_t p, uint64_t seed, double* nu, double* prop, void* prop_op, int dtype, double* sq_parts,
                 double* es, int64_t* ei, void* stream);
int qn_ess_iter(const double* sse_prop, int nparts, double sigma, double priorsigma, int n_rows, int max_shrink, int C, int chain0,
                int64_t p, int nmcmc, uint64_t seed, double* cur, double* nu, double* prop, void* prop_op, int dtype, double* best,
                double* best_lp, double* chain, double* lps, int32_t* nev, double* sq_parts, double* es, int64_t* ei, int parity,
                void* stream);

/* The No-U-Turn sampler on the device (Hoffman & Gelman 2014 with the multinomial weights of Betancourt 2017: biased
 * progressive sampling between subtrees, uniform within a subtree; build-only, the reference has no such sampler): no
 * trajectory length.  The ITERATIVE form: one leapfrog, that is one gradient call, per iteration; every U-turn test of the
 * trajectory's binary tree is made from checkpoints.  The chains' steps are ASYNCHRONOUS: every chain has its own step t, its
 * own tree (d doublings merged, leaf i of the subtree being built, direction v) and ends its step when ITS tree does.  A run
 * is qn_nuts_begin, then (qn_mlp_sse_fwdbwd at q, qn_prior_fold if there is a prior, qn_nuts_iter) until every chain has made
 * nmcmc steps.  quinn_amd/mcmc/nuts.py states the rule in full and restates it in numpy; its recursive builder is the authority.
 * Whitened momenta u = scale * r as in qn_hmc_begin_s (scale [C, p] or NULL = 1): kinetic energy |u|^2 / 2, U-turn tests are
 * dot products.  lp = gs sse - (n_rows / 2) log 2 pi - n_rows log sigma, force gs g, gs = -0.5 / sigma^2, g = d sse / d w float64.
 * With hk = v ((eps / 2) gs), dr = v eps: u_half = u + (hk scale) g, q' = q + (dr scale) u_half, u' = u_half + (hk scale) g'
 * -- one rounding per operation, no contraction: the elementwise results equal numpy's bit for bit.
 * Philox4x32-10 keyed by (seed, stream = the chain's step t, counter = [GLOBAL chain id = chain0 + c : 24][purpose : 4]
 * [index : 36]): purpose 9 = the momenta (index = column pair; the float32-transcendental normals of the HMC momenta), purpose
 * 10 = the scalar uniforms, index (kind << 32) | n: kind 0 the direction of doubling n (v = +1 iff u < 0.5), kind 1 the merge
 * of doubling n, kind 2 the leaf whose n_leap was n before the increment.
 * Per-chain state, double-buffered by the launch parity the caller alternates (slot `parity` is read, slot 1 - parity
 * written -- copied for done chains; slot 0 holds the state after qn_nuts_begin):
 *     es [2, C, 12] float64 = (eps, mu, hbar, logbar, H0, logW, logW_sub, sum_a, sse_cur, lp_cur, sse_sub, lp_sub)
 *         (eps: the chain's step size, written only by the in-kernel dual averaging; H0 is formed at a step's first leaf)
 *     ei [2, C, 8] int64 = (t, d, i, v, n_leap, ndiv, ntreedepth, ngrad)        best_lp [2, C]
 *     zz_parts [2, C, qn_hmc_parts(p)]: partial sums of squares of a step's momenta (the next launch adds them for H0)
 * and the float64 vectors, updated in place (an element belongs to one thread): cur, gcur (the tree's proposal and its
 * gradient -- at a step's start and end the chain's current point), the edges ql, ul, gl, qr, ur, gr, rho, the pending point q
 * with the half-kicked momentum u, of the subtree rho_sub, sub_q, sub_g and the checkpoints ck_u, ck_rho [C, max_depth, p], and
 * best: (15 + 2 max_depth) p doubles per chain, the gradient array of the operator and the stored chain not counted.
 * dot_parts [C, qn_hmc_parts(p), 27] is scratch of one call (fixed-order partial sums: slot 0 |u'|^2; 1 + 2k, 2 + 2k checkpoint
 * k; 25, 26 the tree), added left to right: the order depends on p alone.
 *
 * qn_nuts_begin: start of step 0 of every chain from cur, gcur [C, p] and sse_cur [C] with the step sizes eps0 [C]:
 *     z ~ N(0, I); both edges = (cur, z, gcur), rho = z, logW = 0, d = i = n_leap = 0, sum_a = 0, v = direction of doubling 0,
 *     u = z + (hk scale) gcur, q = cur + (dr scale) u; es (mu = log(10 eps0), hbar = logbar = 0), ei, best_lp = lp_cur, slot 0.
 * qn_nuts_iter: with sse [C] and grad [C, p] of the pending points q, for every chain with t < nmcmc -- leaf i of 2^d:
 *     u' = u + (hk scale) grad; rho_sub = (i == 0 ? u' : rho_sub + u'); dE = (-lp' + |u'|^2 / 2) - H0, NaN counted as +inf;
 *     sum_a += min(1, exp(-dE)); n_leap += 1; ngrad += 1; the leaf is divergent iff dE > 1000: the step ends, ndiv += 1;
 *     logW_sub = (i == 0 ? -dE : logaddexp(logW_sub, -dE)); with probability exp(-dE - logW_sub) the leaf becomes the subtree's
 *     proposal (sub_q, sub_g, sse_sub, lp_sub);
 *     i even, i + 1 < 2^d: ck_u[k] = u', ck_rho[k] = rho_sub for k = popcount(i >> 1) =: idx_max;
 *     i odd: for k = idx_max .. idx_max - (trailing one bits of i) + 1, r = (rho_sub - ck_rho[k]) + ck_u[k]: the subtree turns
 *     iff r . ck_u[k] <= 0 or r . u' <= 0, and the step ends;
 *     i + 1 < 2^d: i += 1, the next leapfrog starts from the leaf (u, q as above);
 *     i + 1 == 2^d: with probability min(1, exp(logW_sub - logW)) (cur, gcur, sse_cur, lp_cur) <- the subtree's proposal;
 *     logW = logaddexp(logW, logW_sub); d += 1; with rho' = rho + rho_sub and the edge on side v = the leaf, the step ends if
 *     rho' . ul <= 0 or rho' . ur <= 0, or else if d == max_depth (ntreedepth += 1); otherwise rho = rho', the edge is stored, a
 *     new direction is drawn and leaf 0 starts from that side's edge.  The classic criterion: Stan's later extra checks across
 *     adjacent subtrees are not made.
 *   Step end: chain[c, t + 1, :] <- cur (chain [C, nmcmc + 1, p] or NULL), lps[c, t + 1] = lp_cur, alphas[c, t + 1] = sum_a /
 *     n_leap, depth[c, t + 1] = the doublings started (d, or d + 1 when the step ended inside a subtree), nleap[c, t + 1] =
 *     n_leap (int32 [C, nmcmc + 1]); best [C, p] <- cur where lp_cur >= best_lp; if t < adapt, eps is dual-averaged as by
 *     qn_hmc_adapt (same constants and formula, m = t + 1, a = sum_a / n_leap, NaN counted as 0) and frozen to exp(logbar) at
 *     t == adapt - 1 (the step size only: no mass windows); t += 1; if t < nmcmc the next step starts as in qn_nuts_begin.
 *   A chain with t == nmcmc is done: none of its arrays is read or written, its scalars are copied.  (So is a chain whose
 *   caller-written counters could index outside an array: d outside 0 .. max_depth - 1, i outside 0 .. 2^d - 1, t < 0.)
 * Two launches (reduce; decide and move) on the qn_hmc_parts(p)-workgroups-per-chain grid.  No atomics, no fences: equal inputs
 * give equal bits, and a chain's result does not depend on C, on its place in the launch, or on what the other chains do.
 * QN_EINVAL with a message, before any pointer is touched: C outside 1 .. 65535; chain0 < 0; p < 1; n_rows < 1; nmcmc < 1;
 *   max_depth outside 1 .. 12; adapt outside 0 .. nmcmc; target_accept outside (0, 1); sigma not > 0 or not finite; a parity
 *   other than 0 / 1; a NULL pointer other than chain / scale. */
int qn_nuts_begin(const double* sse_cur, const double* eps0, const double* scale, double sigma, int n_rows, int C, int chain0,
                  int64_t p, uint64_t seed, const double* cur, const double* gcur, double* ql, double* ul, double* gl, double* qr,
                  double* ur, double* gr, double* rho, double* q, double* u, double* zz_parts, double* best_lp, double* es,
                  int64_t* ei, void* stream);
int qn_nuts_iter(const double* sse, const double* grad, const double* scale, double sigma, int n_rows, int max_depth, int adapt,
                 double target_accept, int C, int chain0, int64_t p, int nmcmc, uint64_t seed, double* cur, double* gcur,
                 double* ql, double* ul, double* gl, double* qr, double* ur, double* gr, double* rho, double* q, double* u,
                 double* rho_sub, double* sub_q, double* sub_g, double* ck_u, double* ck_rho, double* best, double* best_lp,
                 double* chain, double* lps, double* alphas, int32_t* depth, int32_t* nleap, double* dot_parts, double* zz_parts,
                 double* es, int64_t* ei, int parity, void* stream);

/* Moments of a predictive ensemble on the device (QUiNNBase.predict_mom_sample, quinn/solvers/quinn.py:75-104):
 * Y [M, K] dtype = M members x K = N * o prediction entries as qn_mlp_sse_fwd writes them ([B, Nb, o] with B = M);
 * mean_out [K], var_out [K] (unbiased, ddof = 1; NULL to skip; needs M >= 2), float64.  The per-output covariance of
 * msc = 2 is a plain GEMM of the centred ensemble and is left to the BLAS of the host side. */
int qn_pred_moments(const void* Y, int dtype, int64_t M, int64_t K, double* mean_out, double* var_out, void* stream);

/* Curvature of the data term for the Laplace approximation (quinn/solvers/nn_laplace.py:76-122, quinn/nns/nnwrap.py:153-229),
 * in plain float64 arithmetic (accurate tanh, no int8-slice kernels; the result is inverted by the caller).  Arguments as
 * qn_mlp_sse_fwdbwd: W [B, p], shared X [N, d] / Y [N, o], optional row_idx [B, Nb]; r_bn = f_{W[b]}(x) - y of row n of member b.
 *   QN_CURV_HESS_FULL  out [B, p, p]: the exact Hessian d2/dW2 sum_n |r_bn|^2 / 2 (residual curvature included, so it can be
 *                      indefinite); both triangles are written and the matrix is symmetric bit for bit.  p <= 16384.
 *   QN_CURV_EF_DIAG    out [B, p]: the empirical-Fisher diagonal (1/Nb) sum_n (d/dW_j |r_bn|^2 / 2)^2.
 *   QN_CURV_GGN_FULL   out [B, p, p]: the generalised Gauss-Newton matrix sum_n sum_k J_nk^T J_nk, J_nk = d f_k(x_n) / dW (the
 *                      Hessian without its residual term: positive semi-definite by construction); both triangles, symmetric
 *                      bit for bit.  p <= 16384.
 *   QN_CURV_GGN_DIAG   out [B, p]: its diagonal sum_n sum_k J_nk[j]^2 -- a SUM over the rows, where EF_DIAG is a MEAN over the
 *                      rows (and squares the residual-weighted gradient).  No p limit.
 * The GGN kinds do not read Y (it may be NULL).
 * The 1/sigma^2 (FULL) and 1/sigma^4 (DIAG) scales of the reference's NegLogPost are the caller's.  Any MLP descriptor
 * (tanh / relu / identity, with or without bias); a residual-network descriptor, an unknown kind or a FULL kind with p > 16384 is
 * QN_EINVAL with a message.  Sums run in a fixed order with no atomics: two calls give the same bits.
 * qn_curv_workspace_bytes returns 0 for arguments qn_mlp_curv refuses (qn_last_error() says why); it needs no device. */
#define QN_CURV_HESS_FULL 0
#define QN_CURV_EF_DIAG   1
#define QN_CURV_GGN_FULL  2
#define QN_CURV_GGN_DIAG  3
size_t qn_curv_workspace_bytes(const qn_desc* desc, int kind, int B, int Nb);
int qn_mlp_curv(const qn_desc* desc, int kind, const double* W, const double* X, const double* Y,
                const int32_t* row_idx, int B, int N, int Nb, double* out,
                void* workspace, size_t workspace_bytes, void* stream);

/* Linearised ("GLM") predictive of a Gaussian weight posterior N(W[b], Sigma[b]) of an MLP, float64, in closed form:
 *   mean_out [B, N, o]     f_{W[b]}(x_n)
 *   cov_out  [B, N, o, o]  J_nk Sigma[b] J_nl^T,  J_nk = d f_k(x_n) / dW at W[b] (flat parameter order)
 * QN_GLM_COV_FULL: Sigma [B, p, p] (read as given, row P times column Q; meant to be symmetric), p <= 16384;
 * QN_GLM_COV_DIAG: Sigma [B, p], the diagonal.  X [N, d] are the query points, shared by the members.
 * J is never stored: T = J Sigma is a GEMM on v_mfma_f64_16x16x4_f64 whose A operand is formed from the per-row backward
 * signals and layer inputs, and the epilogue contracts each accumulator tile with the matching J entries, so T stays on the
 * chip as well.  Entries (k, l) and (l, k) are one computed number.  Fixed summation order, no atomics: two calls give the
 * same bits and the result of a member does not depend on B.  A residual-network descriptor, an unknown cov_kind or
 * COV_FULL with p > 16384 is QN_EINVAL with a message; qn_glm_workspace_bytes returns 0 for those (qn_last_error() says why)
 * and needs no device.  The workspace holds B x min(N, 4096) rows of layer inputs and backward signals, never N x p. */
#define QN_GLM_COV_FULL 0
#define QN_GLM_COV_DIAG 1
size_t qn_glm_workspace_bytes(const qn_desc* desc, int cov_kind, int B, int N);
int qn_mlp_glm_predict(const qn_desc* desc, int cov_kind, const double* W, const double* X, const double* Sigma, int B, int N,
                       double* mean_out, double* cov_out, void* workspace, size_t workspace_bytes, void* stream);

/* Derivatives with respect to the INPUTS of an MLP, float64 (plain arithmetic, accurate tanh), and the derivative-informed
 * loss of the reference's GradLoss (quinn/nns/losses.py:84-145) with its weight gradient.  Arguments as qn_mlp_sse_fwdbwd:
 * W [B, p], shared X [N, d], optional row_idx [B, Nb] (member b sees rows row_idx[b]; without it Nb == N).
 * qn_mlp_input_jac:  jac_out [B, Nb, o, d] = d f_k(x_n) / d x_j at W[b];  pred_out [B, Nb, o] = f (or NULL).
 * qn_mlp_sobolev_fwdbwd:  sse_out [B] = sum_n |f - y|^2,  gsse_out [B] = sum_n sum_kj (J_kj - G_kj)^2 (either may be NULL),
 *   gradW_out [B, p] = wv d sse / dW + wg d gsse / dW, or NULL (values only).  Y [N, o] may be NULL when wv == 0 and
 *   sse_out == NULL; G [N, o, d], the gradient observations indexed by the same rows as X, may be NULL when wg == 0 and
 *   gsse_out == NULL.
 * A data row and its d input tangents are 1 + d rows of one matrix: the tangent forward, the adjoint pass and the weight
 * gradient (a reverse pass over the forward-mode pass) are matrix products over those rows on v_mfma_f64_16x16x4_f64, with
 * one fused elementwise kernel per layer and direction in between.  Any MLP descriptor (tanh / relu / identity, with or without
 * bias) with d <= 16 and o <= 16; a residual-network descriptor, d > 16 or o > 16 is QN_EINVAL with a message before any
 * pointer is touched, and qn_sobolev_workspace_bytes returns 0 for those (qn_last_error() says why; it needs no device).
 * Rows go in tiles of at most 2048 (fewer for wide networks: 256 MB of extended rows per member); the workspace is B times
 * that plus a slab of weight-gradient partial sums, never N x p.  Sums run in a fixed order with no atomics: two calls give
 * the same bits and a member's result does not depend on B.  want_grad = 0 sizes the workspace of qn_mlp_input_jac and of
 * qn_mlp_sobolev_fwdbwd without gradW_out. */
size_t qn_sobolev_workspace_bytes(const qn_desc* desc, int B, int Nb, int want_grad);
int qn_mlp_input_jac(const qn_desc* desc, const double* W, const double* X, const int32_t* row_idx, int B, int N, int Nb,
                     double* pred_out, double* jac_out, void* workspace, size_t workspace_bytes, void* stream);
int qn_mlp_sobolev_fwdbwd(const qn_desc* desc, const double* W, const double* X, const double* Y, const double* G,
                          const int32_t* row_idx, int B, int N, int Nb, double wv, double wg, double* sse_out,
                          double* gsse_out, double* gradW_out, void* workspace, size_t workspace_bytes, void* stream);

/* SWAG (quinn/solvers/nn_swag.py): the SGD phase of swag_calc and the posterior draws of predict_sample, float64 state.
 * qn_swag_step: one pass over the B x p parameters of W [B, p]; by mode
 *   QN_SWAG_INIT          m1 = W, m2 = W * W (G, lr, D unused)
 *   QN_SWAG_SGD           W -= lr[b] * (G * gscale)  (G [B, p] of dtype gdtype = QN_F64 / QN_F32, lr [B])
 *   QN_SWAG_SGD_COLLECT   the SGD step, then with the new W and n (the collections already averaged, >= 1, used as a double):
 *                         m1 = (n m1 + W) / (n + 1),  m2 = (n m2 + W * W) / (n + 1)  and, if D is not NULL, row `slot` of the
 *                         ring buffer D [B, K, p] gets W - m1 (the updated mean).
 *   Numpy's order of operations with one rounding each (no contraction, IEEE division): the result equals numpy's bit for bit.
 * qn_swag_sample: M draws; draw s uses member js[s] (int32 [M], each in [0, B)), z1 [M, p] and, when D is not NULL, z2 [M, K]:
 *   corr = sqrt(.5) * (sqrt(diag_j) * z1_s) + sqrt(.5) * (D_j z2_s) / sqrt(K - 1)   (D [B, K, p], rows oldest to newest)
 *   corr = sqrt(diag_j) * z1_s                                                    (D NULL: diagonal covariance)
 *   theta[s] = mean_j + corr.  drift = 1: mean_j = theta[s] afterwards, in sample order (the reference's in-place
 *   `theta += corr`); drift = 0: mean is not written.  A negative diag entry gives NaN, as np.sqrt does.  Only D_j z2_s
 *   is summed in an order of its own; everything else equals numpy's bit for bit.  mean [B, p], diag [B, p], theta [M, p]. */
#define QN_SWAG_INIT        0
#define QN_SWAG_SGD         1
#define QN_SWAG_SGD_COLLECT 2
int qn_swag_step(int mode, double* W, const void* G, int gdtype, const double* lr, double gscale, double* m1, double* m2,
                 double* D, int K, int slot, int64_t n, int B, int64_t p, void* stream);
int qn_swag_sample(double* mean, const double* diag, const double* D, int K, const int32_t* js, const double* z1,
                   const double* z2, int M, int B, int64_t p, int drift, double* theta, void* stream);

/* Kronecker-factored Gauss-Newton of an MLP ("kron" Laplace), float64.  With ~in_i = [in_i; 1] (length e_i = h_i + has_bias) the
 * input of Linear layer i and g^k_i the backward signal at its output from output unit vector e_k, the factors are the SUMS
 *   A_i = sum_n ~in_i ~in_i^T  [e_i, e_i],     S_i = sum_n sum_k g^k_i g^k_i^T  [h_{i+1}, h_{i+1}]
 * over a member's rows; the layer-i diagonal block of sum_n sum_k J_nk^T J_nk is approximated by (S_i (x) A_i) / Nb, row index
 * (unit a, input slot b), cross-layer blocks by zero (exact for Nb = 1, and for the last layer at every Nb).
 * qn_kron_layout: offsets of the layers in a member's packed factors (offA, offS: arrays of nlayers entries, A_i at offA[i] of
 *   lenA = sum e_i^2 doubles, S_i at offS[i] of lenS = sum h_{i+1}^2) and in KRON ORDER of a length-p vector: layer i, unit a,
 *   slot c < e_i at offK[i] + a e_i + c -- not the flat parameter order when there are biases.  Any pointer may be NULL.
 * qn_mlp_kron_factors: A_out [B, lenA], S_out [B, lenS]; the other arguments as for qn_mlp_curv (Y is not needed).  Symmetric
 *   rank-k updates over row tiles on v_mfma_f64_16x16x4_f64; one triangle is computed and mirrored, so both triangles are written
 *   and equal bit for bit.  Row-chunk partial sums in the workspace are added in a fixed order, no atomics: two calls give the
 *   same bits and a member's result does not depend on B.
 * qn_mlp_kron_glm_predict: the linearised predictive of qn_mlp_glm_predict for the posterior whose layer-i covariance is
 *   (U_S (x) U_A) diag(Dinv_i) (U_S (x) U_A)^T.  UA [B, lenA], US [B, lenS]: the eigenvector matrices of the factors (eigenvectors
 *   in the COLUMNS, row-major, packed like the factors); Dinv [B, p] in kron order: the variance of pair (a, c).
 *     cov_out[b][n][k][l] = sum_i sum_{a,c} Dinv_i[a][c] gh^k_a gh^l_a ah_c^2,   gh^k = U_S^T g^k_i,  ah = U_A^T ~in_i at x_n
 *   The rotations and the product (ah o ah) Dinv_i^T run on the f64 MFMA; the latter's accumulator tile is contracted with
 *   gh^k o gh^l in the epilogue and never leaves the chip.  Entries (k, l) and (l, k) are one computed number; fixed summation
 *   order, independent of B.  The workspace holds B x min(N, 1024) rows of layer inputs and backward signals, never N x p.
 * qn_kron_sample: W_out [M, p] (flat order): draw m of member js[m] (int32 [M]) with the standard normals Z[m] ([M, p], flat
 *   order): layer block = mean + U_S (Z_i o Dih_i) U_A^T, Z_i[a][b] the number at the flat position of parameter (i, a, b),
 *   mean [B, p] flat, Dih [B, p] kron order (the standard deviation of pair (a, c)).  One launch for all M <= 65535 draws.
 * Any MLP descriptor (tanh / relu / identity, with or without bias), layer widths up to 512, no limit on p.  A residual-network
 * descriptor or a wider layer is QN_EINVAL with a message; the two workspace queries then return 0 (qn_last_error() says why).
 * qn_kron_layout and the workspace queries need no device. */
int qn_kron_layout(const qn_desc* desc, int64_t* offA, int64_t* offS, int64_t* offK, int64_t* lenA, int64_t* lenS);
size_t qn_kron_workspace_bytes(const qn_desc* desc, int B, int Nb);
int qn_mlp_kron_factors(const qn_desc* desc, const double* W, const double* X, const int32_t* row_idx, int B, int N, int Nb,
                        double* A_out, double* S_out, void* workspace, size_t workspace_bytes, void* stream);
size_t qn_kron_glm_workspace_bytes(const qn_desc* desc, int B, int N);
int qn_mlp_kron_glm_predict(const qn_desc* desc, const double* W, const double* X, const double* UA, const double* US,
                            const double* Dinv, int B, int N, double* mean_out, double* cov_out, void* workspace,
                            size_t workspace_bytes, void* stream);
int qn_kron_sample(const qn_desc* desc, const double* mean, const double* UA, const double* US, const double* Dih,
                   const int32_t* js, const double* Z, double* W_out, int M, void* stream);

/* Multi-chain MCMC diagnostics: the per-chain statistics from which split-R-hat, batch-means ESS and pooled moments follow
 * (quinn_amd/mcmc/diagnostics.py combines them; the reference runs one chain and has no counterpart).
 * chain [C, T, K] contiguous, dtype QN_F64 or QN_F32 (a stored chain, a log-posterior trace with K = 1, or the predictions
 * [C, nens, N * o] of thinned draws).  Rows t0 .. t0 + 2 * nbatch * blen - 1 of every chain are used: two HALVES (h = 0, 1) of
 * nbatch batches of blen consecutive rows each, n = nbatch * blen rows per half.  stats [C, 6, K] float64; for chain c, entry k:
 *   row h      mean_h      = mean of the half's n rows
 *   row 2 + h  M2_h        = sum over the half's rows of (x - mean_h)^2
 *   row 4 + h  Sb_h        = sum over the half's nbatch batches of (batch mean - mean_h)^2
 * Float64 accumulation whatever the input type, on shifted values (x minus the first row of its batch; batch means relative to
 * the first row of the half), so a large common offset costs no digits.  Every batch of every (c, k) is summed by ONE thread in
 * row order and the batches of a half are merged in batch order: the summation order depends on (nbatch, blen) only -- not on
 * C, K, t0 or the launch geometry -- there are no atomics, and two calls give the same bits; statistics of a sub-stack of
 * chains equal the corresponding rows of the whole stack's bit for bit.  A NaN / Inf at (c, t, k) makes rows h, 2 + h, 4 + h of
 * (c, k) not-finite for the half h that holds t and changes nothing else.
 * Needs 1 <= C <= 32767, t0 >= 0, nbatch >= 2, blen >= 1, t0 + 2 * nbatch * blen <= T, else QN_EINVAL with a message before any
 * pointer is touched; qn_chain_stats_workspace_bytes returns 0 for such arguments (qn_last_error() says why) and needs no
 * device.  The workspace ([C, 2 nbatch, 2, K] float64 batch statistics) needs no initialisation and keeps no state. */
size_t qn_chain_stats_workspace_bytes(int C, int64_t T, int64_t K, int nbatch, int64_t blen);
int qn_chain_stats(const void* chain, int dtype, int C, int64_t T, int64_t K, int64_t t0, int nbatch, int64_t blen,
                   double* stats, void* workspace, size_t workspace_bytes, void* stream);

/* Scores of a predictive ensemble against data (quinn_amd/scoring.py forms the scalar summaries; the reference has no
 * counterpart, these formulas are the contract).  F [M, K] contiguous, dtype QN_F64 or QN_F32: member m's predictive mean of
 * entry k -- what qn_mlp_sse_fwd writes as pred_out with B = M, K = N * o.  V [M, K] of the same dtype or NULL: a
 * per-member predictive variance.  Y [K] float64: the targets, shared by the members.  Member m predicts
 * N(f_mk, s_mk^2), s_mk^2 = sigma^2 + V_mk, and the predictive is the equal-weight mixture of the members.  With
 * ll_mk = -0.5 (y_k - f_mk)^2 / s_mk^2 - 0.5 log(2 pi s_mk^2), out [QN_SCORE_NOUT, K] float64 holds per entry:
 *   row 0  lppd    logsumexp_m ll_mk - log M                                             (QN_SCORE_LPPD)
 *   row 1  p_waic  variance (ddof = 1) over the members of ll_mk                          (QN_SCORE_PWAIC)
 *   row 2  pit     (1/M) sum_m Phi((y_k - f_mk) / s_mk); a member with s_mk = 0 counts 1 / 0.5 / 0 for f < y, f == y, f > y
 *                                                                                        (QN_SCORE_PIT)
 *   row 3  crps    (1/M) sum_i A(y_k - f_ik, s_ik^2) - (1/(2 M^2)) sum_i sum_j A(f_ik - f_jk, s_ik^2 + s_jk^2), with
 *                  A(mu, s^2) = 2 s phi(mu/s) + mu (2 Phi(mu/s) - 1) and A(mu, 0) = |mu|   (QN_SCORE_CRPS)
 *   row 4, 5       mean and variance (ddof = 1) over the members of f_mk                   (QN_SCORE_MOMENTS)
 * Rows that `what` does not ask for are left untouched.  All arithmetic is float64 whatever the input type.  The log-sum-exp
 * keeps a running maximum and both variances are Welford recurrences: a common offset of ll costs no digits and identical
 * members give exactly 0.  The CRPS pair sum is O(M^2 K) (only j <= i is evaluated); with sigma = 0 and V = NULL it is the
 * ensemble CRPS, with no transcendental.  Every sum runs in an order fixed by M alone, without atomics: an entry's six numbers
 * do not depend on K, on the other entries of the call or on the launch geometry, and two calls give the same bits.
 * A non-finite f, V or y, or sigma^2 + V_mk < 0, makes the requested rows of THAT entry NaN and changes no other entry; with
 * V given, s_mk = 0 at an entry makes lppd and p_waic of that entry NaN (pit and crps take the degenerate forms above).
 * QN_EINVAL with a message, before any pointer is touched: M < 2, K < 1, a bad dtype, what == 0 or unknown bits, sigma < 0
 * or not finite, LPPD / PWAIC / PIT with sigma == 0 and V == NULL, a NULL F, Y or out (or workspace, if the CRPS is asked);
 * a workspace that is too small is QN_EWORKSPACE.  qn_pred_score_workspace_bytes returns 0 for (M, K, what) the call would
 * refuse (qn_last_error() says why) and needs no device; it is never 0 otherwise.  The workspace ([ceil(M / 32), K] float64
 * partial pair sums) needs no initialisation and keeps no state. */
#define QN_SCORE_LPPD 1
#define QN_SCORE_PWAIC 2
#define QN_SCORE_PIT 4
#define QN_SCORE_CRPS 8
#define QN_SCORE_MOMENTS 16
#define QN_SCORE_NOUT 6
size_t qn_pred_score_workspace_bytes(int64_t M, int64_t K, int what);
int qn_pred_score(const void* F, const void* V, int dtype, const double* Y, int64_t M, int64_t K, double sigma, int what,
                  double* out /* [QN_SCORE_NOUT, K] float64 */, void* workspace, size_t workspace_bytes, void* stream);

/* Diagnostic: y[i] = device tanh(x[i]) in float64 (the activation used by every kernel). */
int qn_debug_tanh(const double* x, double* y, int64_t n, void* stream);
/* Diagnostic: the variant the fused kernels use when all weights and inputs are finite and bounded
 * (no NaN handling; same values for every non-NaN input). */
int qn_debug_tanh_finite(const double* x, double* y, int64_t n, void* stream);
/* Diagnostic: the table-assisted tanh of the fused kernels (tanh(n/16) from LDS + a short polynomial;
 * nansafe = 1: NaN-propagating variant, 0: the variant for arguments that cannot be NaN; 2: the absolute-accuracy variant
 * of the int8-slice forward kernel (tanh(n/64) table, arguments that cannot be NaN). */
int qn_debug_tanh_table(const double* x, double* y, int64_t n, int nansafe, void* stream);

const char* qn_last_error(void);
/* "quinn_amd <version> gfx950" */
const char* qn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QUINN_AMD_H */
