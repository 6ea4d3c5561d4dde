"""Stochastic-gradient MCMC (SGLD, Welling & Teh 2011; SGHMC, Chen et al. 2014; cyclical step size, Zhang et al. 2020): the
contract of the device engines `DeviceSGLD` / `DeviceSGHMC` (qn_sg_rows / qn_sg_step, csrc/qn_sgmcmc.hip), restated in numpy.

Target: the Gaussian likelihood with noise sigma, U(theta) = SSE(theta) / (2 sigma^2) + const, as every sampler of this package
(with `priorsigma` the engines fold a Gaussian weight prior into SSE and gradient beforehand, unscaled by N / Nb:
`quinn_amd.mcmc.prior`).  Inner step t of a chain with minibatch rows B_t (Nb rows drawn uniformly WITH replacement from the N data rows):

    g   = (N / Nb) * d SSE_{B_t} / d theta / (2 sigma^2)          # unbiased estimate of the gradient of U
    eta = eta0                                                     schedule 'constant'
          eta0 / 2 * (cos(pi * (t mod K) / K) + 1)                 schedule 'cyclic', K inner steps per cycle
    on  = 1 ('constant');  (t mod K) / K >= explore_frac ('cyclic': the head of each cycle is plain SGD with momentum)
    v     <- (1 - alpha) v - eta g + on * sqrt(2 alpha eta T) z,   z ~ N(0, I)
    theta <- theta + v

alpha = 1 is SGLD (v is never read).  T is the temperature (1: the posterior; 0: no noise).  Random numbers are Philox4x32-10
blocks keyed by (seed, stream = t, counter = [global chain id : 24][purpose : 4][index : 36]): purpose 4 draws the rows
(`minibatch_rows`, pure integer arithmetic: the device rows equal it bit for bit), purpose 5 the noise.
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
PURPOSE_ROWS, PURPOSE_NOISE = 4, 5
SCHEDULES = ('constant', 'cyclic')


def philox4x32(seed, stream, ctr):
    """Philox4x32-10 (Salmon et al. 2011) with the device's layout: counter words (ctr lo, ctr hi, stream lo, stream hi),
    key (seed lo, seed hi).  ctr: uint64 array of any shape -> uint32 array [..., 4]."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    seed, stream = int(seed), int(stream)
    c0, c1 = ctr & _M32, ctr >> np.uint64(32)
    c2 = np.full_like(ctr, stream & 0xFFFFFFFF)
    c3 = np.full_like(ctr, (stream >> 32) & 0xFFFFFFFF)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    m0, m1, sh = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                                  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def ctr_of(chain, purpose, index):
    """The counter of one draw: [global chain id : 24][purpose : 4][index : 36] (csrc/qn_mcmc_shared.h)."""
    return (np.uint64(chain) << np.uint64(40)) | (np.uint64(purpose) << np.uint64(36)) | \
        (np.asarray(index, dtype=np.uint64) & np.uint64(0xFFFFFFFFF))


def minibatch_rows(seed, step, chain, N, Nb):
    """int32 [Nb]: the rows of GLOBAL chain `chain` at inner step `step`.  Entry j is floor(r * N / 2^32) with r = word j & 3
    of the block (seed, stream = step, ctr_of(chain, 4, j >> 2)): independent, uniform on [0, N), with replacement."""
    j = np.arange(int(Nb))
    blocks = philox4x32(seed, step, ctr_of(chain, PURPOSE_ROWS, np.arange((int(Nb) + 3) // 4)))
    r = blocks[j >> 2, j & 3].astype(np.uint64)
    return ((r * np.uint64(N)) >> np.uint64(32)).astype(np.int32)


def step_size(t, eta0, schedule='constant', K=None):
    """Step size of inner step t."""
    if schedule == 'constant':
        return float(eta0)
    return float(eta0) / 2 * (np.cos(np.pi * (t % K) / K) + 1)


def noise_on(t, K=None, explore_frac=0.0):
    """Whether inner step t draws noise: always without a cycle (K None); in a cycle once (t mod K) / K >= explore_frac."""
    if K is None:
        return True
    return (t % K) / K >= explore_frac


def grad_scale(N, Nb, sigma):
    """(N / Nb) / (2 sigma^2): what turns d SSE / d theta of a minibatch of Nb rows into the estimated gradient of U."""
    return (N / Nb) * (0.5 / (sigma * sigma))


def sg_step(theta, v, grad, z, eta, alpha, gscale, temperature=1.0, on=True):
    """One update with the caller's normals z: (theta', v').  grad = d SSE / d theta of the minibatch, gscale = `grad_scale`.
    alpha = 1 does not read v (None allowed)."""
    ns = np.sqrt(2.0 * alpha * eta * temperature) if on else 0.0
    vn = - eta * (gscale * grad) + ns * z
    if alpha != 1.0:
        vn = (1.0 - alpha) * v + vn
    return theta + vn, vn


def ula_cov(Lambda, eta):
    """Exact stationary covariance of full-batch SGLD with step eta on a Gaussian target of precision Lambda:
    inv(Lambda - eta Lambda^2 / 2) (theta' = (I - eta Lambda) theta + sqrt(2 eta) z leaves it invariant); the target's own
    covariance inv(Lambda) as eta -> 0."""
    Lambda = np.atleast_2d(np.asarray(Lambda, dtype=np.float64))
    return np.linalg.inv(Lambda - eta * (Lambda @ Lambda) / 2)


def check_sg_args(eta, alpha=1.0, batch=None, thin=1, schedule='constant', cycles=1, explore_frac=0.0, temperature=1.0,
                  nmcmc=None):
    """Refuses what the samplers cannot run; returns K, the inner steps per cycle (None for the constant schedule or while
    `nmcmc`, the number of stored rows, is unknown)."""
    if not float(eta) > 0.0:
        raise ValueError(f"eta = {eta!r}: the step size must be > 0")
    if not 0.0 < float(alpha) <= 1.0:
        raise ValueError(f"alpha = {alpha!r}: the friction must lie in (0, 1] (1 is SGLD)")
    if batch is not None and (isinstance(batch, bool) or int(batch) != batch or int(batch) < 1):
        raise ValueError(f"batch = {batch!r}: a minibatch has >= 1 rows (None: all rows)")
    if isinstance(thin, bool) or int(thin) != thin or int(thin) < 1:
        raise ValueError(f"thin = {thin!r}: every thin-th state is stored, thin >= 1")
    if schedule not in SCHEDULES:
        raise ValueError(f"schedule = {schedule!r}: 'constant' or 'cyclic'")
    if not float(temperature) >= 0.0:
        raise ValueError(f"temperature = {temperature!r}: must be >= 0")
    if schedule == 'constant':
        return None
    if isinstance(cycles, bool) or int(cycles) != cycles or int(cycles) < 1:
        raise ValueError(f"cycles = {cycles!r}: the cyclic schedule needs >= 1 cycles")
    if not 0.0 <= float(explore_frac) <= 1.0:
        raise ValueError(f"explore_frac = {explore_frac!r}: must lie in [0, 1]")
    if nmcmc is None:
        return None
    K = (int(nmcmc) * int(thin)) // int(cycles)
    if K < 2:
        raise ValueError(f"cycles = {cycles}: {nmcmc} stored rows x thin = {thin} leave {K} inner steps per cycle; need >= 2")
    return K
