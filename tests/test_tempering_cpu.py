"""CPU: the replica-exchange contract (`quinn_amd.mcmc.tempering`) that the device kernels are checked against -- ladder, pair
scheme, swap uniform, exchange round, round trips -- a numpy HMC that needs the ladder to cross a barrier, and the argument
refusals of qn_pt_swap that need no device."""
import numpy as np
import pytest

from quinn_amd import _lib
from quinn_amd.mcmc import tempering as pt


def test_ladder_values_and_refusals():
    b = pt.ladder(4, 0.001)
    assert b.shape == (4,) and b[0] == 1.0 and b[-1] == 0.001
    assert np.allclose(b, [1.0, 0.1, 0.01, 0.001], rtol=1e-14)
    assert np.array_equal(pt.ladder(2, 0.5), [1.0, 0.5])
    assert np.array_equal(pt.ladder([1.0, 0.3, 0.2]), [1.0, 0.3, 0.2])
    for bad in (1, 0, -3, 2.5, True):
        with pytest.raises(ValueError):
            pt.ladder(bad, 0.1)
    for bm in (0.0, 1.0, -0.1, 2.0):
        with pytest.raises(ValueError):
            pt.ladder(3, bm)
    for seq in ([0.9, 0.5], [1.0], [1.0, 1.0], [1.0, 0.2, 0.3], [1.0, 0.0], [[1.0, 0.5]]):
        with pytest.raises(ValueError):
            pt.ladder(seq)


def test_check_temper_args():
    assert np.array_equal(pt.check_temper_args(2, 0.25, 3, C=8, chain0=4), [1.0, 0.25])
    for kw in (dict(swap_every=0), dict(swap_every=1.5), dict(swap_every=True), dict(C=7), dict(chain0=3), dict(use_graph=True)):
        with pytest.raises(ValueError):
            pt.check_temper_args(2, 0.25, **kw)
    with pytest.raises(ValueError):
        pt.check_whole_ladders(4, 8, 2)
    with pytest.raises(ValueError):
        pt.check_whole_ladders(4, 6, 0)
    pt.check_whole_ladders(4, 8, 4)


@pytest.mark.parametrize("R", [2, 3, 4, 5, 8])
def test_swap_pairs_cover_every_neighbour_pair_once_in_two_rounds(R):
    for k in (0, 1, 6):
        a, b = pt.swap_pairs(R, k), pt.swap_pairs(R, k + 1)
        assert sorted(a + b) == list(range(R - 1))              # each pair (r, r + 1) exactly once
        for pairs in (a, b):
            assert all(r2 - r1 >= 2 for r1, r2 in zip(pairs, pairs[1:]))      # pairs of one round are disjoint
        assert a == pt.swap_pairs(R, k + 2)
    assert pt.swap_pairs(R, 0)[0] == 0 and (R == 2 or pt.swap_pairs(R, 1)[0] == 1)


def test_swap_uniform_open_interval_and_distinct():
    chains = np.arange(4096)
    u = pt.swap_uniform(5, 11, chains)
    assert u.shape == (4096,) and np.all(u > 0.0) and np.all(u < 1.0)
    assert len(np.unique(u)) == 4096
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * 4096)
    v = pt.swap_uniform(5, 12, chains)
    assert not np.any(u == v)
    assert pt.swap_uniform(5, 11, 7) == u[7]
    assert not np.any(pt.swap_uniform(6, 11, chains) == u)


@pytest.mark.parametrize("R,K", [(2, 3), (3, 2), (4, 3), (5, 2)])
def test_swap_round_is_a_neighbour_permutation(R, K):
    rs = np.random.RandomState(R * 10 + K)
    C = R * K
    beta = np.tile(pt.ladder(R, 0.05), K)
    seen = set()
    for k in range(6):
        lp = -50.0 + 3.0 * rs.randn(C)
        u = rs.rand(C)
        sw, perm = pt.swap_round(lp, beta, R, k, u)
        assert sorted(perm) == list(range(C))
        assert np.array_equal(perm[perm], np.arange(C))         # an involution: disjoint transpositions
        moved = np.flatnonzero(perm != np.arange(C))
        assert np.all(np.abs(perm[moved] - moved) == 1) and np.all(perm[moved] // R == moved // R)
        for c in np.flatnonzero(sw):
            assert c % R in pt.swap_pairs(R, k) and perm[c] == c + 1 and perm[c + 1] == c
            d = (beta[c] - beta[c + 1]) * (lp[c + 1] - lp[c])
            assert u[c] < np.exp(d)
        assert np.array_equal(np.flatnonzero(sw), moved[perm[moved] > moved])
        seen |= set(sw[[c for c in range(C) if c % R in pt.swap_pairs(R, k)]])
    assert seen == {True, False}
    # a hotter state with a higher log-posterior always moves down; NaN / infinite log-posteriors never move
    lp = np.arange(C, dtype=np.float64)
    sw, _ = pt.swap_round(lp, beta, R, 0, np.full(C, 1.0 - 1e-16))
    assert all(sw[k * R + r] for k in range(K) for r in pt.swap_pairs(R, 0))
    for badv in (np.nan, -np.inf, np.inf):
        for at in (0, 1):
            lp2 = lp.copy()
            lp2[at] = badv
            assert not pt.swap_round(lp2, beta, R, 0, np.full(C, 1e-300))[0][0]
    with pytest.raises(ValueError):
        pt.swap_round(lp[:-1], beta[:-1], R, 0, lp[:-1])


def _double_well_run(R, nsteps, seed, beta_min=0.01, eps=0.05, L=5):
    """numpy HMC on pi ~ exp(-(w^2 - 1)^2 / 0.02), one ladder of R rungs (R = 1: no ladder) started in the right-hand well, an
    exchange round after every step.  Returns the cold chain's states."""
    rs = np.random.RandomState(seed)
    beta = pt.ladder(R, beta_min) if R > 1 else np.ones(1)
    lp = lambda w: -(w * w - 1.0) ** 2 / 0.02
    glp = lambda w: -4.0 * w * (w * w - 1.0) / 0.02
    w = np.ones(R)
    step = eps / np.sqrt(beta)
    out = np.empty(nsteps)
    for t in range(nsteps):
        r0 = rs.randn(R)
        q, r = w.copy(), r0 + 0.5 * step * beta * glp(w)
        for j in range(L):
            q = q + step * r
            r = r + (1.0 if j < L - 1 else 0.5) * step * beta * glp(q)
        with np.errstate(over='ignore', invalid='ignore'):
            mh = np.exp((-beta * lp(w) + 0.5 * r0 * r0) - (-beta * lp(q) + 0.5 * r * r))
        take = rs.rand(R) < mh
        w = np.where(take, q, w)
        if R > 1:
            _, perm = pt.swap_round(lp(w), beta, R, t, pt.swap_uniform(seed, t + 1, np.arange(R)))
            w = w[perm]
        out[t] = w[0]
    return out


def test_double_well_needs_the_ladder():
    """The barrier at w = 0 is 50 nats high: HMC alone never leaves the well it starts in (the fraction of rows with w < 0 is
    exactly 0), a ladder down to beta = 0.01 (a 0.5 nat barrier for the top rung) hands the cold chain both wells."""
    control = _double_well_run(1, 4000, seed=3)
    assert np.mean(control < 0) == 0.0
    cold = _double_well_run(6, 4000, seed=3)
    frac = np.mean(cold[500:] < 0)
    assert 0.2 < frac < 0.8, frac
    assert np.all(np.abs(np.abs(cold[500:]) - 1.0) < 0.5)       # the cold chain stays at the cold target's scale


def test_round_trips_hand_written_trace():
    # R = 3, one ladder; replica 0 climbs to the top and returns once, replica 2 comes down and only climbs back
    rep = np.array([[0, 1, 1, 2, 2, 0, 0],
                    [1, 0, 2, 1, 0, 2, 2],
                    [2, 2, 0, 0, 1, 1, 1]])
    assert np.array_equal(pt.round_trips(rep, 3), [1, 0, 0])
    # two ladders with an id offset (a group starting at global chain 6), R = 2: every exchange is a half trip
    rep2 = np.array([[6, 7, 6, 7, 6], [7, 6, 7, 6, 7], [8, 8, 8, 8, 8], [9, 9, 9, 9, 9]])
    assert np.array_equal(pt.round_trips(rep2, 2), [2, 1, 0, 0])
    assert np.array_equal(pt.round_trips(np.arange(4)[:, None], 2), [0, 0, 0, 0])


def test_c_abi_sizes_and_refusals_without_a_device():
    _lib.build()
    L = _lib.lib()
    for name in ("qn_hmc_begin_t", "qn_hmc_leap_t", "qn_hmc_accept_t", "qn_pt_swap"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.qn_hmc_parts(23) == 1 and L.qn_hmc_parts(8513) == 9         # the partial sums the _t kernels share with _s
    one = 8                                                                # a non-NULL pointer that is never touched
    ok = dict(cur=one, grad_cur=one, cur_lp=one, best_lp=one, lps=one, chain=None, beta=one, rid=one, rep=None, swap_acc=one,
              swap_try=one, step_ptr=one, R=2, round=0, nrounds=4, C=4, chain0=2, p=5, nmcmc=10, seed=1, parity=0, rid_parity=1, stream=None)
    for bad in (dict(R=1), dict(R=0), dict(R=3), dict(C=0), dict(C=5), dict(C=70000), dict(chain0=1), dict(chain0=-2), dict(p=0),
                dict(nmcmc=0), dict(round=-1), dict(round=4), dict(nrounds=0), dict(parity=2), dict(rid_parity=-1), dict(rid_parity=2), dict(cur=None), dict(grad_cur=None),
                dict(cur_lp=None), dict(best_lp=None), dict(lps=None), dict(beta=None), dict(rid=None), dict(swap_acc=None),
                dict(swap_try=None), dict(step_ptr=None)):
        args = dict(ok, **bad)
        assert L.qn_pt_swap(*args.values()) == -1, bad
        assert b"qn_pt_swap" in L.qn_last_error()
    assert L.qn_hmc_begin_t(None, one, 0.1, one, None, one, 4, 0, 5, 1, one, one, one, one, None) == -1
    assert b"qn_hmc_begin_t" in L.qn_last_error()
    assert L.qn_hmc_leap_t(None, 0, 0.1, one, None, one, 0, 4, 5, one, one, one, None) == -1
    assert b"qn_hmc_leap_t" in L.qn_last_error()
    assert L.qn_hmc_accept_t(one, one, one, one, one, 0.0, 8, 4, 0, 5, 10, 1, one, one, one, one, one, None, one, one, one, one, 0,
                             one, None) == -1
    assert b"qn_hmc_accept_t" in L.qn_last_error()
