"""CPU: which leapfrog / accept entry points `DeviceHMC._begin`, `_leap` and `_step` call for each shape of the run state, and
with which arguments in which order -- against the tuples written down by hand from the header (include/quinn_amd.h).  A wrong
argument order would go through ctypes unnoticed, so stub functions on a fake library record every call; no device is needed."""
import pytest

from quinn_amd.mcmc.device_hmc import DeviceHMC

SIGMA, EPSILON, CHAIN0, SEED, NMCMC, N_ROWS, QDT, C, P, STREAM = 0.25, 0.0125, 6, 991, 40, 48, 1, 4, 97, "stream"
NAMES = ["qn_hmc_begin", "qn_hmc_leap", "qn_hmc_accept", "qn_hmc_begin_s", "qn_hmc_leap_s", "qn_hmc_begin_t", "qn_hmc_leap_t",
         "qn_hmc_accept_t"]


class _T:
    """Stands for a device tensor: an address and a shape."""

    def __init__(self, addr):
        self.addr, self.shape = addr, (C, P)

    def data_ptr(self):
        return self.addr


class _Lib:
    def __init__(self, calls):
        for n in NAMES:
            setattr(self, n, lambda *a, _n=n: calls.append((_n, a)) or 0)


class _Op:
    qdt, N = QDT, N_ROWS

    def __init__(self, calls):
        self.calls = calls

    def sse_grad(self, q, out):
        self.calls.append(("sse_grad", (q.addr, out[0].addr, out[1].addr)))


class _Engine(DeviceHMC):
    def _stream(self):
        return STREAM


def _engine(L_):
    calls = []
    e = _Engine.__new__(_Engine)
    e.sigma, e.epsilon, e.L, e.chain0, e.seed, e._prior = SIGMA, EPSILON, L_, CHAIN0, SEED, None
    e._L, e.op = _Lib(calls), _Op(calls)
    return e, calls


KEYS = ['cur', 'gcur', 'mom', 'q', 'gq', 'sse', 'kcur', 'kprop', 'cur_lp', 'best', 'best_lp', 'chain', 'lps', 'alphas', 'nacc',
        'step', 'eps', 'scale', 'beta']
A = {k: 0x1000 * (i + 1) for i, k in enumerate(KEYS)}                     # the address of every array of the state


def _state(par, **extra):
    s = {k: _T(A[k]) for k in KEYS[:16]}
    s.update(par=par, qc=None, g64=None)
    s.update({k: (None if v is None else _T(A[k])) for k, v in extra.items()})
    return s


# state shape -> suffix of the begin / leap entry points, their step-size arguments, the accept entry point and its extra argument
SHAPES = {
    "plain": (dict(), "", (EPSILON,), "qn_hmc_accept", ()),
    "adapt, step size only": (dict(eps=1, scale=None), "_s", (A['eps'], None), "qn_hmc_accept", ()),
    "adapt": (dict(eps=1, scale=1), "_s", (A['eps'], A['scale']), "qn_hmc_accept", ()),
    "ladder": (dict(beta=1, eps=1), "_t", (A['eps'], None, A['beta']), "qn_hmc_accept_t", (A['beta'],)),
    "ladder + adapt, step size only": (dict(beta=1, eps=1, scale=None), "_t", (A['eps'], None, A['beta']), "qn_hmc_accept_t",
                                       (A['beta'],)),
    "ladder + adapt": (dict(beta=1, eps=1, scale=1), "_t", (A['eps'], A['scale'], A['beta']), "qn_hmc_accept_t", (A['beta'],)),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("par", [0, 1])
def test_begin_and_leap_pick_the_entry_point_from_the_state(shape, par):
    extra, sfx, step, _, _ = SHAPES[shape]
    e, calls = _engine(3)
    s = _state(par, **extra)
    e._begin(s, STREAM)
    e._leap(s, False, STREAM)
    e._leap(s, True, STREAM)
    assert calls == [
        ("qn_hmc_begin" + sfx, (A['cur'], A['gcur'], SIGMA) + step + (C, CHAIN0, P, SEED, A['step'] + 8 * par, A['mom'], A['q'],
                                                                      A['kcur'], STREAM)),
        ("qn_hmc_leap" + sfx, (A['gq'], QDT, SIGMA) + step + (0, C, P, A['mom'], A['q'], A['kprop'], STREAM)),
        ("qn_hmc_leap" + sfx, (A['gq'], QDT, SIGMA) + step + (1, C, P, A['mom'], A['q'], A['kprop'], STREAM))]
    assert all(type(a[-7]) is int for _, a in calls[1:])                      # `last` goes through ctypes as an int


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("L_", [1, 3])
def test_step_enqueues_begin_gradient_leap_accept_in_order(shape, L_):
    extra, sfx, step, accept, accept_extra = SHAPES[shape]
    e, calls = _engine(L_)
    s = _state(1, **extra)
    e._step(s, NMCMC)
    assert s['par'] == 0
    assert [n for n, _ in calls] == ["qn_hmc_begin" + sfx] + ["sse_grad", "qn_hmc_leap" + sfx] * L_ + [accept]
    assert [a[-7] for n, a in calls if n.startswith("qn_hmc_leap")] == [0] * (L_ - 1) + [1]
    assert all(a == (A['q'], A['sse'], A['gq']) for n, a in calls if n == "sse_grad")
    assert calls[-1][1] == (A['q'], A['gq'], A['sse'], A['kcur'], A['kprop'], SIGMA, N_ROWS, C, CHAIN0, P, NMCMC, SEED, A['cur'],
                            A['gcur'], A['cur_lp'], A['best'], A['best_lp'], A['chain'], A['lps'], A['alphas'], A['nacc'],
                            A['step'], 1) + accept_extra + (STREAM,)
