"""GPU: the int8-slice forward (csrc/qn_i8_slice.h, qn_fused_i8.hip: k_fused_fwd_i8 in its 8-wave and 4-wave forms;
qn_wide_i8.hip: k_i8_wide_fwd, k_i8_wide_fwd_u) pinned to the exact integer model of tests/test_i8_slice_ref_cpu.py.

Observation: networks with exactly two hidden layers have ONE sliced product, and the second hidden layer is consumed as
float64.  The output layer is one-hot with zero bias (a fused dot with zeros is exact in any order), so prediction k of a
chain IS one hidden unit; the chains of a batch cycle through all units.  Inputs are one-hot rows and b0 = 0, so the first
pre-activation of row n is column n mod d of W0 with no rounding.

Bars (none of them fitted to the device's output):
  relu / identity: the model reproduces the pre-activation bit for bit where every step is exact; where the kept sum does not
    fit 53 bits the model performs the code's roundings in the code's order and COUNTS them: the pair recombination of
    k_fused_fwd_i8's epilogue stages 1-3 (three fma's with 65536, the first exact below 2^53), the level-by-level `st < NLEV`
    micro-steps of k_i8_wide_fwd / k_i8_wide_fwd_u (six fma's with 256), and the fma with {scale, bias} (stage 3; `st == NLEV`)
    -- at most 3 + 1 and 6 + 1.  The bar is (roundings that were inexact) x 2^-53 x sum|terms|; 0 where there were none.
  tanh: the first layer is fed atanh(m 2^-46) for chosen integers m, so the device's rint lands on m (margin asserted on the
    CPU); pred is held to tanh_ref(z_model) within 2^-51 (the device tanh: test_tanh_tab512_cpu.py, and the header of
    qn_tanh_f64_tab64 in qn_math.h) plus the
    counted roundings of z through sech^2 <= 1 plus half an ulp of the reference's own rounding: ~5e-16.
Every test prints its largest distance from the model in units of its bar (run with -s; the record is
profiles/i8_slice_pin.txt)."""
import numpy as np
import pytest

from quinn_amd import _lib
from quinn_amd.ops import BatchedMLP, MLPArch
from test_i8_slice_ref_cpu import (CASE_NAMES, cases, chain_reference, deep_case, guard_case, hidden_model, sse_case, tanh_hp,
                                   true_model)

pytestmark = pytest.mark.gpu


def _ratio(diff, bar):
    """Largest diff / bar; a difference where the bar is 0 (bit-for-bit) counts as infinite."""
    diff, bar = np.asarray(diff, dtype=np.float64), np.broadcast_to(np.asarray(bar, dtype=np.float64), np.shape(diff))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, np.where(bar > 0, diff / bar, np.inf))
    return float(r.max())


def _sse_bound_check(sse, pred, Y):
    """The SSE against the left-to-right float64 sum of the device's own squared residuals: any summation order of n terms
    stays within n x 2^-53 x the sum (all terms >= 0), plus one rounding per square and per residual."""
    worst = 0.0
    for b in range(pred.shape[0]):
        res = pred[b] - Y[b]
        s = 0.0
        for v in (res * res).ravel():
            s += v
        n = res.size + 2
        assert abs(sse[b] - s) <= n * 2.0 ** -53 * s, (b, sse[b], s)
        worst = max(worst, abs(sse[b] - s) / (n * 2.0 ** -53 * s) if s > 0 else 0.0)
    return worst


@pytest.mark.parametrize("name", CASE_NAMES)
def test_forward_equals_the_integer_model(name):
    c = cases()[name]
    model, _ = true_model(name)
    rs = np.random.RandomState(3)
    Y = rs.randint(-64, 65, size=(c.N, c.o)) / 32.0
    op = BatchedMLP(MLPArch(c.dims, c.act), c.X, Y)
    Nb = c.N if c.row_idx is None else c.row_idx.shape[1]
    assert op.arith(c.B, Nb, False) == (_lib.ARITH_I8_WIDE if c.wide else _lib.ARITH_I8_FUSED)
    sse, pred = (t.cpu().numpy() for t in op.sse_pred(c.W, row_idx=c.row_idx))
    worst, exact, total = 0.0, 0, 0
    Yb = []
    for b in range(c.B):
        rows = np.arange(c.N) if c.row_idx is None else c.row_idx[b]
        z, nr, mag = model[b]
        want = c.expected(z)[rows % c.d]                                   # [Nb, o]
        bar = c.bar(z, nr, mag)[rows % c.d]
        diff = np.abs(pred[b] - want)
        worst = max(worst, _ratio(diff, bar))
        exact += int(np.sum(nr[rows % c.d] == 0)); total += diff.size
        assert np.all(diff <= bar), (name, b, float(diff.max()), np.argwhere(diff > bar)[:4].tolist())
        Yb.append(Y[rows])
    w_sse = _sse_bound_check(sse, pred, np.stack(Yb))
    print(f"i8_slice_pin {name}: B={c.B} max |pred - model| / bar = {worst:.3g} ({exact}/{total} predictions with no rounding: bit for bit); "
          f"SSE / bound = {w_sse:.3g}")


@pytest.mark.parametrize("act", ["tanh", "identity"])
def test_sse_of_exact_residuals_is_bit_exact(act):
    """Residuals are small dyadic numbers (test_sse_case_is_exact_in_any_order): the chain's SSE is the left-to-right float64 sum
    of the squared model residuals bit for bit, through the lane / wave / split order of the kernel, qn_sse_finish's
    left-to-right sum over the splits, and sse_parts (whose left-to-right sum is the SSE)."""
    dims, X, Y, W, P = sse_case(act)
    op = BatchedMLP(MLPArch(dims, act), X, Y)
    assert op.arith(W.shape[0], X.shape[0], False) == _lib.ARITH_I8_FUSED
    sse, pred = (t.cpu().numpy() for t in op.sse_pred(W))
    assert np.array_equal(pred, P)
    want = np.zeros(W.shape[0])
    for b in range(W.shape[0]):
        s = 0.0
        for v in ((P[b] - Y) ** 2).ravel():
            s += v
        want[b] = s
    assert np.array_equal(sse, want)
    parts = op.sse_parts(W).cpu().numpy()
    acc = np.zeros(W.shape[0])
    for k in range(parts.shape[1]):
        acc = acc + parts[:, k]
    assert np.array_equal(acc, want)
    print(f"i8_slice_pin sse_{act}: SSE and the sum of {parts.shape[1]} parts equal the exact sum, distance 0")


def test_tiny_activation_guard_selects_the_path_per_16_rows():
    """tanh, 8-wave form, d = 5 (DP = 8), o = 4.  Groups (16 rows = one wave's rows) whose activations are all below 2^-5 are
    redone in plain float64 (slow_tile in qn_fused_i8.hip): z = bias, then 64 fma's; activations and result through
    qn_tanh_f64 (< 3 ulp: the header of qn_math.h).  Counted bound on z: 64 fma roundings + 3 ulp on each activation (through its weight:
    6 x 2^-53 |w a|) -> (64 + 6) x 2^-53 x sum|terms|, and 3 ulp <= 2^-51 on the result (|pred| < 0.5); the reference is the
    same chain in long double.  The other groups are held to the integer model with the tanh bar of this file.  The two
    models differ by more than both bars on the tiny groups (test_guard_case_paths_differ_by_more_than_the_bars), so a tiny
    group on the integer path fails here; the all-zero group gives tanh(bias) on either path."""
    dims, X, W, z1, ms, chains = guard_case()
    op = BatchedMLP(MLPArch(dims, "tanh"), X, np.zeros((X.shape[0], dims[-1])))
    assert op.arith(W.shape[0], X.shape[0], False) == _lib.ARITH_I8_FUSED
    _, pred = (t.cpu().numpy() for t in op.sse_pred(W))
    w_chain = w_int = 0.0
    for b, c in enumerate(chains):
        u = c["units"]
        for g in range(5):
            got = pred[b, 16 * g:16 * g + 16]                              # [16, o]
            assert np.all(got == got[0])
            if g in (0, 2, 4):
                a1 = np.array([float(tanh_hp(v)) for v in z1[g]])
                zc, mag = chain_reference(c["M"][u], c["b1"][u], a1)
                want = np.tanh(zc).astype(np.float64)
                bar = 70 * 2.0 ** -53 * mag + 2.0 ** -51 + 2.0 ** -54
                w_chain = max(w_chain, _ratio(np.abs(got[0] - want), bar))
                assert np.all(np.abs(got[0] - want) <= bar), (b, g)
            else:
                z, nr, mag, _ = hidden_model(c["M"][u], c["b1"][u], None, False, m_a=np.array([ms[g]], dtype=np.int64))
                want = np.array([float(tanh_hp(v)) for v in z[0]])
                bar = 2.0 ** -51 + nr[0] * 2.0 ** -53 * mag[0] + 2.0 ** -54
                w_int = max(w_int, _ratio(np.abs(got[0] - want), bar))
                assert np.all(np.abs(got[0] - want) <= bar), (b, g)
    print(f"i8_slice_pin guard: tiny groups vs float64 chain {w_chain:.3g} of the bar, other groups vs integer model {w_int:.3g}")


@pytest.mark.parametrize("name", ["tanh_d2_o4", "identity_d7_o3", "relu_d1_o1"])
def test_weight_of_2_pow_20_leaves_the_fast_path(name):
    """A sliced matrix with an entry of 2^20 is outside the contract (I8_MAX_WEIGHT_EXP): that chain runs in plain float64 and
    agrees with the layer-wise float64 kernels (PATH_GENERIC) on the non-finite pattern, values within two float64 chains'
    (64 + 1) x 2^-53 x sum|terms| each (tanh: through sech^2 <= 1, plus 3 ulp of each tanh on both sides: 8 x 2^-53 of
    |pred| <= 1 and 6 x 2^-53 sum|terms| for the activations); the other chains of the launch stay on the integer model."""
    c = cases()[name]
    model, _ = true_model(name)
    W = c.W.copy()
    h, d = c.h, c.d
    bad = 2
    j = c.units[bad][0]
    off = h * d + h + j * h + 9
    W[bad, off] = 2.0 ** 20
    op = BatchedMLP(MLPArch(c.dims, c.act), c.X, np.zeros((c.N, c.o)))
    assert op.arith(c.B, c.N, False) == _lib.ARITH_I8_FUSED
    res = {}
    for path in (_lib.PATH_AUTO, _lib.PATH_GENERIC):
        old = op.set_path(path)
        try:
            res[path] = tuple(t.cpu().numpy() for t in op.sse_pred(W))
        finally:
            op.set_path(old)
    (s8, p8), (sg, pg) = res[_lib.PATH_AUTO], res[_lib.PATH_GENERIC]
    assert np.array_equal(np.isfinite(p8), np.isfinite(pg)) and np.array_equal(np.isfinite(s8), np.isfinite(sg))
    # sum|terms| of the observed units of the bad chain from the exact first-layer outputs
    ch = c.chains[bad]
    M = ch["M"].copy(); M[j, 9] = 2.0 ** 20
    rows = np.array(ch["rows"].copy() if c.act != "tanh" else [[float(tanh_hp(c.W[bad, i * d + r])) for i in range(h)] for r in range(d)], dtype=np.float64)
    if c.act == "relu":
        rows = np.maximum(rows, 0.0)
    u = c.units[bad]
    mag = np.abs(ch["b1"][u])[None, :] + np.abs(rows) @ np.abs(M[u]).T      # [d, o]
    bar = (2 * 65 + (12 if c.act == "tanh" else 0)) * 2.0 ** -53 * mag + (16 * 2.0 ** -53 if c.act == "tanh" else 0.0)
    diff = np.abs(p8[bad] - pg[bad])
    w = _ratio(diff, bar[np.arange(c.N) % d])
    assert np.all(diff <= bar[np.arange(c.N) % d]), (name, float(diff.max()))
    worst = 0.0
    for b in range(c.B):
        if b == bad:
            continue
        z, nr, mag_b = model[b]
        r = np.arange(c.N) % d
        df = np.abs(p8[b] - c.expected(z)[r])
        assert np.all(df <= c.bar(z, nr, mag_b)[r]), (name, b)
        worst = max(worst, _ratio(df, c.bar(z, nr, mag_b)[r]))
    print(f"i8_slice_pin big_weight {name}: flagged chain vs layer-wise float64 {w:.3g} of the bar; other chains vs model {worst:.3g}")


def test_four_hidden_layers_pin_the_last_sliced_product():
    """tanh, four hidden layers: the 4-wave tanh form (tanh(n / 64) table, 20-stage epilogue, slice4 inside the epilogue feeding
    the next sliced layer), three sliced products.  deep_case() puts nothing but +-1 and 0 into layers 1..3, where the device
    saturates exactly (|z| >= 24 is clamped to the table's last node tanh(20) = 1.0 with b = 0; z = 0 gives 0), so z2 and z3 are
    exact and the last sliced product is known to the integer model: pred is held to tanh_ref(z_model) with the tanh bar of
    this file.  What it pins: the path epilogue -> digits -> next product of the 4-wave tanh form (a wrong sign, a lost zero or a
    wrong top digit of +-2^46 in a later layer moves z4 by a whole weight), and the weight digits of the last matrix against
    the top activation digit +-64."""
    dims, X, W, chains = deep_case()
    op = BatchedMLP(MLPArch(dims, "tanh"), X, np.zeros((X.shape[0], dims[-1])))
    assert op.arith(W.shape[0], X.shape[0], False) == _lib.ARITH_I8_FUSED
    _, pred = (t.cpu().numpy() for t in op.sse_pred(W))
    worst = 0.0
    r = np.arange(X.shape[0]) % dims[0]
    for b, c in enumerate(chains):
        want = np.array([[float(tanh_hp(v)) for v in row] for row in c["z"]])[r]
        bar = (2.0 ** -51 + c["nr"] * 2.0 ** -53 * c["mag"] + 2.0 ** -54)[r]
        diff = np.abs(pred[b] - want)
        worst = max(worst, _ratio(diff, bar))
        assert np.all(diff <= bar), (b, float(diff.max()))
    print(f"i8_slice_pin deep_tanh_4x64: B={len(chains)} max |pred - model| / bar = {worst:.3g}")
