"""CPU: an exact integer model of the int8-slice forward's digit arithmetic (csrc/qn_i8_slice.h, qn_fused_i8.hip,
qn_wide_i8.hip), read off the kernels, in numpy int64 and Python integers -- and the input cases of
tests/test_gpu_i8_slice_pin.py, which holds the kernels to this model.

The scheme is an error-free product: both operands are rounded to integers (m_a = rint(a 2^(46 - f)), m_w = rint(w 2^(46 - e))),
cut into six balanced base-256 digits, every digit product of level p + q >= LMIN = 4 is an exact int8 x int8 -> int32 MFMA, the
level sums are recombined in float64 in a fixed order and one fma applies {scale, bias}.  Every step is either exact integer
arithmetic or ONE correctly rounded float64 operation on integers, so Python integers and `float(int)` (round-half-even)
reproduce a hidden pre-activation bit for bit, roundings of the recombination included.

Checked here, without a device: the digits reconstruct m at every edge value; the 36 products sum to m_w m_a; the dropped
levels stay below the 2^-51 of the row scale per term that the kernel header claims; every int32 accumulator (and every int32
pair sum of the epilogue) of every GPU case fits; and the GPU cases can tell a wrong kernel from a right one: six plausible
mistakes (LMIN = 5, truncation, a lost carry out of digit 0, a flipped top digit, a row exponent off by one at a power of two,
ties away from zero) each move the model by more than 100 times the bar of the GPU test on at least one case."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

H, NS, QB, LMIN = 64, 6, 46, 4
BIAS5 = 0x8080808080                       # the five low bytes of kMagic (kMagic in qn_i8_slice.h)
MAX_WEIGHT_EXP = 20                        # I8_MAX_WEIGHT_EXP
TWO46 = 1 << QB


# ---------------------------------------------------------------------------------------------- extended-precision tanh
def _frac_of_mpf(v):
    s, m, e, _ = v._mpf_
    return Fraction(-int(m) if s else int(m)) * Fraction(2) ** int(e)


def tanh_hp(x):
    """tanh of a double / Fraction as a Fraction, far beyond float64 (mpmath at 220 bits if it imports, else decimal at 70 digits)."""
    x = Fraction(x)
    try:
        import mpmath
        with mpmath.workprec(220):
            return _frac_of_mpf(mpmath.tanh(mpmath.mpf(x.numerator) / mpmath.mpf(x.denominator)))
    except ImportError:
        from decimal import Decimal, localcontext
        with localcontext() as c:
            c.prec = 70
            d = Decimal(x.numerator) / Decimal(x.denominator)
            e = (-2 * abs(d)).exp()
            r = (1 - e) / (1 + e)
            return Fraction(-r if d < 0 else r)


def atanh_double(a):
    """atanh of a Fraction |a| < 1, rounded to the nearest double."""
    a = Fraction(a)
    try:
        import mpmath
        with mpmath.workprec(220):
            return float(mpmath.atanh(mpmath.mpf(a.numerator) / mpmath.mpf(a.denominator)))
    except ImportError:
        from decimal import Decimal, localcontext
        with localcontext() as c:
            c.prec = 70
            d = Decimal(a.numerator) / Decimal(a.denominator)
            return float(((1 + d) / (1 - d)).ln() / 2)


# ---------------------------------------------------------------------------------------------- the model
def _round(v, mode):
    """An exactly scaled float64 array -> integers.  'rint': round-half-even, what the fma with kMagic does (the constant is an
    even integer with an ulp of 1); the other modes are the mistakes the cases must expose."""
    v = np.asarray(v, dtype=np.float64)
    if mode == "rint":
        r = np.rint(v)
    elif mode == "trunc":
        r = np.trunc(v)
    elif mode == "away":
        r = np.sign(v) * np.floor(np.abs(v) + 0.5)
    else:
        raise ValueError(mode)
    return r.astype(np.int64)


def row_exponent(row):
    """e of k_i8_slice_w / stage(): the largest biased exponent field E of the row gives |w| < 2^(E - 1022); clamped at -900."""
    bits = np.abs(np.asarray(row, dtype=np.float64)).view(np.uint64)
    e = int((bits >> np.uint64(52)).max()) - 1022
    return max(e, -900)


def slice_w(Wrow, mode="rint", e_bump_pow2=0):
    """(e, m_w) of one weight row; `e_bump_pow2`: the off-by-one mistake at a row whose largest |w| is a power of two."""
    Wrow = np.asarray(Wrow, dtype=np.float64)
    e = row_exponent(Wrow)
    mx = np.abs(Wrow).max()
    if e_bump_pow2 and mx > 0 and math.frexp(mx)[0] == 0.5:
        e += e_bump_pow2
    return e, _round(np.ldexp(Wrow, QB - e), mode)


def slice_a(a, mode="rint"):
    """m_a for the fixed scale 2^-46 (tanh activations)."""
    return _round(np.ldexp(np.asarray(a, dtype=np.float64), QB), mode)


def slice_a_rows(a, mode="rint"):
    """(f_n, m_a) with one scale per data row (relu / identity; slice_rows of k_fused_fwd_i8 and k_i8_wide_fwd_u): E = exponent
    field of the row's largest |a|, at least 122; f = E - 1022, so 2^f > every |a| of the row; m_a = rint(a 2^(46 - f))."""
    a = np.asarray(a, dtype=np.float64)
    E = int(np.abs(a).view(np.uint64).max() >> np.uint64(52))
    E = max(E, 122)
    f = E - 1022
    return f, _round(np.ldexp(a, QB - f), mode)


def digits(m, mistake=None):
    """Six balanced digits [..., 6] of integers |m| <= 2^46: digits 0..4 = bytes of m + 0x8080808080 xor 0x80 as signed bytes
    (in [-128, 127]), the top digit = bits 40.. of that sum as they stand (two's complement, in [-64, 64])."""
    m = np.asarray(m, dtype=np.int64)
    t = m + BIAS5
    d = np.stack([((t >> (8 * k)) & 0xff) - 128 for k in range(5)] + [t >> 40], axis=-1)
    if mistake == "no_carry0":             # the carry of digit 0's +0x80 into byte 1 is lost
        d[..., 1] -= ((m & 0xff) >= 0x80).astype(np.int64)
    elif mistake == "top_xor":             # the top digit treated like the others
        x = (d[..., 5] & 0xff) ^ 0x80
        d[..., 5] = np.where(x >= 128, x - 256, x)
    elif mistake is not None:
        raise ValueError(mistake)
    return d


def level_sums(dw, da, lmin=LMIN):
    """dw [J, K, 6], da [R, K, 6] -> int64 [R, J, 11 - lmin]: the exact sum over K of the digit products of each kept level."""
    dw, da = np.asarray(dw, dtype=np.int64), np.asarray(da, dtype=np.int64)
    out = np.zeros((da.shape[0], dw.shape[0], 2 * (NS - 1) - lmin + 1), dtype=np.int64)
    for p in range(NS):
        for q in range(NS):
            if p + q >= lmin:
                out[:, :, p + q - lmin] += da[:, :, q] @ dw[:, :, p].T
    return out


def kept_sum(m_w, m_a, lmin=LMIN):
    """The exact integer sum_i sum_{p + q >= lmin} dw_p da_q 256^(p + q) of two integer vectors."""
    lv = level_sums(digits(m_w)[None], digits(m_a)[None], lmin)[0, 0]
    return sum(int(v) << (8 * (lmin + l)) for l, v in enumerate(lv))


def _fits_i32(v):
    return -(1 << 31) <= v < (1 << 31)


def recombine(levels, wide=False):
    """The epilogue's float64 recombination of the int32 level sums (lowest level first in `levels`), in units of 256^lmin.
    64-wide kernels (qn_fused_i8.hip, epilogue stages 0-3): levels in int32 pairs a[l] + (a[l + 1] << 8) from the top, an odd top level
    alone, ts = fma(ts, 65536, pair).  Wide kernels (qn_wide_i8.hip, the `st < NLEV` micro-steps of both epilogues): ts = fma(ts, 256, a[l]) level by level.
    Returns (ts as float, number of these fma's that rounded, exact integer, sum of |level terms| as an integer)."""
    lv = [int(v) for v in levels]
    assert all(_fits_i32(v) for v in lv)
    n = len(lv)
    nr = 0
    if wide:
        ts = float(lv[n - 1])
        for l in range(n - 2, -1, -1):
            ex = int(ts) * 256 + lv[l]
            ts2 = float(ex)
            nr += int(ts2) != ex
            ts = ts2
    else:
        top = n
        if n & 1:
            ts = float(lv[n - 1])
            top = n - 1
        else:
            pair = lv[n - 2] + (lv[n - 1] << 8)
            assert _fits_i32(pair)
            ts = float(pair)
            top = n - 2
        for l in range(top - 2, -1, -2):
            pair = lv[l] + (lv[l + 1] << 8)
            assert _fits_i32(pair)
            ex = int(ts) * 65536 + pair
            ts2 = float(ex)
            nr += int(ts2) != ex
            ts = ts2
    exact = sum(v << (8 * l) for l, v in enumerate(lv))
    mag = sum(abs(v) << (8 * l) for l, v in enumerate(lv))
    return ts, nr, exact, mag


def z_model(levels, e, bias, f=0, lmin=LMIN, wide=False):
    """Pre-activation of one (row, feature): fma(ts 2^f, 2^(e - 92 + 8 lmin), bias) (stage 3 of the epilogue in qn_fused_i8.hip, `st == NLEV` in qn_wide_i8.hip; the products with
    powers of two are exact).  Returns (z, roundings: those of the recombination + 1 if the final fma rounded, sum of |terms|
    as a float: |bias| + the scaled |level sums|)."""
    ts, nr, _, mag = recombine(levels, wide)
    sc = Fraction(2) ** (e - 2 * QB + 8 * lmin + f)
    ex = Fraction(int(ts)) * sc + Fraction(float(bias))
    z = float(ex)
    nr += Fraction(z) != ex
    return z, nr, float(Fraction(mag) * sc + abs(Fraction(float(bias))))


VARIANTS = {                                # name -> keyword overrides of hidden_model: the mistakes of the issue
    "lmin5": dict(lmin=5),
    "trunc": dict(mode="trunc"),
    "no_carry0": dict(mistake="no_carry0"),
    "top_xor": dict(mistake="top_xor"),
    "e_off_by_one": dict(e_bump=1),
    "ties_away": dict(mode="away"),
}


def hidden_model(Wm, bias, A, per_row, wide=False, lmin=LMIN, mode="rint", mistake=None, e_bump=0, m_a=None):
    """One sliced layer: Wm [J, K], bias [J], activations A [R, K] (float64, or for tanh the integers `m_a` [R, K] the device's
    rint lands on).  Returns z [R, J], roundings [R, J], sum|terms| [R, J], and the largest |int32 accumulator|."""
    J, K = Wm.shape
    es, mw = zip(*[slice_w(Wm[j], mode, e_bump) for j in range(J)])
    dw = digits(np.stack(mw), mistake)
    if m_a is not None:
        fs, ma = [0] * len(m_a), np.asarray(m_a, dtype=np.int64)
    elif per_row:
        fs, ma = zip(*[slice_a_rows(A[r], mode) for r in range(A.shape[0])])
        ma = np.stack(ma)
    else:
        fs, ma = [0] * A.shape[0], slice_a(A, mode)
    da = digits(ma, mistake)
    lv = level_sums(dw, da, lmin)
    R = da.shape[0]
    z, nr, mag = np.zeros((R, J)), np.zeros((R, J), dtype=np.int64), np.zeros((R, J))
    for r in range(R):
        for j in range(J):
            z[r, j], nr[r, j], mag[r, j] = z_model(lv[r, j], es[j], bias[j], fs[r], lmin, wide)
    return z, nr, mag, int(np.abs(lv).max())


# ---------------------------------------------------------------------------------------------- the cases of the GPU pin
def from_digits(ds):
    return sum(int(d) << (8 * k) for k, d in enumerate(ds))


# digit patterns (low five digits, top digit): all +127, all -128, alternating, 0x80 in each byte position, one unit in digit 0
PATTERNS = [from_digits([127] * 5 + [63]), from_digits([-128] * 5 + [-63]), from_digits([127, -128, 127, -128, 127, 40]),
            from_digits([-128, 127, -128, 127, -128, -40]), 1, -1, TWO46 - 1, -(TWO46 - 1), 0,
            from_digits([127] * 5 + [0]), from_digits([-128] * 5 + [0])] + \
           [(0x80 << (8 * k)) + (s << 40) for k in range(5) for s in (33, -35)] + [-(0x80 << (8 * k)) for k in range(5)]


def pack(mats, biases):
    return np.concatenate([np.concatenate([np.asarray(M, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64)])
                           for M, b in zip(mats, biases)])


@functools.lru_cache(maxsize=None)
def _weight_matrix(h, variant, wexp):
    """An h x h hidden matrix of pattern integers m 2^(e_j - 46) whose rows cover the digit patterns, the coherent-sign case, the
    rint ties and the row-exponent edges; `wexp`: the common exponent of the ordinary rows (tanh networks: -7, so |z| <= 0.5)."""
    rs = np.random.RandomState(1000 + variant)
    M = np.zeros((h, h))
    for j in range(h):
        e = wexp - (j % 3)
        kind = j % 16
        m = np.array([PATTERNS[(5 * j + 3 * i + variant) % len(PATTERNS)] for i in range(h)], dtype=object)
        if kind in (1, 9):                   # coherent: every low digit positive in all terms, a few large cancelling entries
            m = np.array([from_digits([127 - (i % 3), 120 + (i % 7), 127, 101 + (i % 20), 127, i % 2]) for i in range(h)], dtype=object)
            for i in range(0, h, 16):
                m[i] = from_digits([127, 127, 127, 127, 127, -5 - (i // 16 % 3)])
        elif kind == 2:                      # ties: (2k + 1) 2^-47 of the row scale, k even and odd
            m = np.array([Fraction(2 * (int(rs.randint(1 << 30)) * 4 + (i & 3)) + 1, 2) * (1 if i % 5 else -1) for i in range(h)], dtype=object)
        elif kind == 3:                      # random digits
            m = np.array([int(rs.randint(-(1 << 31), 1 << 31)) * (1 << 14) + int(rs.randint(1 << 14)) for _ in range(h)], dtype=object)
        row = np.array([float(Fraction(v) * Fraction(2) ** (e - QB)) for v in m])
        row[j % h] = math.ldexp(0.75 + 2.0 ** -30, e)                    # the anchor that fixes the row's exponent e
        if kind == 4: row *= 0.25; row[(j + 1) % h] = math.ldexp(1.0, e - 1); row[j % h] = math.ldexp(1.0, e - 9)      # largest |w| exactly 2^(e-1)
        if kind == 5: row[j % h] = -math.ldexp(1.0 - 2.0 ** -53, e)      # just below 2^e: m_w = -2^46, top digit -64
        if kind == 6: row[j % h] = math.ldexp(1.0 + 2.0 ** -52, e - 1)   # just above 2^(e-1)
        if kind == 7: row[:] = 0.0                                      # all-zero row: e = -900
        if kind == 8: row[:] = math.ldexp(1.0, e - 2) * np.where(np.arange(h) % 2, 1.0, -1.0) * (1 + 2.0 ** -44 * (np.arange(h) % 5))   # largest |w| a power of two, the others with their last kept bit set: e off by one loses it
        if kind == 8: row[j % h] = math.ldexp(1.0, e - 1)
        M[j] = row
    return M


def _big_rows(M):
    """Row 10: largest entry 2^20 - 2^-20 next to entries of 2^-20 (inside the contract)."""
    M = M.copy()
    h = M.shape[1]
    M[10] = 2.0 ** -20 * np.where(np.arange(h) % 3, 1.0, -1.0)
    M[10, 5] = 2.0 ** 20 - 2.0 ** -20
    return M


@functools.lru_cache(maxsize=None)
def _act_rows(act, d, h, variant):
    """The d distinct first-layer outputs [d][h]: for tanh integers m (a* = m 2^-46), else doubles (relu: negative ones are
    clipped by the device and by the model)."""
    rs = np.random.RandomState(2000 + variant)
    rows = []
    for r in range(d):
        kind = (r + variant) % 5
        m = [PATTERNS[(7 * r + 5 * i + variant) % len(PATTERNS)] for i in range(h)]
        if kind == 1:                        # coherent low digits, all positive
            m = [from_digits([127, 125 - (i % 5), 127, 127 - (i % 11), 119 + (i % 9), (i % 3)]) for i in range(h)]
            for i in range(3, h, 16):
                m[i] = from_digits([127, 127, 127, 127, 127, 9 + (i // 16)])
        if kind == 2:
            m = [int(rs.randint(-(1 << 31), 1 << 31)) * (1 << 14) + int(rs.randint(1 << 14)) for _ in range(h)]
        if act == "tanh":
            if kind == 3:                    # saturation (top digit +-64) and exact zeros, MIXED into rows of ordinary values (not
                                             # cases of their own; deep_case has layers of nothing but +-1 / 0)
                m = [TWO46 if i % 4 == 0 else -TWO46 if i % 4 == 1 else 0 if i % 4 == 2 else m[i] for i in range(h)]
            rows.append([int(v) for v in m])
        else:
            f = (3, 0, -5, 11, -2)[kind]
            a = np.array([float(Fraction(v) * Fraction(2) ** (f - QB)) for v in m])
            if kind in (0, 4):               # ties in the activations: (2k + 1) 2^(f - 47), k even and odd
                for i in range(0, h, 3):
                    a[i] = float(Fraction(2 * (int(rs.randint(1 << 30)) * 4 + (i & 3)) + 1, 2) * Fraction(2) ** (f - QB)) * (-1 if i % 2 else 1)
            a[(11 * r + 1) % h] = math.ldexp(1.0, f - 1) if kind == 3 else math.ldexp(0.8125, f)      # the row maximum: 2^(f-1) exactly / inside
            rows.append(a)
    return rows


@functools.lru_cache(maxsize=None)
def tanh_input(m):
    """x* with tanh(x*) 2^46 within 1/2 - 2^-4 of m (asserted): the device tanh (absolute error < 2^-51 = 2^-5 grid steps) then
    rounds to m whatever its last bits are.  m = +-2^46: x* = +-20, where the device returns exactly +-1 (the clamp at 20 meets
    the last node of either table, tanh(20) = 1.0 to the last bit, and b = 0: qn_tanh_f64_tab512, qn_tanh_f64_tab64); m = 0: x* = 0 -> 0."""
    if m == 0: return 0.0
    if abs(m) == TWO46: return math.copysign(20.0, m)
    x = atanh_double(Fraction(m, TWO46))
    assert abs(tanh_hp(x) * TWO46 - m) < Fraction(1, 2) - Fraction(1, 16), m
    return x


class Case:
    """A two-hidden-layer network whose first pre-activations are exact by construction and whose output layer is one-hot:
    prediction k of chain b IS hidden unit units[b][k] of the second hidden layer."""

    def __init__(self, name, act, d, h, o, variant=0, N=80, use_idx=False, wide=False):
        self.name, self.act, self.d, self.h, self.o, self.N, self.wide = name, act, d, h, o, N, wide
        self.dims = (d, h, h, o)
        self.hp = -(-h // 64) * 64 if h < 64 or h % 64 else h              # the padded twin's width
        self.B = -(-h // o)
        tanh = act == "tanh"
        self.X = np.zeros((N, d))
        self.X[np.arange(N), np.arange(N) % d] = 1.0                      # one-hot rows: z1[n] = W0[:, n mod d] exactly (b0 = 0)
        rsx = np.random.RandomState(7)
        self.row_idx = rsx.randint(0, N, size=(self.B, N - 13)).astype(np.int32) if use_idx else None
        self.units = [[(b * o + k) % h for k in range(o)] for b in range(self.B)]
        self.chains = []
        Ws = []
        for b in range(self.B):
            v = variant + b % 4
            M = _weight_matrix(h, v, -8 - max(0, h.bit_length() - 7) if tanh else 2)
            if b % 4 == 1: M = _big_rows(M)
            rs = np.random.RandomState(b)
            b1 = np.ldexp(rs.randint(-(1 << 20), 1 << 20, size=h).astype(np.float64), -23 if tanh else -10)
            rows = _act_rows(act, d, h, v)
            if tanh and d == 1:
                if b % 2:                                                  # (odd chains observe the coherent weight rows 1, 9, 17, ...)
                    rows = _act_rows(act, d, h, 1 + 5 * (b % 4))           # kind 1: coherent activations
                # one row type: the coherent rows can have row exponent 0 with z made small by the BIAS -- dropping level 4
                # then costs ~2^-38 against a bar of ~2^-47 (this is the tanh case that tells LMIN 4 from 5)
                M = M.copy()
                for j in range(h):
                    if j % 16 in (1, 9):
                        M[j] = np.ldexp(M[j], 8 + j % 3)
                        s = sum(Fraction(float(w)) * Fraction(int(m), TWO46) for w, m in zip(M[j], rows[0]))
                        b1[j] = -float(Fraction(round(s * (1 << 23)), 1 << 23))
            W0 = np.zeros((h, d))
            for r in range(d):
                W0[:, r] = [tanh_input(m) for m in rows[r]] if tanh else rows[r]
            Wl = np.zeros((o, h))
            for k in range(o):
                Wl[k, self.units[b][k]] = 1.0
            self.chains.append(dict(M=M, b1=b1, rows=rows))
            Ws.append(pack([W0, M, Wl], [np.zeros(h), b1, np.zeros(o)]))
        self.W = np.stack(Ws)

    def _padded(self, c):
        """The operands as the kernel sees them: a 50-wide network runs as its 64-wide zero-padded twin (exact zeros)."""
        h, hp = self.h, self.hp
        M = np.zeros((hp, hp)); M[:h, :h] = c["M"]
        b1 = np.zeros(hp); b1[:h] = c["b1"]
        rows = np.zeros((self.d, hp), dtype=object if self.act == "tanh" else np.float64)
        for r in range(self.d):
            rows[r, :h] = c["rows"][r]
        return M, b1, rows

    def model(self, **variant):
        """z2 [B][d, o], roundings, sum|terms| of the observed units for the d distinct rows, and the largest |accumulator|."""
        out, amax = [], 0
        for b, c in enumerate(self.chains):
            M, b1, rows = self._padded(c)
            u = self.units[b]
            if self.act == "tanh":
                z, nr, mag, am = hidden_model(M[u], b1[u], None, False, self.wide, m_a=np.array(rows.tolist(), dtype=np.int64), **variant)
            else:
                A = rows.astype(np.float64)
                if self.act == "relu":
                    A = np.maximum(A, 0.0)
                z, nr, mag, am = hidden_model(M[u], b1[u], A, True, self.wide, **variant)
            out.append((z, nr, mag))
            amax = max(amax, am)
        return out, amax

    def bar(self, z, nr, mag):
        """The GPU test's bar on a prediction, from the counted roundings (see test_gpu_i8_slice_pin.py)."""
        rnd = nr * 2.0 ** -53 * mag
        if self.act == "tanh":                                           # (sech^2 at the near end of [z - rnd, z + rnd]: mean value theorem)
            return 2.0 ** -51 + rnd * (1.0 - np.tanh(np.maximum(np.abs(z) - rnd, 0.0)) ** 2) * (1 + 2.0 ** -40) + 2.0 ** -54
        return rnd

    def expected(self, z):
        if self.act == "tanh":
            return np.array([[float(tanh_hp(v)) for v in row] for row in z])
        return np.maximum(z, 0.0) if self.act == "relu" else z


def _cases():
    cs = []
    for d, o in ((1, 1), (2, 4), (3, 1), (5, 4)):                         # the 8-wave form: DP = 1, 2, 4, 8
        cs.append(Case(f"tanh_d{d}_o{o}", "tanh", d, 64, o, variant=d, use_idx=(d == 3)))
    for act in ("relu", "identity"):                                     # the 4-wave form
        for d, o in ((1, 1), (7, 3)):
            cs.append(Case(f"{act}_d{d}_o{o}", act, d, 64, o, variant=d + o, use_idx=(d == 7 and act == "relu")))
    cs.append(Case("tanh_padded50", "tanh", 2, 50, 1, variant=2))
    cs.append(Case("identity_padded50", "identity", 3, 50, 1, variant=1))
    for h in (128, 256):                                                 # k_i8_wide_fwd / k_i8_wide_fwd_u: o = 1
        cs.append(Case(f"wide_tanh_{h}", "tanh", 2, h, 1, variant=h // 128, wide=True))
        cs.append(Case(f"wide_identity_{h}", "identity", 2, h, 1, variant=3, wide=True))
    return cs


@functools.lru_cache(maxsize=None)
def cases():
    return {c.name: c for c in _cases()}


CASE_NAMES = ["tanh_d1_o1", "tanh_d2_o4", "tanh_d3_o1", "tanh_d5_o4", "relu_d1_o1", "relu_d7_o3", "identity_d1_o1", "identity_d7_o3",
              "tanh_padded50", "identity_padded50", "wide_tanh_128", "wide_identity_128", "wide_tanh_256", "wide_identity_256"]


@functools.lru_cache(maxsize=None)
def true_model(name):
    return cases()[name].model()


# ---------------------------------------------------------------------------------------------- the CPU assertions
EDGES = [0, 1, -1, TWO46, -TWO46, TWO46 - 1, -(TWO46 - 1), from_digits([127] * 5 + [63]), from_digits([-128] * 5 + [-63]),
         from_digits([127] * 5 + [-64]), from_digits([-128] * 5 + [63])] + [s * (0x80 << (8 * k)) for k in range(5) for s in (1, -1)] + \
        [0x7f, 0x80, 0x81, -0x7f, -0x80, -0x81, 0x8080808080, -0x8080808080, 0x7f7f7f7f7f]


def test_digits_reconstruct_every_edge_value():
    rs = np.random.RandomState(0)
    ms = np.array(EDGES + [int(v) for v in rs.randint(-TWO46, TWO46 + 1, size=5000, dtype=np.int64)], dtype=np.int64)
    d = digits(ms)
    assert d[:, :5].min() >= -128 and d[:, :5].max() <= 127 and d[:, 5].min() >= -64 and d[:, 5].max() <= 64
    for m, dd in zip(ms, d):
        assert from_digits(dd) == int(m)
    assert list(digits(TWO46)) == [0, 0, 0, 0, 0, 64] and list(digits(-TWO46)) == [0, 0, 0, 0, 0, -64]
    assert list(digits(0x80)) == [-128, 1, 0, 0, 0, 0]                   # a byte of exactly 0x80 carries into the next digit
    assert list(digits(0x80 << 32)) == [0, 0, 0, 0, -128, 1]
    assert -128 in d[:, :5] and 127 in d[:, :5]


def test_all_36_products_give_the_exact_product():
    rs = np.random.RandomState(1)
    for _ in range(50):
        mw = rs.randint(-TWO46, TWO46 + 1, size=64, dtype=np.int64)
        ma = rs.randint(-TWO46, TWO46 + 1, size=64, dtype=np.int64)
        mw[:len(EDGES)] = EDGES
        ma[:20] = rs.permutation(EDGES)[:20]
        assert kept_sum(mw, ma, lmin=0) == sum(int(a) * int(b) for a, b in zip(mw, ma))


def test_dropped_levels_are_below_2_pow_minus_51_per_term():
    """Levels 0..3 of one term: at most sum_{L < 4} (L + 1) 128^2 256^L < 2^40.01 in units of 2^-92 of the row scale, i.e.
    2^-51.99 -- the header's "< 2^-51 of the row scale".  Checked on the worst digits and on random operands."""
    worst = sum((L + 1) * 128 * 128 * 256 ** L for L in range(LMIN))
    assert Fraction(worst, 1 << 92) < Fraction(1, 1 << 51)
    rs = np.random.RandomState(2)
    mw = np.concatenate([[from_digits([-128] * 5 + [0])], rs.randint(-TWO46, TWO46 + 1, size=2000, dtype=np.int64)])
    ma = np.concatenate([[from_digits([-128] * 5 + [0])], rs.randint(-TWO46, TWO46 + 1, size=2000, dtype=np.int64)])
    for a, b in zip(mw, ma):
        dropped = int(a) * int(b) - kept_sum([a], [b])
        assert abs(dropped) <= worst
    assert int(mw[0]) * int(ma[0]) - kept_sum(mw[:1], ma[:1]) == worst   # the bound is attained: all digits -128


@pytest.mark.parametrize("name", CASE_NAMES)
def test_accumulators_of_the_gpu_cases_fit_int32(name):
    """Per accumulator at most 6 products x K x 2^14 (K = 64: < 2^23, the header's figure; K = 256: < 2^25); the int32 pair sums
    a[l] + (a[l + 1] << 8) of the 64-wide epilogue are asserted inside recombine()."""
    c = cases()[name]
    _, amax = true_model(name)
    assert amax < 6 * c.hp * (1 << 14) <= 1 << 25 and amax < 1 << 31
    print(f"{name}: largest |level accumulator| {amax} = 2^{math.log2(max(amax, 1)):.1f}")


def test_first_layer_is_exact_and_tanh_margins_hold():
    """The first pre-activation of every row is W0[:, n mod d] itself (one-hot x, b0 = 0); for tanh the margin of the device's
    rint is asserted inside tanh_input()."""
    for c in cases().values():
        assert np.array_equal(c.X.sum(axis=1), np.ones(c.N)) and set(np.unique(c.X)) <= {0.0, 1.0}
        assert c.W.shape == (c.B, sum(a * b + b for a, b in zip(c.dims[:-1], c.dims[1:])))
        if c.act == "tanh":                                             # |z2| <= 0.5 except the row with the 2^20 - 2^-20 entry
            for b, (z, _, _) in enumerate(true_model(c.name)[0]):
                for k, u in enumerate(c.units[b]):
                    assert np.abs(z[:, k]).max() <= 0.5 or (u == 10 and b % 4 == 1), (c.name, b, u)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_cases_tell_wrong_from_right(variant):
    """Each mistake moves the model's prediction by more than 100 bars of the GPU test on at least one (case, chain, row, unit)."""
    best, where = 0.0, None
    for name in CASE_NAMES:
        c = cases()[name]
        wrong, _ = c.model(**VARIANTS[variant])
        for b, ((z, nr, mag), (zw, _, _)) in enumerate(zip(true_model(name)[0], wrong)):
            diff = np.abs(c.expected(zw) - c.expected(z))
            bar = c.bar(z, nr, mag)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                ratio = np.where(diff > 0, diff / np.where(bar > 0, bar, 2.0 ** -1074), 0.0)
            if ratio.max() > best:
                best, where = float(ratio.max()), (name, b)
    print(f"{variant}: largest |wrong - right| / bar = {best:.3g} at {where}")
    assert best > 100.0, (variant, best, where)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_tanh_cases_tell_wrong_from_right_at_their_finite_bar(variant):
    """The same over the tanh cases only, whose bar is never 0 (>= 2^-51): the ratio is printed for every mistake and asserted
    for those a tanh case can show: the coherent rows of tanh_d1_o1 (row exponent 0, z cancelled by the bias) are what tells
    LMIN 4 from 5.  The activations of a tanh case sit ON the 2^-46 grid by construction and its weights are scaled to 2^-8 to
    keep |z| <= 0.5, so a rounding mistake in the weights (truncation, ties, a halved row) moves z by at most
    64 x 2^-47 x 2^-8 ~ 2^-49, about the 2^-51 bar itself: those three belong to the relu / identity cases, whose bar is 0."""
    best, where = 0.0, None
    for name in CASE_NAMES:
        c = cases()[name]
        if c.act != "tanh":
            continue
        wrong, _ = c.model(**VARIANTS[variant])
        for b, ((z, nr, mag), (zw, _, _)) in enumerate(zip(true_model(name)[0], wrong)):
            ratio = np.abs(c.expected(zw) - c.expected(z)) / c.bar(z, nr, mag)
            if ratio.max() > best:
                best, where = float(ratio.max()), (name, b)
    print(f"{variant} (tanh cases): largest |wrong - right| / bar = {best:.3g} at {where}")
    if variant in ("lmin5", "top_xor", "no_carry0"):
        assert best > 100.0, (variant, best, where)


# ---------------------------------------------------------------------------------------------- SSE and guard cases
def sse_case(act):
    """Small dyadic operands: every product, pre-activation, residual and squared residual is exact in float64, so the SSE of a
    chain is ONE number whatever the order of the sum (asserted below with Fractions).  identity: the 4-wave form, o = 3;
    tanh: the 8-wave form, o = 2, the second layer saturated (|z| >= 24: the device returns exactly +-1) or exactly 0."""
    rs = np.random.RandomState(5 if act == "tanh" else 6)
    d, o, N, B = (1, 2, 80, 5) if act == "tanh" else (2, 3, 80, 5)
    dims = (d, H, H, o)
    X = np.zeros((N, d)); X[np.arange(N), np.arange(N) % d] = 1.0
    Ws, P, Ys = [], [], []
    for b in range(B):
        M = rs.randint(-8, 9, size=(H, H)) / 16.0
        if act == "tanh":
            W0 = np.full((H, d), 20.0) * np.where(np.arange(H) % 2, 1.0, -1.0)[:, None]           # a1 = +-1 exactly
            b1 = np.where(np.arange(H) % 3 == 0, 0.0, np.where(np.arange(H) % 3 == 1, 64.0, -64.0))
            M[np.arange(H) % 3 == 0] = 0.0
            a1 = np.tanh(W0.T)                                             # (+-1: tanh(20) rounds to 1)
            assert set(np.unique(a1)) == {-1.0, 1.0}
            z2 = a1 @ M.T + b1
            assert np.all((z2 == 0) | (np.abs(z2) >= 24))
            a2 = np.sign(z2)
        else:
            W0 = rs.randint(-40, 41, size=(H, d)) / 8.0
            b1 = rs.randint(-64, 65, size=H) / 32.0
            a2 = W0.T @ M.T + b1                                           # exact: small dyadic numbers
        units = [(7 * b + 5 * k) % H for k in range(o)]
        Wl = np.zeros((o, H)); Wl[np.arange(o), units] = 1.0
        pred = a2[np.arange(N) % d][:, units]                              # [N, o]
        res = rs.randint(-128, 129, size=(N, o)) / 64.0
        Ws.append(pack([W0, M, Wl], [np.zeros(H), b1, np.zeros(o)]))
        P.append(pred); Ys.append(res)
    # one Y for all chains: chain b's residual is pred_b - Y; Y = pred_0 - res_0 keeps every chain's residual dyadic
    Y = P[0] - Ys[0]
    return dims, X, Y, np.stack(Ws), np.stack(P)


@pytest.mark.parametrize("act", ["tanh", "identity"])
def test_sse_case_is_exact_in_any_order(act):
    dims, X, Y, W, P = sse_case(act)
    for b in range(W.shape[0]):
        res = P[b] - Y
        assert all(Fraction(float(p)) - Fraction(float(y)) == Fraction(float(r)) for p, y, r in zip(P[b].ravel(), Y.ravel(), res.ravel()))
        sq = res * res
        assert all(Fraction(float(r)) ** 2 == Fraction(float(s)) for r, s in zip(res.ravel(), sq.ravel()))
        s = 0.0
        for v in sq.ravel():
            s += v
        assert Fraction(s) == sum(Fraction(float(v)) for v in sq.ravel())


def guard_case():
    """The tiny-activation guard of the tanh kernels (top_digits_large in qn_i8_slice.h): d = 5, x_n = e_(n // 16), so each of
    the five 16-row groups (= one wave's rows) has ONE activation vector.  Group 0 and 4: every |a| < 2^-5, not all zero (the
    wave's rows are redone in plain float64: slow_tile); group 1: tiny on-grid values and a single 2^-4 (top digit 4: the
    integer path); group 2: all zero (float64 chain, z = bias); group 3: ordinary on-grid values (integer path).
    Weights of ordinary size (row exponent 0), so the 2^-47 quantisation of the tiny rows would be visible."""
    rs = np.random.RandomState(11)
    d, o, N, B = 5, 4, 80, 16
    dims = (d, H, H, o)
    X = np.zeros((N, d)); X[np.arange(N), np.arange(N) // 16] = 1.0
    z1 = np.zeros((d, H))
    z1[0] = rs.uniform(-1, 1, H) * 2.0 ** -8
    z1[4] = -np.abs(rs.uniform(0.5, 1, H)) * 2.0 ** -7
    m1 = [int(v) for v in rs.randint(-(1 << 38), 1 << 38, size=H)]
    m1[17] = 1 << 42
    m3 = [PATTERNS[(3 * i) % len(PATTERNS)] for i in range(H)]
    z1[1] = [tanh_input(m) for m in m1]
    z1[3] = [tanh_input(m) for m in m3]
    ms = {1: m1, 3: m3}
    Ws, chains = [], []
    for b in range(B):
        M = rs.uniform(-1, 1, size=(H, H)) * np.where(rs.rand(H, H) < 0.3, 1.0, 2.0 ** -3)
        M[:, 17] *= 2.0 ** -3                                              # keeps |z2| <= 0.5 in group 1
        M *= 0.5
        b1 = rs.randint(-(1 << 20), 1 << 20, size=H) * 2.0 ** -23
        units = [(b * o + k) % H for k in range(o)]
        Wl = np.zeros((o, H)); Wl[np.arange(o), units] = 1.0
        Ws.append(pack([z1.T.copy(), M, Wl], [np.zeros(H), b1, np.zeros(o)]))
        chains.append(dict(M=M, b1=b1, units=units))
    return dims, X, np.stack(Ws), z1, ms, chains


def chain_reference(M, b1, a1):
    """The plain float64 chain of slow_tile in extended precision: (z, sum of |terms|) per unit."""
    Ml, al = M.astype(np.longdouble), a1.astype(np.longdouble)
    return b1.astype(np.longdouble) + Ml @ al, np.abs(b1) + np.abs(M) @ np.abs(a1)


def test_guard_case_paths_differ_by_more_than_the_bars():
    """On the tiny groups the integer model (activations rounded to 2^-46) and the float64 chain differ by more than the sum of
    both bars for most units: the GPU test can tell which path a tiny group took."""
    dims, X, W, z1, ms, chains = guard_case()
    told = 0
    for g in (0, 4):
        a1 = np.array([float(tanh_hp(v)) for v in z1[g]])
        assert 0 < np.abs(a1).max() < 2.0 ** -5
        for c in chains:
            u = c["units"]
            zc, mag = chain_reference(c["M"][u], c["b1"][u], a1)
            zi, nr, magi, _ = hidden_model(c["M"][u], c["b1"][u], a1[None], False)
            bar_c = 80 * 2.0 ** -53 * mag + 2.0 ** -51
            bar_i = 2.0 ** -51 + nr[0] * 2.0 ** -53 * magi[0] + 2.0 ** -54
            told += int(np.sum(np.abs(zi[0] - zc.astype(np.float64)) * 0.9 > bar_c + bar_i))     # (tanh' >= 0.9 for |z| <= 0.3)
            assert np.abs(zc).max() <= 0.3
    assert told > 0.5 * 2 * len(chains) * dims[-1], told
    for g in (1, 3):
        assert max(abs(m) for m in ms[g]) >= 1 << 42


# ---------------------------------------------------------------------------------------------- four hidden layers
def deep_case():
    """tanh, four hidden layers: the 4-wave form (its image with the tanh(n / 512) table no longer fits one CU), tanh(n / 64)
    table, three sliced products, slice4 inside the epilogue feeding the next sliced layer.  Intermediate activations of a tanh
    network are only known to 2^-51 -- except where the device saturates EXACTLY: |z| >= 20 is clamped to the last table node
    tanh(20) = 1.0 with b = 0 (qn_tanh_f64_tab64), and z = 0 gives 0.  Layers 1..3 therefore hold nothing but +-1 and 0:
    a1 = tanh(+-20); W1, W2 are small dyadic numbers with one entry of +-40 per row and bias 0, or all-zero rows, so z2, z3 are
    exact (every product with +-2^46 is an exact integer, no level is dropped) and either 0 or >= 24 in magnitude.  The LAST
    sliced product W3 a3 -- rich weight digits against the top activation digit +-64 -- is then pinned by the integer model.
    d = 2: the two row types differ in the sign of a1[0], which flips a2 and a3."""
    rs = np.random.RandomState(21)
    d, o, N, B = 2, 2, 80, 32
    dims = (d, H, H, H, H, o)
    X = np.zeros((N, d)); X[np.arange(N), np.arange(N) % d] = 1.0
    Ws, chains = [], []
    for b in range(B):
        W0 = 20.0 * np.where(rs.rand(H, d) < 0.5, 1.0, -1.0)
        W0[0] = [20.0, -20.0]
        a = np.sign(W0.T)                                                  # [d, H]: a1
        layers = []
        for col in (0, 1):                                                 # W1 keyed on a1[0], W2 on a2[1] (row 1 is never a zero row)
            M = rs.randint(-8, 9, size=(H, H)) / 16.0
            M[:, col] = 40.0 * np.where(rs.rand(H) < 0.5, 1.0, -1.0)
            M[np.arange(H) % 5 == 0] = 0.0
            z = a @ M.T                                                    # exact: |sum of 63 entries <= 1/2| < 32
            assert np.all((z == 0) | (np.abs(z) >= 24)) and np.abs(a[:, col]).min() == 1
            zi, nr, _, _ = hidden_model(M, np.zeros(H), None, False, m_a=(a * TWO46).astype(np.int64))
            assert np.array_equal(zi, z) and nr.max() == 0                 # the integer model agrees: no rounding anywhere
            a = np.sign(z)
            layers.append(M)
        assert len(np.unique(a, axis=0)) == 2 and set(np.unique(a)) == {-1.0, 0.0, 1.0}
        M3 = _weight_matrix(H, b % 4, -8)
        b3 = np.ldexp(rs.randint(-(1 << 20), 1 << 20, size=H).astype(np.float64), -23)
        units = [(b * o + k) % H for k in range(o)]
        Wl = np.zeros((o, H)); Wl[np.arange(o), units] = 1.0
        z4, nr, mag, amax = hidden_model(M3[units], b3[units], None, False, m_a=(a * TWO46).astype(np.int64))
        assert np.abs(z4).max() <= 0.5
        Ws.append(pack([W0, layers[0], layers[1], M3, Wl], [np.zeros(H), np.zeros(H), np.zeros(H), b3, np.zeros(o)]))
        chains.append(dict(z=z4, nr=nr, mag=mag, amax=amax))
    return dims, X, np.stack(Ws), chains


def test_every_other_gpu_case_fits_int32_too():
    """The accumulators (and, inside recombine(), the pair sums) of the cases outside CASE_NAMES: the deep case's last product,
    the guard case's integer groups, the SSE cases, and the matrix with the 2^20 entry of the big-weight test (that chain runs in
    float64 on the device; the model still must not overflow if it did not)."""
    worst = max(c["amax"] for c in deep_case()[3])
    dims, X, W, z1, ms, chains = guard_case()
    for c in chains:
        for g in (1, 3):
            worst = max(worst, hidden_model(c["M"], c["b1"], None, False, m_a=np.array([ms[g]], dtype=np.int64))[3])
    for act in ("tanh", "identity"):
        dims, X, Y, W, P = sse_case(act)
        d = dims[0]
        for b in range(W.shape[0]):
            W0 = W[b, :H * d].reshape(H, d)
            M = W[b, H * d + H:H * d + H + H * H].reshape(H, H)
            b1 = W[b, H * d + H + H * H:H * d + 2 * H + H * H]
            if act == "tanh":
                worst = max(worst, hidden_model(M, b1, None, False, m_a=(np.sign(W0.T) * TWO46).astype(np.int64))[3])
            else:
                worst = max(worst, hidden_model(M, b1, W0.T.copy(), True)[3])
    for name in ("tanh_d2_o4", "identity_d7_o3", "relu_d1_o1"):
        c = cases()[name]
        ch = c.chains[2]
        M = ch["M"].copy(); M[c.units[2][0], 9] = 2.0 ** 20
        if c.act == "tanh":
            worst = max(worst, hidden_model(M, ch["b1"], None, False, m_a=np.array(ch["rows"], dtype=np.int64))[3])
        else:
            A = np.array(ch["rows"], dtype=np.float64)
            worst = max(worst, hidden_model(M, ch["b1"], np.maximum(A, 0.0) if c.act == "relu" else A, True)[3])
    assert worst < 6 * 64 * (1 << 14)
    print(f"other cases: largest |level accumulator| {worst} = 2^{math.log2(worst):.1f}")
