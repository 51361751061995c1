"""Host arithmetic of the conjugate-gradient mirror (parity_checks.cg_solve_mirror) checked against exact references: the
float32 fused multiply-add against fractions.Fraction, the workgroup sum of k_cg_step against math.fsum and a literal
thread-by-thread transcription, the padded parameter layout against the network it describes."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import policy as op
from tests import helpers


def _round_f32(q):
    """the float32 nearest to the rational q, ties to the even significand (zero: +0)"""
    f = np.float32(float(q))          # within one float32 step of the answer
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    best = None
    for c in cands:
        if not np.isfinite(c):
            continue
        d = abs(Fraction(float(c)) - q)
        key = (d, int(np.array(c, np.float32).view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, c)
    return np.float32(best[1])


def _fma_exact(a, b, c):
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if q == 0:       # IEEE 754: an exact zero sum is +0 under round to nearest, unless both addends are -0
        neg = (np.signbit(a) != np.signbit(b)) and np.signbit(c)
        return np.float32(-0.0) if neg else np.float32(0.0)
    return _round_f32(q)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _fma_cases():
    rng = np.random.RandomState(0)
    cols = []
    # random values over many binades, both signs
    n = 6000
    mag = lambda k: (rng.uniform(1, 2, k) * np.exp2(rng.randint(-30, 30, k))) * rng.choice([-1, 1], k)
    cols.append((mag(n), mag(n), mag(n)))
    # a * b and c of comparable size with opposite signs: heavy cancellation
    a = mag(2000)
    b = mag(2000)
    c = -(a.astype(np.float32).astype(np.float64) * b.astype(np.float32)) * (1 + rng.uniform(-1e-6, 1e-6, 2000))
    cols.append((a, b, c))
    # constructed ties: a * b = (1 + i 2^-12)(1 + j 2^-12) with i j odd lies exactly halfway between two float32 values;
    # c = 0 (a true tie: to even) or a tiny c of either sign (the exact sum is off the midpoint, a double-rounded fma errs)
    i = rng.randint(1, 2048, 3000) | 1
    j = rng.randint(1, 2048, 3000) | 1
    sc = np.exp2(rng.randint(-20, 20, 3000))
    sg = rng.choice([-1, 1], 3000)
    a = (1 + i * 2.0 ** -12) * sc * sg
    b = 1 + j * 2.0 ** -12
    tiny = rng.choice([-1, 0, 1], 3000) * rng.uniform(1, 2, 3000) * np.exp2(rng.randint(-80, -60, 3000)) * sc
    cols.append((a, b, tiny))
    # exact cancellation to +-0 (products exact in float32), and signed zeros
    a = rng.randint(-4096, 4096, 500).astype(np.float64)
    b = rng.randint(-4096, 4096, 500).astype(np.float64)
    cols.append((a, b, -(a * b)))
    cols.append((np.array([0.0, -0.0, 0.0, -0.0, -0.0, 1.0, -1.0]), np.array([1.0, 1.0, -1.0, -1.0, 3.0, 0.0, -0.0]),
                 np.array([-0.0, -0.0, -0.0, 0.0, -0.0, -0.0, -0.0])))
    # near a binade edge: results just below / at / above a power of two
    below1 = np.float32(1) - np.float32(2 ** -24)
    k = 500
    a = np.full(k, below1, np.float64) * np.exp2(rng.randint(-10, 10, k))
    b = np.exp2(-np.log2(np.abs(a)).round()) * rng.choice([1.0, float(below1), 1 + 2.0 ** -23], k)
    c = rng.choice([-1, 1], k) * np.exp2(rng.randint(-50, -20, k)) * rng.uniform(1, 2, k)
    cols.append((a, b, c))
    # subnormal results
    a = rng.uniform(1, 2, 200) * 2.0 ** -70
    b = rng.uniform(-2, 2, 200) * 2.0 ** -60
    c = rng.uniform(-1, 1, 200) * 2.0 ** -128
    cols.append((a, b, c))
    a, b, c = (np.concatenate([x[m] for x in cols]).astype(np.float32) for m in range(3))
    return a, b, c


def test_fma32_is_the_exactly_rounded_fused_multiply_add():
    a, b, c = _fma_cases()
    assert a.size >= 10000
    got = helpers.fma32(a, b, c)
    want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, [(a[k], b[k], c[k], got[k], want[k]) for k in bad[:5]]
    # the cases exercise what they claim: ties that a float64 multiply-add rounded to float32 gets wrong, exact zeros of both signs
    naive = (a.astype(np.float64) * b + c).astype(np.float32)
    assert np.count_nonzero(_bits(naive) != _bits(want)) > 100
    z = want == 0
    assert np.any(z & np.signbit(want)) and np.any(z & ~np.signbit(want))


def test_fma32_scalars_and_specials():
    assert helpers.fma32(np.float32(2), np.float32(3), np.float32(1)) == np.float32(7)
    assert np.isnan(helpers.fma32(np.float32(np.nan), np.float32(0), np.float32(0)))
    assert np.isnan(helpers.fma32(np.float32(0), np.float32(np.inf), np.float32(1)))
    assert helpers.fma32(np.float32(np.inf), np.float32(1), np.float32(1)) == np.inf


def _block_sum_literal(p):
    """k_cg_step's sum written out thread by thread, barrier by barrier"""
    buf = [0.0] * 1024
    for t in range(1024):
        s = 0.0
        for j in range(t, len(p), 1024):
            s += float(p[j])
        buf[t] = s
    s = 512
    while s > 0:
        for t in range(s):
            buf[t] += buf[t + s]
        s >>= 1
    return buf[0]


@pytest.mark.parametrize('n', [1, 1023, 1024, 1025, 70000])
def test_cg_block_sum_against_fsum_and_the_literal_order(n):
    rng = np.random.RandomState(n)
    p = rng.randn(n) * np.exp2(rng.randint(-20, 20, n))
    got = helpers.cg_block_sum(p)
    assert got == _block_sum_literal(p)
    exact = math.fsum(p)
    assert abs(got - exact) <= 4 * np.spacing(np.abs(p).sum()), (got, exact)
    # products of float32 values: the terms k_cg_step adds
    q = rng.randn(n).astype(np.float32).astype(np.float64) * rng.randn(n).astype(np.float32)
    assert helpers.cg_block_sum(q) == _block_sum_literal(q)


def test_cg_block_sum_models_the_order():
    """1e16 and -1e16 meet in thread 0 and cancel before the 1 of thread 1 is added: the workgroup order keeps the 1 that a
    pairwise (np.sum) or left-to-right order loses"""
    p = np.zeros(2048)
    p[0], p[1], p[1024] = 1e16, 1.0, -1e16
    assert helpers.cg_block_sum(p) == 1.0 == math.fsum(p)
    assert float(np.sum(p)) != 1.0 and sum(p.tolist()) != 1.0


@pytest.mark.parametrize('O,A,hidden,padded', [(20, 6, (100, 100), (128, 128)), (4, 2, (40, 40), (64, 64)),
                                               (5, 3, (20, 50), (32, 64)), (40, 3, (32, 32), (64, 64)),
                                               (20, 6, (64, 64), (64, 64)), (20, 6, (48, 48, 48), (48, 48, 48)),
                                               (10, 2, (16, 100), (128, 128)), (200, 4, (40, 40), (40, 40))])
def test_padded_layout_transcription(O, A, hidden, padded):
    """pad_dims / remap_params of promp_hip.hip in NumPy: the instantiated widths, a lossless round trip, and the padding where
    the network puts it -- the extra units have zero incoming weights, zero bias and zero outgoing weights"""
    assert helpers.padded_hidden(O, A, hidden) == padded
    assert helpers.padded_hidden(O, A, hidden, plain_tanh=False) == tuple(hidden)
    nu, npd = op.PolicySpec(O, A, hidden).n_params, op.PolicySpec(O, A, padded).n_params
    v = np.arange(1, nu + 1, dtype=np.float32)
    w = helpers.remap_params(O, A, hidden, padded, v, True)
    assert w.shape == (npd,) and np.count_nonzero(w) == nu
    np.testing.assert_array_equal(helpers.remap_params(O, A, hidden, padded, w, False), v)
    if len(hidden) != 2:
        return
    su, sp = op.PolicySpec(O, A, hidden), op.PolicySpec(O, A, padded)
    pu, pp = su.to_ordered_dict(v.astype(np.float64)), sp.to_ordered_dict(w.astype(np.float64))
    for name, m in pp.items():
        u = pu[name]
        sl = tuple(slice(0, s) for s in u.shape)
        np.testing.assert_array_equal(m[sl], u, err_msg=name)
        rest = m.copy()
        rest[sl] = 0
        assert not rest.any(), name
