"""The keyed streams over their whole key space and the scalar math pointwise, on the HOST instantiation of the library's inline code
(mmg_selftest_keyed and the older self tests with device = -1) against the CPU oracle: no GPU needed.  tests/test_gpu_key_space.py runs
the same checks (tests/key_space_checks.py) in kernels.

High seed words, chains up to the Gamma stream's 24 bits, 64-bit stream ids and iterations up to 2^32 - 1 are the part of the key
space the parity tests, the fuzz and the golden chains never enter (the key space)."""
import numpy as np
import pytest

import key_space_checks as K


@pytest.fixture(scope="module")
def gibbs():
    from mmseq_amd import gibbs
    return gibbs


def test_streams_over_the_key_space_equal_the_spec(gibbs, orc):
    K.check_streams(gibbs, orc, -1)


def test_stream_identities_of_the_key_derivation(gibbs):
    K.check_stream_identities(gibbs, -1)


@pytest.mark.parametrize("shape", K.GAMMA_SHAPES)
def test_gamma_shapes_equal_oracle(gibbs, orc, shape):
    K.check_gamma_shape(gibbs, orc, -1, shape)


@pytest.mark.parametrize("nn,p", K.BINOMIALS)
def test_binomial_edges_equal_oracle(gibbs, orc, nn, p):
    K.check_binomial(gibbs, orc, -1, nn, p)


def test_normal_equals_oracle(gibbs, orc):
    K.check_normal(gibbs, orc, -1)


def test_probit_equals_as241_transcription(gibbs, orc):
    K.check_probit(gibbs, orc, -1)


# The largest relative error of the transcription (hence of dprobit, bit for bit) over the grid, against mpmath at 50 digits: measured
# 7.57e-16 at p = 8.9e-176 in the far tail (r > 5); 6.5e-16 in the near tail (at 1 - 2e-5), 3.7e-16 in the central branch.  The bits are
# fixed; the factor 2 only guards a later change of the grid.
PROBIT_MAX_REL_ERR = 7.57e-16


def _probit_mp(x):
    """sqrt(2) erfinv(2 p - 1) at 50 digits.  In the tails 2 p - 1 is not representable near -1 at any affordable precision: there the value
    is the fp64 one refined by a Newton step on Phi(z) = p with mpmath's ncdf / npdf (the step squares a relative error of 1e-15)."""
    import mpmath as mp
    out = []
    with mp.workdps(50):
        for p in x:
            flip = p > 0.5
            pp = 1 - mp.mpf(p) if flip else mp.mpf(p)                    # exact: a double and its complement
            if pp > mp.mpf("1e-12"):
                z = mp.sqrt(2) * mp.erfinv(2 * pp - 1)
            else:
                z = mp.mpf(float(K.probit_as241(np.array([float(pp)]))[0]))
                z = z - (mp.ncdf(z) - pp) / mp.npdf(z)
            out.append(-z if flip else z)
    return out


def test_probit_transcription_accuracy_against_mpmath(orc):
    import mpmath as mp
    x = K.probit_grid()[:-6]                                               # the grid without its specials
    x = x[(x != 0.5) & (x < 1.0)]                                          # (probit(1/2) = 0 exactly; 1 - p rounds to 1 for the smallest p: +inf)
    got = K.probit_as241(x, orc.log_v)
    ref = _probit_mp(x)
    with mp.workdps(50):
        rel = [float(abs((mp.mpf(float(g)) - r) / r)) for g, r in zip(got, ref)]
    worst = int(np.argmax(rel))
    print("probit: max rel err %.3e at p = %r" % (rel[worst], x[worst]))
    assert rel[worst] <= 2 * PROBIT_MAX_REL_ERR


def test_lgamma_equals_numpy_restatement(gibbs):
    K.check_lgamma(gibbs, -1)


# stirling_tail against log(k!) - [(k + 1/2) log(k + 1) - (k + 1) + log(2 pi) / 2] at 50 digits, k = 0 .. 12, 1e9, 4.29e9: the largest
# relative error measured is 3.99e-9 at k = 10, the first argument of the three-term series (its truncation, 1 / (1680 (k + 1)^7) of a
# value 1 / (12 (k + 1))); 1e-16 at the large arguments; the table entries are good to 9.2e-15.
STIRLING_MAX_REL_ERR = 3.99e-9


def test_stirling_tail_against_log_factorial(gibbs):
    got = K.check_stirling(gibbs, -1)
    ref = [K.stirling_tail_mp(k) for k in K.STIRLING_K]
    rel = [abs(float((g - r) / r)) for g, r in zip(got, ref)]
    print("stirling_tail: rel err", ["%.2e" % v for v in rel])
    assert max(rel) <= 2 * STIRLING_MAX_REL_ERR
    assert max(rel[:10]) <= 1e-13                                          # the table


def test_ilogb_of_subnormals_against_frexp(gibbs):
    K.check_ilogb(gibbs, -1)


def test_word_maps_at_the_extreme_words_are_exact(gibbs):
    K.check_word_maps(gibbs, -1)


def test_gamma_stream_sees_24_bits_of_the_chain(orc):
    """Why mmg_sampler_create refuses chain indices beyond 2^24 (tests/test_gpu_error_paths.py): chain 2^24 redraws mu from the uniforms
    of chain 0 while it draws different rows -- and (seed + 2^32, chain 0) from those of (seed, chain 1)."""
    p, _ = orc.synth_problem(R=600, T=80, avg_hits=3, seed=5)
    rng = np.random.default_rng(0)
    cnt = rng.integers(0, 50, p.n).astype(np.int32)
    mu = rng.gamma(1.0, 1.0, p.n)
    base = orc.gamma_update(cnt, p.l, .1, .1, 1234, 0, 5)
    assert np.array_equal(base, orc.gamma_update(cnt, p.l, .1, .1, 1234, 1 << 24, 5))
    assert not np.array_equal(base, orc.gamma_update(cnt, p.l, .1, .1, 1234, (1 << 24) - 1, 5))
    assert np.array_equal(orc.gamma_update(cnt, p.l, .1, .1, 1234 + (1 << 32), 0, 5), orc.gamma_update(cnt, p.l, .1, .1, 1234, 1, 5))
    rows = orc.sample_counts(p, mu, 1234, 0, 5)
    assert not np.array_equal(rows, orc.sample_counts(p, mu, 1234, 1 << 24, 5))
    assert not np.array_equal(orc.sample_counts(p, mu, 1234 + (1 << 32), 0, 5), orc.sample_counts(p, mu, 1234, 1, 5))
