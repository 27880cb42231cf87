"""CPU checks of `mmdiff -chains`: every refusal exits 1 with its message before any device is touched, a valid run passes every check
and ends at the missing device, and the pooling restatement (tests/mmdiff_chains_ref.py) against closed forms."""
import math
import os

import numpy as np
import pytest

import mmdiff_chains_ref as CR
import mmdiff_ref as R
from test_mmdiff_cli import run, samples, write_matrices
from test_mmdiff_poly_cli import ALT_A, ALT_B

FAST = ["-burnin", "1024", "-iter", "1024", "-notune"]


@pytest.mark.parametrize("value", ["0", "17", "-1", "2.5", "x", "3x", ""])
def test_chains_value_must_be_an_integer_from_1_to_16(tmp_path, value):
    files = samples(tmp_path, S=4, F=20)
    r = run(["-chains", value, "-de", "2", "2"] + files)
    assert r.returncode == 1 and b"Error: -chains takes an integer between 1 and 16." in r.stderr, r.stderr
    assert b"no HIP device" not in r.stderr and r.stdout == b""


def test_refusals_come_before_the_device(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    a, b = write_matrices(tmp_path / "a.mat", ALT_A), write_matrices(tmp_path / "b.mat", ALT_B)
    r = run(["-chainout", str(tmp_path / "o"), "-de", "2", "2"] + files)
    assert r.returncode == 1 and b"Error: -chainout needs -chains." in r.stderr and b"Usage: mmdiff" in r.stderr
    for n in ("1", "3"):
        r = run(["-chains", n, "-m", a, "-m", b] + files)
        assert r.returncode == 1 and b"Error: -chains cannot be combined with more than one -m or with -polyclass" in r.stderr, r.stderr
        assert b"left for later" in r.stderr and b"no HIP device" not in r.stderr and r.stdout == b""
    r = run(["-polyclass", "-chains", "2", "x.mmdiff", "y.mmdiff"])
    assert r.returncode == 1 and b"Error: -chains cannot be combined with more than one -m or with -polyclass" in r.stderr
    r = run(["-chains"])
    assert r.returncode == 1 and b"Error: mandatory arguments missing." in r.stderr
    # BASE that cannot be created: with several chains and with one
    for n in ("3", "1"):
        r = run(FAST + ["-chains", n, "-chainout", str(tmp_path / "no_such_dir" / "base"), "-de", "2", "2"] + files)
        assert r.returncode == 1 and b"Error: couldn't create" in r.stderr and b".chain0.mmdiff" in r.stderr, r.stderr
        assert b"no HIP device" not in r.stderr and r.stdout == b""
    r = run(["-de", "2", "2", "-chains", "2"] + files)
    assert r.returncode == 1 and b"Error: optional arguments must be specified before -de or -m." in r.stderr


def test_no_refusal_reaches_a_device(tmp_path):
    """The refusals above run with HIP_VISIBLE_DEVICES=-1; here with the caller's environment."""
    files = samples(tmp_path, S=4, F=20)
    r = run(["-chains", "17", "-de", "2", "2"] + files, env=dict(os.environ))
    assert r.returncode == 1 and b"no HIP device" not in r.stderr and r.stdout == b""


@pytest.mark.parametrize("n", [1, 3])
def test_valid_chains_run_passes_every_check_then_needs_a_device(tmp_path, n):
    files = samples(tmp_path, S=4, F=120)
    base = str(tmp_path / "out")
    r = run(FAST + ["-chains", str(n), "-chainout", base, "-de", "2", "2"] + files)
    assert r.returncode == 1 and r.stdout == b""
    assert b"Analysing 120 features" in r.stderr and b"Design matrix for model 1" in r.stderr
    assert r.stderr.rstrip().endswith(b"Error: no HIP device available: mmdiff has no CPU fallback")
    assert all(os.path.exists("%s.chain%d.mmdiff" % (base, c)) for c in range(n))      # creatable: checked before the device


def test_usage_lists_the_new_options():
    r = run(["-h"])
    for text in (b"-chains INT", b"-chainout STRING", b"STRING.chain<c>.mmdiff", b"chains of several alternatives are left for later",
                 b"log_bf, log_bf_sd, log_bf_mcse, chains_mixed", b"-chains C [-chainout BASE]", b"16 chains."):
        assert text in r.stderr, text


def test_library_checks_chains_arguments_before_the_device():
    from mmseq_amd._lib import MMGError
    from mmseq_amd.diff import DiffChains
    M, P0, P1, C = R.de_design([3, 3])
    y, e = np.ones((4, 6)), np.full((4, 6), 0.1)
    for n in (0, 17):
        with pytest.raises(MMGError) as ex:
            DiffChains(y, e, M, P0, P1, C, n, 1024)
        assert ex.value.code == 1 and "chains must be between 1 and 16" in str(ex.value)
    for total in (0, 8, 1000):
        with pytest.raises(MMGError) as ex:
            DiffChains(y, e, M, P0, P1, C, 2, total)
        assert ex.value.code == 1 and "multiple of 16" in str(ex.value)


# ---- the pooling restatement against closed forms --------------------------------------------------------------------------
T = 1024


def even_batches(G):
    """Batch sums of a chain whose gamma sum G is spread as evenly as integers allow."""
    q, r = divmod(int(G), CR.NB)
    return [float(q + (1 if k < r else 0)) for k in range(CR.NB)]


def pool(Gs, os_, gbs=None):
    """One feature: the chains' gamma sums and logit p'."""
    gbs = [even_batches(G) for G in Gs] if gbs is None else gbs
    r = CR.pool(np.array(Gs, np.float64)[:, None], np.array(os_, np.float64)[:, None], np.array(gbs, np.float64)[:, :, None], T)
    return {k: v[0] for k, v in r.items()}


def logit(g):
    return math.log(g) - math.log1p(-g)


@pytest.mark.parametrize("C,G,o", [(2, 512, 0.0), (3, 100, 1.25), (8, 1000, -3.5), (16, 1, 0.3)])
def test_equal_chains_give_the_single_chain_estimate(C, G, o):
    """C chains with equal g and o: sum sigmoid(b + o) = C g, so b = logit(g) - o; 64 halvings of a 2048-wide bracket leave 2^-53, and
    the 1e-12 allows for the few ulps of dexp in the sigmoid."""
    r = pool([G] * C, [o] * C)
    assert abs(r["log_bf"] - (logit(G / T) - o)) <= 1e-12
    assert r["chains_mixed"] == C and r["log_bf_sd"] <= 1e-12          # (the mean of C equal numbers is rounded)
    assert r["log_bf_mcse"] >= 0.0 and math.isfinite(r["log_bf_mcse"])


def test_no_draw_and_every_draw_of_model_1():
    r = pool([0, 0, 0], [0.5, -0.5, 0.0])
    assert r["log_bf"] == -math.inf and r["chains_mixed"] == 0 and math.isnan(r["log_bf_sd"]) and math.isnan(r["log_bf_mcse"])
    assert CR.bayes_factor(r["log_bf"]) == 0.0
    r = pool([T, T], [0.5, -0.5])
    assert r["log_bf"] == math.inf and r["chains_mixed"] == 0 and math.isnan(r["log_bf_sd"]) and math.isnan(r["log_bf_mcse"])
    assert CR.bayes_factor(r["log_bf"]) == math.inf


@pytest.mark.parametrize("stuck", [0, T])
def test_one_stuck_chain_pulls_the_estimate_towards_its_side(stuck):
    """Two mixed chains and one stuck in model 0 (or 1): the estimate stays finite and moves from the mixed chains' own pooled estimate
    towards the stuck side (the direction only).  The stuck chain is not among the mixed, so the sd is that of the two."""
    Gs, os_ = [300, 420, stuck], [0.2, -0.1, 0.4]
    r = pool(Gs, os_)
    two = pool(Gs[:2], os_[:2])
    ell = [logit(Gs[c] / T) - os_[c] for c in range(2)]
    assert math.isfinite(r["log_bf"]) and r["chains_mixed"] == 2 and min(ell) < two["log_bf"] < max(ell)
    assert r["log_bf"] < two["log_bf"] if stuck == 0 else r["log_bf"] > two["log_bf"]
    assert abs(r["log_bf_sd"] - abs(ell[0] - ell[1]) / math.sqrt(2.0)) <= 1e-12
    assert r["log_bf_sd"] == two["log_bf_sd"]


def test_sd_of_two_chains():
    Gs, os_ = [200, 700], [0.7, -1.1]
    r = pool(Gs, os_)
    ell = [logit(Gs[c] / T) - os_[c] for c in range(2)]
    assert abs(r["log_bf_sd"] - abs(ell[0] - ell[1]) / math.sqrt(2.0)) <= 1e-12 * abs(ell[0] - ell[1])
    assert min(ell) < r["log_bf"] < max(ell)
    one = pool([200, 0], os_)
    assert one["chains_mixed"] == 1 and math.isnan(one["log_bf_sd"])


def test_mcse_of_one_offset_is_the_delta_method():
    """Equal offsets: b = logit(mean g) - o and w_c = g (1 - g) for every chain, so mcse = sqrt(sum v_c) / (C g (1 - g)): the standard
    error of the mean of the chains' g through d logit / d g."""
    rng = np.random.default_rng(4)
    gbs = rng.integers(10, 50, (4, CR.NB)).astype(np.float64)
    Gs = gbs.sum(1)
    r = pool(list(Gs), [0.3] * 4, gbs)
    g = Gs.sum() / (4 * T)
    v = sum(((gbs[c] / (T // CR.NB) - Gs[c] / T) ** 2).sum() / 15 / 16 for c in range(4))
    assert abs(r["log_bf_mcse"] - math.sqrt(v) / (4 * g * (1 - g))) <= 1e-9 * r["log_bf_mcse"]


@pytest.mark.parametrize("o", [math.inf, -math.inf])
def test_a_non_finite_offset_makes_the_row_nan(o):
    r = pool([300, 400], [0.0, o])
    assert all(math.isnan(r[k]) for k in ("log_bf", "log_bf_sd", "log_bf_mcse"))
    assert math.isnan(CR.bayes_factor(r["log_bf"]))


def test_chain_streams_put_the_chain_into_the_key_and_restore_it():
    k0 = R.stream_key(77, 0, R.TAG_DIFF)
    with CR.chain_streams(3):
        inside = R.Streams(77, R.TAG_DIFF, [0], 0)
        perm = R.permutation(77, 5, 6)
    assert (inside.k0, inside.k1) == (k0[0], k0[1] ^ 3)
    assert (inside.k0, inside.k1) == R.stream_key(77 ^ (3 << 32), 0, R.TAG_DIFF)       # the seed-shifted single chain
    assert perm == R.permutation(77, 5, 6) and R.stream_key(77, 0, R.TAG_DIFF) == k0
