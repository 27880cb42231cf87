"""mmseq_amd.run_auto on two planted problems: every stage's decision is the rule of tests/autolength_ref.py applied to that stage's
device diagnostics, and the trace it ends with is the trace of a plain sampler of the final length.

The inputs were fixed on the CPU before any device run -- the oracle's keyed chain (oracle.binding.gibbs_keyed on the canonical layout,
two chains, seed 99) through tests/convergence_ref.py and tests/autolength_ref.py -- with trace_len 128, gibbs_iter 128, E = 125,
R = 1.05, f = 0.9, max_iter 4096.  40 transcripts, all judged, ceil(f judged) = 36.  Reference counts per stage (length: passes, least
ESS, largest R-hat):

  easy (every transcript 150 .. 400 reads of its own, 6 shared with its neighbour)
     128: 40 passes, 163.7, 1.025  -> stop at the first stage
  hard (10 pairs that share 400 reads and have 3 and 2 of their own, beside 20 easy transcripts)
     128: 24, 5.2, 1.340 -> extend      256: 30, 11.4, 1.134 -> extend     512: 32, 31.1, 1.061 -> extend
    1024: 33, 74.1, 1.033 -> extend    2048: 40, 137.3, 1.019 -> stop, before max_iter

No stage's count is within 2 of 36, and no transcript's ESS is within 3 % of E at any stage, so the 1e-8 by which a device ESS may
differ from the reference's cannot move a count: the test holds the device's counts to the reference's."""
import numpy as np
import pytest

import autolength_ref as A

pytestmark = pytest.mark.gpu
S, CHAINS, SEED, MAX_ITER = 128, 2, 99, 4096
ESS, RHAT, FRAC = 125.0, 1.05, 0.9
REFERENCE = {"easy": [(128, 40, "stop")],
             "hard": [(128, 24, "extend"), (256, 30, "extend"), (512, 32, "extend"), (1024, 33, "extend"), (2048, 40, "stop")]}


def planted(kind, seed=1):
    rng = np.random.default_rng(seed)
    n, rows = 40, []
    first_easy = 0
    if kind == "hard":
        first_easy = 20
        for a in range(0, 20, 2):                              # 10 pairs that share all but a few reads
            rows += [[a, a + 1]] * 400 + [[a]] * 3 + [[a + 1]] * 2
    for t in range(first_easy, n):
        rows += [[t]] * int(rng.integers(150, 400))
        if t + 1 < n:
            rows += [[t, t + 1]] * 6
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    rp = np.zeros(len(rows) + 1, np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([t for r in rows for t in r], np.uint32)
    return rp, ci, rng.uniform(500.0, 2500.0, n)


@pytest.mark.parametrize("kind", ["easy", "hard"])
def test_stages_follow_the_rule_and_end_on_the_plain_trace(gpu, kind):
    from mmseq_amd import run_auto
    rp, ci, l = planted(kind)
    prob = gpu.Problem.from_csr(rp, ci, l)
    mu0, _ = prob.start_values()
    s = gpu.Sampler(prob, mu0, seed=SEED, n_chains=CHAINS, gibbs_iter=S, trace_len=S)
    stages = run_auto(s, MAX_ITER, ess=ESS, rhat=RHAT, frac=FRAC)
    for st in stages:
        print(kind, st["gibbs_iter"], st["judged"], st["passes"], st["min_ess"], st["max_rhat"], st["decision"])
    for j, st in enumerate(stages):
        want = A.judge(st["rhat"], st["ess_bulk"], st["ess_tail"], ESS, RHAT, FRAC)
        assert (st["judged"], st["passes"]) == (want["judged"], want["passes"]) and st["min_ess"] == want["min_ess"] and st["max_rhat"] == want["max_rhat"]
        assert st["gibbs_iter"] == S << j and st["gibbs_ss"] == 1 << j
        assert st["decision"] == ("stop" if want["stop"] else "extend" if 2 * st["gibbs_iter"] <= MAX_ITER else "max")
        assert abs(st["passes"] - want["needed"]) > 2           # the margin the inputs were chosen for
    assert [(st["gibbs_iter"], st["passes"], st["decision"]) for st in stages] == REFERENCE[kind]
    assert all(st["judged"] == 40 for st in stages)
    L = stages[-1]["gibbs_iter"]
    assert s.gibbs_iter == L and s.iteration == L
    plain = gpu.Sampler(prob, mu0, seed=SEED, n_chains=CHAINS, gibbs_iter=L, trace_len=S)
    plain.run(L)
    for c in range(CHAINS):
        assert np.array_equal(s.trace(c).view(np.uint64), plain.trace(c).view(np.uint64))
        for a, b in zip(s.moments(c), plain.moments(c)):
            assert np.array_equal(a, b)


def test_max_iter_ends_the_run_with_max(gpu):
    from mmseq_amd import run_auto
    rp, ci, l = planted("hard")
    prob = gpu.Problem.from_csr(rp, ci, l)
    mu0, _ = prob.start_values()
    s = gpu.Sampler(prob, mu0, seed=SEED, n_chains=CHAINS, gibbs_iter=S, trace_len=S)
    stages = run_auto(s, 2 * S, ess=ESS, rhat=RHAT, frac=FRAC)
    assert [(st["gibbs_iter"], st["passes"], st["decision"]) for st in stages] == [(128, 24, "extend"), (256, 30, "max")]
    assert s.gibbs_iter == 2 * S and s.iteration == 2 * S
    with pytest.raises(ValueError):
        run_auto(s, S)
