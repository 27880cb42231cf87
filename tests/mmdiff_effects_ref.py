"""numpy restatement of mmdiff's effect summaries (mmg_effects_of_rows, mmg_diff_effects_summarize).

rows (S, P, F): thinned states of a chain, gamma (0.0 / 1.0) as parameter P - 1.  Parameter s belongs to model model_of[s], and its
draws for feature f are rows[r, s, f] of the rows r whose own gamma, rows[r, P - 1, f], equals that model, in row order.  With n of
them:
    n[m, f]      the number of rows with gamma == m
    mean         the sequential sum of the draws in row order, divided by n
    sd           sqrt(sum (x - mean)^2 / (n - 1)), the sum again sequential in row order, in a second pass
    n_gt         the number of draws with x > 0 (neither -0.0 nor +0.0 counts)
    q[s, j, f]   the sorted draw at index floor(percentiles[j] / 100 * (n - 1) + 0.5)
mean, sd and q are NaN for n = 0, sd for n = 1.  The sums go through np.cumsum, which adds in index order (np.sum adds pairwise), and a
product is rounded before it is added, so that the numbers are the kernel's bit for bit.
"""
import math

import numpy as np


def picked_index(p, n):
    """The index of the sorted draws that percentile p picks among n >= 1 of them."""
    return int(math.floor(p / 100.0 * (n - 1) + 0.5))


def effects(rows, model_of, percentiles=(2.5, 50.0, 97.5)):
    rows = np.asarray(rows, np.float64)
    S, P, F = rows.shape
    model_of = np.asarray(model_of).ravel()
    pct = [float(p) for p in np.asarray(percentiles, np.float64).ravel()]
    if S < 1 or S > 4096 or P < 2 or len(pct) > 32 or len(model_of) != P - 1:
        raise ValueError("shapes out of range")
    if any(not (0.0 <= p <= 100.0) for p in pct) or np.any((model_of != 0) & (model_of != 1)):
        raise ValueError("percentiles must be in [0, 100] and models 0 or 1")
    gamma = rows[:, P - 1, :]
    if np.any((gamma != 0.0) & (gamma != 1.0)):
        raise ValueError("gamma must be 0.0 or 1.0")
    Q = P - 1
    out = dict(n=np.empty((2, F), np.uint32), mean=np.full((Q, F), np.nan), sd=np.full((Q, F), np.nan),
               n_gt=np.zeros((Q, F), np.uint32), q=np.full((Q, len(pct), F), np.nan))
    for m in range(2):
        out["n"][m] = (gamma == float(m)).sum(0)
    for f in range(F):
        keep = [gamma[:, f] == 0.0, gamma[:, f] == 1.0]
        for s in range(Q):
            x = rows[keep[model_of[s]], s, f]
            n = x.size
            if n == 0:
                continue
            with np.errstate(over="ignore", invalid="ignore"):
                mean = np.cumsum(x)[-1] / np.float64(n)
            out["mean"][s, f] = mean
            if n > 1:
                with np.errstate(over="ignore"):     # draws near 1e300: the squares overflow to inf here and in the kernel
                    d = x - mean
                    out["sd"][s, f] = np.sqrt(np.cumsum(d * d)[-1] / np.float64(n - 1))
            out["n_gt"][s, f] = np.count_nonzero(x > 0.0)
            xs = np.sort(x)
            for j, p in enumerate(pct):
                out["q"][s, j, f] = xs[picked_index(p, n)]
    return out


def model_of_names(names):
    """The model of each traced parameter from its name (tests/mmdiff_trace_ref.py: param_names, gamma excluded): the digit after the stem."""
    out = []
    for nm in names:
        stem = nm.split("_")[0]
        out.append(int(stem[-1]))
    return np.array(out, np.uint8)
