"""What tests/test_mmsim_cli.py and tests/test_gpu_sim.py share: where the mmsim binary lies, generated tables and gzip traces in the
formats tests/test_mmfold_cli.py writes, and draws as tests/test_gpu_fold.py makes them.  The writers are restated here, so that the
similarity tests collect whatever becomes of those modules."""
import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")
MMSIM = os.path.join(BIN_DIR, "mmsim")
INFIX = {"transcript": "", "identical": ".identical", "gene": ".gene"}


def draws(rng, F, S, sig=None):
    """(F, S) log-normal draws around a spread of levels, each feature with a spread of its own; sig: significant digits kept"""
    x = np.exp(rng.normal(-3.0, 2.0, F)[:, None] + rng.uniform(0.01, 1.5, F)[:, None] * rng.normal(0.0, 1.0, (F, S)))
    if sig is None:
        return x
    return np.array([float("%.*g" % (sig, v)) for v in x.ravel()]).reshape(x.shape)


def write_table(path, ids, log_mu, uh):
    with open(path, "w") as f:
        f.write("# Mapped fragments: 1000\n")
        f.write("feature_id\tlog_mu\tsd\tmcse\tiact\teffective_length\ttrue_length\tunique_hits\n")
        for n, m, u in zip(ids, log_mu, uh):
            f.write("%s\t%s\t0.1\t0.01\t1\t1000\t1200\t%d\n" % (n, m if isinstance(m, str) else repr(float(m)), u))


def write_trace(path, ids, draws, rows):
    """draws: (len(ids), rows or more); written as mmseq writes them, six significant digits.  Returns the values as they read back."""
    text = [" ".join(ids)]
    for k in range(rows):
        text.append(" ".join("%g" % draws[c][k] for c in range(len(ids))))
    with gzip.open(path, "wt") as f:
        f.write("\n".join(text) + "\n")
    return np.array([[float("%g" % v) for v in row] for row in draws])
