"""mmseq_amd -- MI355X-native Gibbs hot path of mmseq (eturro/mmseq), behind a C ABI.

csrc/      HIP kernels (gfx950), the C ABI (include/mmgibbs.h) and the C++ host code
gibbs.py   numpy-facing mirror of the C ABI (Problem, Sampler)
assign.py  posterior assignment probability of every hit from a chain's trace (Assign)
contrast.py posterior log-ratios between sets of transcripts of one sample from a chain's trace (Contrast)
pairs.py   posterior correlation of pairs of transcripts that share reads from a chain's trace (Pairs)
fold.py    posterior log fold change of features between two samples from all pairs of their draws (Fold)
similarity.py posterior distances and correlations between samples from their joint draws (Similarity)
isoforms.py posterior isoform usage within groups of transcripts: dominant-isoform probabilities and usage entropy (Isoforms, switch_probability)
"""
from .assign import Assign  # noqa: F401
from .isoforms import Isoforms, switch_probability  # noqa: F401
from .contrast import Contrast  # noqa: F401
from .pairs import Pairs  # noqa: F401
from .fold import Fold  # noqa: F401
from .similarity import Similarity  # noqa: F401
from .gibbs import Problem, Sampler, device_count  # noqa: F401
from .autolength import run_auto  # noqa: F401
