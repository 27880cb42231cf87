"""The random problems of the differential fuzz on long tile ranges (tools/fuzz_ranges.py): 48 fixed seeds under MMG_OPT_K1_RANGES
1 ... 40, every list a sample call launches over, the kernel and the cuts asserted against tests/k1_range_ref.py, every chain and two
EM sweeps compared bit for bit with the oracle.  The census -- no device -- shows what the fixed seeds reach: for every kind of list
the cases that walk one at 8 entries per range or more."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_census_of_the_fixed_seeds(orc):
    """The floors are conditions on the seeds, not measurements: 6 cases for the main list under the lean kernel, under the general
    kernel, the pair lists, the far / CSR list of paired chains and the multiplicity list, 3 for a main list with CSR-walked tiles."""
    import fuzz_ranges
    assert fuzz_ranges.N_SEEDS == 48
    got = fuzz_ranges.census(range(fuzz_ranges.FIRST_SEED, fuzz_ranges.FIRST_SEED + fuzz_ranges.N_SEEDS), orc)
    print("\ncensus of seeds %d ... %d: %r" % (fuzz_ranges.FIRST_SEED, fuzz_ranges.FIRST_SEED + fuzz_ranges.N_SEEDS - 1, got))
    assert fuzz_ranges.CENSUS_FLOORS == dict(main_lean=6, main_general=6, pairs=6, far_csr=6, multiplicity=6, main_with_csr_tiles=3)
    for kind, floor in fuzz_ranges.CENSUS_FLOORS.items():
        assert got[kind] >= floor, (kind, got[kind], floor)


@pytest.mark.gpu
@pytest.mark.parametrize("block", range(4))
def test_fuzz_ranges_block(gpu, orc, block):
    import fuzz_ranges
    for seed in range(fuzz_ranges.FIRST_SEED + 12 * block, fuzz_ranges.FIRST_SEED + 12 * (block + 1)):
        fuzz_ranges.one_case(seed, gpu, orc, verbose=False)
