"""A short run of the differential fuzz driver (tests/fuzz_gpu.py) so that it stays exercised: random annotation sizes,
read modes, preset flags and overrides, reads of the synthetic generator and of tests/adversarial.py; rows and the records-in / records-out stream against the oracle, and
every round's device row table through quant, the fragment-length histogram and coverage against the yardsticks (tests/route_cases.py)."""
import pytest

from tests import fuzz_gpu

pytestmark = pytest.mark.gpu


# 303: six of its 25 rounds draw from tests/adversarial.py (tests/test_cigar_alphabet_cpu.py replays the draw)
@pytest.mark.parametrize("seed", [101, 202, 303])
def test_fuzz_rounds_agree_with_the_oracle(seed):
    bad = fuzz_gpu.run(25, seed, verbose=False, read_counts=(200, 800), gene_counts=(30, 120))
    assert bad is None, bad
