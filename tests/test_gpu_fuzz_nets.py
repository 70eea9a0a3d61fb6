"""Randomised parity of hk_mlp_forward, hk_train_mlp_forward / hk_train_mlp_backward and hk_pvnet_forward where the driver
sees it: a fixed, seeded slice of tests/fuzz_nets.py per family, every array bit for bit against the numpy rules.
tests/test_fuzz_nets.py holds the slice itself to account without a GPU: what it reaches, how many of its cases are
degenerate, that the comparison can fail."""
import pytest

pytestmark = pytest.mark.gpu

SEED = 20261020
# sized by the rule, which dominates: rule-only seconds over the whole slice, measured without a GPU: mlp 9.8 s,
# train 10.4 s, pvnet 9.0 s (about 10 s per family is the budget; on the MI355X's host the whole tests, rule and
# launches, took 3.4 s, 4.0 s and 3.5 s).  Every launch is a small shape.
COUNT = {"mlp": 250, "train": 160, "pvnet": 95}


@pytest.mark.parametrize("family", list(COUNT))
def test_fuzz_slice(family):
    """run once; a failure names its family, case index, seed and the case's scalars (fuzz_nets.case_at rebuilds it)"""
    import fuzz_nets
    assert fuzz_nets.run_cases(family, COUNT[family], SEED) == COUNT[family]
