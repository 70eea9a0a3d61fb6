"""Randomised parity of hk_mlp_forward, hk_train_mlp_forward / hk_train_mlp_backward, hk_pvnet_forward, hk_pvgrad_forward /
hk_pvgrad_backward and hk_customnet_forward where the driver sees it: a fixed, seeded slice of tests/fuzz_nets.py per
family (five of them), every array bit for bit against the numpy rules.  tests/test_fuzz_nets.py holds the slice itself
to account without a GPU: what it reaches, how many of its cases are degenerate, that the comparison can fail."""
import pytest

pytestmark = pytest.mark.gpu

SEED = 20261020
# sized by the rule, which dominates: rule-only seconds over the whole slice, measured without a GPU: mlp 9.8 s,
# train 10.4 s, pvnet 9.0 s, pvgrad 14.7 s, customnet 8.8 s (about 10 s per family is the budget; on the MI355X's host the
# whole tests, rule and launches, took 3.3 s, 3.9 s, 3.5 s, 5.1 s and 3.3 s: pvgrad within one half over the slowest
# of the others).  pvgrad lies above the budget: 65 cases are the FEWEST of this seed that reach everything
# test_fuzz_nets.missing asks for (its eighteen batches, the table's boundary counts and the net of more than two table
# launches are each a few per cent of the draws), and its rule takes a step of numpy per batch row and Dense whatever the
# widths -- half a second at 4 096 rows for the narrowest net.  Every launch is a small shape.
COUNT = {"mlp": 250, "train": 160, "pvnet": 95, "pvgrad": 65, "customnet": 150}


@pytest.mark.parametrize("family", list(COUNT))
def test_fuzz_slice(family):
    """run once; a failure names its family, case index, seed and the case's scalars (fuzz_nets.case_at rebuilds it)"""
    import fuzz_nets
    assert fuzz_nets.run_cases(family, COUNT[family], SEED) == COUNT[family]
