"""HIP stop-loss env vs oracle/stoploss_oracle.c, bit for bit, on the panels of
tests/twowave_domain_cases.py: closes on a price grid (where `//` is not floor(a / close)), price levels
from 1e-8 to 3e5 with quotients up to 2^49, dyadic prices on which every compare of the rule meets
equality, and zero closes (the reference's "missing data").  Every case first asserts, from the oracle's
trace alone, that the events it exists for occur (profiles/twowave_panel_domain.md has the counts)."""
import pytest

import twowave_domain_cases as tc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
KIND = "stoploss"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


@pytest.mark.parametrize("name,shape,args", tc.cases(KIND), ids=[tc.case_id(*c) for c in tc.cases(KIND)])
def test_stoploss_hip_matches_oracle_on_the_panel_domain(name, shape, args):
    _need_gpu()
    tc.replay_on_device(KIND, name, shape, args)


@pytest.mark.parametrize("name,shape,args", tc.window_cases(KIND),
                         ids=[tc.case_id(*c) for c in tc.window_cases(KIND)])
def test_stoploss_windowed_hip_matches_one_oracle_per_env(name, shape, args):
    _need_gpu()
    tc.replay_windowed(KIND, name, shape, args)
