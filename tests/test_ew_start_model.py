"""CPU model of the cost-derived start state of the in-sweep E/W strip segments (DESIGN.md
§4.4): a numpy restatement of G = min(K (A - min A), P2) and of the segment speculation, on
the bench's own census pair.  With G and a 9-column warmup no more segments enter their strip
in a wrong state than with the zero state and 18 columns (what the patch pass then repairs)."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import sgm_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def study():
    spec = importlib.util.spec_from_file_location("ew_start_study", os.path.join(ROOT, "tools", "ew_start_study.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _G(cols, K, P2):
    """The start state from the n cost columns cols[n][D] (independent restatement)."""
    A = np.sum(np.asarray(cols, np.int64), axis=0)
    return np.minimum(K * (A - A.min()), P2)


def test_start_state_restatement(study):
    rng = np.random.default_rng(7)
    C = rng.integers(0, 63, (3, 50, 32)).astype(np.int64)
    # E line whose first warmup column is 20: columns 19, 18, 17, 16; W line: 21..24
    g = study.start_state(C, 20, 1, 4, 8, 120)
    assert np.array_equal(g[1], _G([C[1, 19], C[1, 18], C[1, 17], C[1, 16]], 8, 120))
    g = study.start_state(C, 20, -1, 4, 8, 120)
    assert np.array_equal(g[2], _G([C[2, 21], C[2, 22], C[2, 23], C[2, 24]], 8, 120))
    assert g.min() == 0 and g.max() <= 120 and (g.min(-1) == 0).all()
    # a guess column outside [0, W1): the zero state; constant costs: A - min A = 0, the zero state
    assert not study.start_state(C, 3, 1, 4, 8, 120).any()
    assert not study.start_state(C, 46, -1, 4, 8, 120).any()
    assert not study.start_state(np.full((2, 50, 32), 17, np.int64), 20, 1, 4, 8, 120).any()


def test_guess_at_9_columns_is_as_good_as_zero_at_18(study):
    C, P1, P2 = study.costs(1003, 150, 199, "census")
    assert (P1, P2) == (10, 120) and C.shape[0] == 49
    for cs in (1, -1):
        T = study.true_states(C, cs, P1, P2)
        guess9, n = study.mismatch(C, T, cs, 9, 4, 8, P1, P2)
        zero18, _ = study.mismatch(C, T, cs, 18, 0, 0, P1, P2)
        zero9, _ = study.mismatch(C, T, cs, 9, 0, 0, P1, P2)
        print(f"dir {cs:+d}: {n} segments, guess/9 {guess9:.4f}, zero/18 {zero18:.4f}, zero/9 {zero9:.4f}")
        assert n > 1000
        assert guess9 <= 1.5 * zero18
    # the true states are the oracle's paths in the min-0 form
    L = sgm_np.aggregate_path(C, sgm_np.DIR_E, P1, P2)
    assert np.array_equal(study.true_states(C, 1, P1, P2), L - L.min(-1, keepdims=True))
