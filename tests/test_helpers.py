"""The shared pieces of the suite (tests/helpers.py, tests/cells.py), without a device."""
from types import SimpleNamespace

import numpy as np
import pytest

from cells import cell_cache
from helpers import bound_chain, both_routes, canonical


def test_canonical_on_sets_and_on_key_shaped_arrays():
    P = SimpleNamespace(moduli=[97, 193, 257])
    cts = np.zeros((3, 2, 2, 8), dtype=np.uint64)  # [count][2][nl][N], nl below the chain's length
    cts[:, :, 0], cts[:, :, 1] = 96, 192
    assert canonical(P, cts)
    cts[2, 1, 1, 5] = 193  # one word equal to q
    assert not canonical(P, cts)
    key = np.zeros((2, 2, 3, 8), dtype=np.uint64)  # [beta][2][L + K][N]
    key[..., 2, :] = 256
    assert canonical(P, key)
    key[1, 0, 0, 7] = 97
    assert not canonical(P, key)


@pytest.mark.parametrize("log_n", [8, 15])
def test_bound_chain_sits_in_the_window_below_the_bound(oracle, log_n):
    P = bound_chain(oracle, log_n, 3, 2)
    qmax = (2**64 - 1) // (3 * log_n + 8)
    assert (P.L, P.K) == (3, 2) and len(set(P.moduli)) == 5
    assert all(qmax - (217 << (log_n + 1)) < q <= qmax and q % (2 << log_n) == 1 for q in P.moduli)


class _FakeContext:
    def __init__(self):
        self.calls = []

    def set_tuning(self, name, value):
        self.calls.append((name, value))


def test_both_routes_runs_on_then_off_and_restores_the_default_when_the_call_raises():
    ctx = _FakeContext()
    assert both_routes(ctx, "SWITCH", lambda: ctx.calls[-1][1]) == (1, 0)
    assert ctx.calls == [("SWITCH", 1), ("SWITCH", 0), ("SWITCH", 1)]

    def call():
        raise KeyError("from the call")

    ctx = _FakeContext()
    with pytest.raises(KeyError):
        both_routes(ctx, "SWITCH", call, default=-1)
    assert ctx.calls == [("SWITCH", 1), ("SWITCH", -1)]


def test_cell_cache_builds_on_demand_and_closes_every_cell_it_made():
    made, closed = [], []

    def make(*key):
        made.append(key)
        return SimpleNamespace(key=key, close=lambda: closed.append(key))

    gen = cell_cache(make)
    get = next(gen)
    assert made == []
    a = get(10)
    assert get(10) is a and get(10, 2).key == (10, 2) and get(12) is not a
    assert made == [(10,), (10, 2), (12,)] and closed == []
    assert next(gen, None) is None
    assert closed == made


def test_cell_cache_closes_the_cells_after_one_whose_close_raises():
    closed = []

    def make(key):
        def close():
            closed.append(key)
            if key == 1:
                raise RuntimeError("close of cell 1")
        return SimpleNamespace(close=close)

    gen = cell_cache(make)
    get = next(gen)
    for key in (1, 2, 3):
        get(key)
    with pytest.raises(RuntimeError, match="close of cell 1"):
        next(gen)
    assert closed == [1, 2, 3]
