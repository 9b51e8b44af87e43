"""lumen_group_poly_eval in the one-process-per-GPU form (lumen_group_create_rank), W host threads playing the W
processes on ONE GPU.  Like tests/group_per_rank_cases.py, NOT collected by a plain `pytest tests`: it needs the RCCL
test double tests/cpp/fake_rccl.cpp in a fresh process; tests/test_poly_eval_rccl.py runs it there."""
import numpy as np
import pytest

from tests.group_per_rank_cases import run_ranks
from tests.helpers import T_REF
from tests.test_group import FAKE, ranks_of, small  # noqa: F401 -- `small` is the module fixture

pytestmark = pytest.mark.gpu
assert FAKE, "run through tests/test_poly_eval_rccl.py (LUMEN_TEST_GROUP_TRANSPORT=rccl + the test double)"


def horner(m, z):
    r = 0
    for c in reversed([int(x) % T_REF for x in m.reshape(-1)]):
        r = (r * z + c) % T_REF
    return r


@pytest.mark.parametrize("world", [2, 4])
def test_per_rank_poly_eval_and_a_rank_with_bad_arguments(small, world):
    """every rank evaluates its own block and receives P(z) of the whole matrix through the one all-gather; then one
    rank passes a bad argument (a block wider than the matrix): every rank fails -- the offender with what is wrong,
    the others with who rejected -- none blocks, and the group is still usable afterwards"""
    from lumenos_amd.hip import Group, LumenError
    P, ctx = small
    rows, cols = 96, 32
    rng = np.random.default_rng(world)
    m = rng.integers(0, 2**64 - 1, size=(rows, cols), dtype=np.uint64, endpoint=True)
    columns = np.ascontiguousarray(m.T)
    z = int(rng.integers(2, T_REF - 1))
    want = horner(m, z)
    assert ctx.poly_eval_columns(columns, 0, cols, z) == want
    ctxs = ranks_of(ctx, world)
    uid = Group.unique_id()
    c = cols // world
    ok = [None] * world

    def body(r):
        g = Group.join(ctxs[r], r, world, uid)
        assert g.transport == "rccl"
        assert g.poly_eval([columns[r * c:(r + 1) * c]], cols, z) == want
        bad = r == world - 1  # the last rank says the matrix has c - 1 columns: its own block of c exceeds that
        with pytest.raises(LumenError, match="exceeds cols" if bad else "rank %d rejected its arguments" % (world - 1)):
            g.poly_eval([columns[r * c:(r + 1) * c]], c - 1 if bad else cols, z)
        assert g.poly_eval([columns[r * c:(r + 1) * c]], cols, z) == want
        g.sync()
        ok[r] = g

    errs = run_ranks(world, body)
    assert errs == [None] * world, errs
    for g in ok:
        g.close()
    for x in ctxs[1:]:
        x.close()
