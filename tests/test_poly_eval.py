"""lumen_poly_eval_columns / lumen_group_poly_eval (include/lumenos_hip.h): the committed polynomial P(z) the server
returns next to the proof (cmd/server/main.go:255-258; P = core.NewDensePolyFromMatrix(matrix), Horner in
core/poly.go:13-45), evaluated on the device, against Horner in Python integers over the row-major flattening."""
import ctypes as C
import random

import numpy as np
import pytest

from tests.helpers import T_REF, make_context, make_params

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (512, 16), (2048, 64)]


def horner(m, z, t=T_REF):
    """core/poly.go:21-30 over M[i][j] mod T in row-major order (coefficient i*cols + j)"""
    r = 0
    for c in reversed([int(x) % t for x in np.asarray(m).reshape(-1)]):
        r = (r * z + c) % t
    return r


def points(seed):
    return [0, 1, T_REF - 1, random.Random(seed).randrange(2, T_REF - 1)]


@pytest.fixture(scope="module")
def pe(oracle):
    P = make_params(oracle, 11, 2)  # N = 2048 >= every row count below
    ctx = make_context(P)
    yield P, ctx
    ctx.close()


def witnesses(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return {
        "reduced": rng.integers(0, T_REF, size=(rows, cols), dtype=np.uint64),
        "max": np.full((rows, cols), T_REF - 1, dtype=np.uint64),
        "unreduced": rng.integers(T_REF, 2**64 - 1, size=(rows, cols), dtype=np.uint64, endpoint=True),  # values >= T
    }


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_whole_matrix_matches_python_horner(pe, rows, cols):
    P, ctx = pe
    for kind, m in witnesses(rows, cols, rows * 7 + cols).items():
        columns = np.ascontiguousarray(m.T)  # [cols][rows]: the layout of lumen_encrypt_values
        for z in points(rows + cols):
            assert ctx.poly_eval_columns(columns, 0, cols, z) == horner(m, z), (rows, cols, kind, z)
    # a point given unreduced counts as its residue
    m = witnesses(rows, cols, 3)["reduced"]
    assert ctx.poly_eval_columns(np.ascontiguousarray(m.T), 0, cols, T_REF + 5) == horner(m, 5)


@pytest.mark.parametrize("rows,cols", [(3, 5), (512, 16), (2048, 64), (7, 40)])
def test_column_blocks_sum_to_the_whole(pe, rows, cols):
    """partials of disjoint blocks with uneven first_column splits sum mod T to P(z); page-locked input too"""
    from lumenos_amd.hip import pinned_empty, pinned_free
    P, ctx = pe
    m = witnesses(rows, cols, 11)["unreduced"]
    columns = np.ascontiguousarray(m.T)
    z = points(cols)[3]
    whole = ctx.poly_eval_columns(columns, 0, cols, z)
    assert whole == horner(m, z)
    rng = random.Random(cols)
    for _ in range(3):
        cuts = sorted({0, cols} | {rng.randrange(0, cols + 1) for _ in range(3)})
        parts = [ctx.poly_eval_columns(columns[a:b], a, cols, z) for a, b in zip(cuts, cuts[1:])]
        assert sum(parts) % T_REF == whole, cuts
        for (a, b), p in zip(zip(cuts, cuts[1:]), parts):
            want = sum(int(m[i, j]) % T_REF * pow(z, i * cols + j, T_REF) for i in range(rows) for j in range(a, b)) % T_REF \
                if rows * (b - a) <= 4096 else p
            assert p == want, (a, b)
    assert ctx.poly_eval_columns(columns[:0], cols, cols, z) == 0  # an empty block at the end
    pin = pinned_empty(columns.shape)
    pin[:] = columns
    assert ctx.poly_eval_columns(pin, 0, cols, z) == whole
    pinned_free(pin)


def test_refused_arguments_name_what_is_wrong(oracle, pe):
    from lumenos_amd.hip import Context, LumenError, _p64
    P, ctx = pe
    cols = np.zeros((4, 8), dtype=np.uint64)
    with pytest.raises(LumenError, match="rows=0 out of range"):
        ctx.poly_eval_columns(np.zeros((4, 0), dtype=np.uint64), 0, 4, 3)
    with pytest.raises(LumenError, match=r"rows=4096 out of range \[1, N = 2048\]"):
        ctx.poly_eval_columns(np.zeros((1, 4096), dtype=np.uint64), 0, 4, 3)
    with pytest.raises(LumenError, match="first_column \\+ count = 1 \\+ 4 exceeds cols = 4"):
        ctx.poly_eval_columns(cols, 1, 4, 3)
    with pytest.raises(LumenError, match="first_column \\+ count = 0 \\+ 4 exceeds cols = 3"):
        ctx.poly_eval_columns(cols, 0, 3, 3)
    lib, out = ctx.lib, C.c_uint64()
    assert lib.lumen_poly_eval_columns(ctx.h, None, 8, 4, 0, 4, 3, C.byref(out)) != 0
    assert b"values is NULL" in lib.lumen_last_error(ctx.h)
    assert lib.lumen_poly_eval_columns(ctx.h, _p64(cols), 8, 4, 0, 4, 3, None) != 0
    assert b"partial is NULL" in lib.lumen_last_error(ctx.h)
    assert lib.lumen_poly_eval_columns(None, _p64(cols), 8, 4, 0, 4, 3, C.byref(out)) != 0
    assert b"ctx is NULL" in lib.lumen_last_error(None)
    no_t = Context(P.logN, P.moduli[:P.L], P.moduli[P.L:], P.psi, 0)  # a context without a plaintext modulus
    with pytest.raises(LumenError, match="no plaintext modulus"):
        no_t.poly_eval_columns(cols, 0, 4, 3)
    no_t.close()
    assert ctx.poly_eval_columns(cols, 0, 4, 3) == 0  # the context is still usable


@pytest.mark.parametrize("world", [2, 4, 8])
def test_group_of_contexts_on_one_gpu_gives_the_one_gpu_value(pe, world):
    """lumen_group_poly_eval with W contexts of one process (copy transport): every rank evaluates its own block,
    the partials are summed inside the library"""
    from lumenos_amd.hip import Group, LumenError
    P, ctx = pe
    rows, cols = 512, 64
    m = witnesses(rows, cols, world)["unreduced"]
    columns = np.ascontiguousarray(m.T)
    z = points(world)[3]
    want = ctx.poly_eval_columns(columns, 0, cols, z)
    assert want == horner(m, z)
    ctxs = [ctx] + [ctx.clone() for _ in range(world - 1)]
    g = Group(ctxs, transport="copy")
    c = cols // world
    assert g.poly_eval([columns[r * c:(r + 1) * c] for r in range(world)], cols, z) == want
    # uneven blocks are fine as long as they cover the matrix in rank order
    cuts = [0, 1] + [c * r + 3 for r in range(1, world - 1)] + [cols]
    assert g.poly_eval([columns[a:b] for a, b in zip(cuts, cuts[1:])], cols, z) == want
    with pytest.raises(LumenError, match="counts sum to"):
        g.poly_eval([columns[r * c:(r + 1) * c - 1] for r in range(world)], cols, z)
    with pytest.raises(LumenError, match="rows=0 out of range"):
        g.poly_eval([np.zeros((c, 0), dtype=np.uint64) for _ in range(world)], cols, z)
    assert g.poly_eval([columns[r * c:(r + 1) * c] for r in range(world)], cols, z) == want
    g.close()
    for x in ctxs[1:]:
        x.close()
