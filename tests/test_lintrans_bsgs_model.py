"""CPU: tests/lintrans_bsgs_model.py, the judge of the double-hoisted transform, is the diagonal method.  N = 2^8 and 2^10,
L = 3, K = 2, T_REF, a fresh pk encryption: for six diagonal sets the model's output decrypts (scale 1) to
sum_k d_k[i] * v[(i + k) mod N/2] on both slot rows.  With every diagonal a baby its words are the single-hoisted model's;
with a giant they differ -- the giants' ModDowns and second decompositions are not the single sum's.  Also here: the index
rules, best_baby_steps against a brute-force count, and what needs no GPU of the C ABI and the kernels."""
import ctypes as C

import numpy as np
import pytest

import lintrans_bsgs_model as bm
import lintrans_model as lm
from test_lintrans_model import _Cell, _decrypts

# name -> (diagonals, n1)
SETS = {
    "dense8": (list(range(8)), 4),
    "sparse": ([1, 6, -1], 4),  # giants without baby 0, no diagonal 0
    "giants": ([4, 8], 4),  # no baby key at all
    "every_giant": ([0, 1, 2], 1),
    "odd": ([0, 1, 2, 3, 4, 5, 7], 3),  # n1 no power of two
    "allbaby": ([0, 1, 2, 3], 64),
}
NEW_SYMBOLS = ("lumen_lintrans_load_bsgs", "lumen_lintrans_best_baby_steps")


@pytest.fixture(scope="module", params=[8, 10])
def cell(oracle, request):
    return _Cell(oracle, request.param)


@pytest.mark.parametrize("name", sorted(SETS))
def test_set_decrypts_to_the_diagonal_sum(cell, name):
    P = cell.P
    ks, n1 = SETS[name]
    values = cell.diagonals(ks)
    diags = cell.encoded(values)
    got = bm.linear_transform(P, cell.ct, diags, n1, cell.key)
    assert got.shape == cell.ct.shape and all(int(got[:, t].max()) < P.moduli[t] for t in range(3))
    _decrypts(cell, got, cell.want(values))
    single = lm.linear_transform(P, cell.ct, diags, cell.key)
    assert np.array_equal(got, single) == (name == "allbaby")


def test_the_split_and_the_elements(cell):
    P, half = cell.P, cell.P.N // 2
    pt = np.zeros((5, P.N), dtype=np.uint64)
    assert [(j, i) for j, i, _ in bm.split(P, {1: pt, 6: pt, -1: pt}, 4)] == [(0, 1), (4, 2), (half - 4, 3)]
    assert bm.babies(P, {1: pt, 6: pt, -1: pt}, 4) == [1, 2, 3] and bm.giants(P, {1: pt, 6: pt, -1: pt}, 4) == [4, half - 4]
    assert bm.elements(P, {4: pt, 8: pt}, 4) == [P.galois_element(4), P.galois_element(8)]
    assert bm.elements(P, {0: pt, 1: pt, 2: pt}, 1) == [P.galois_element(1), P.galois_element(2)]
    assert bm.elements(P, {0: pt, 5: pt, 7: pt}, 3) == [P.galois_element(x) for x in (1, 2, 3, 6)]
    assert bm.elements(P, {0: pt}, 4) == []
    assert bm.elements(P, {0: pt, 1: pt, 2: pt, 3: pt}, 64) == lm.elements(P, {1: pt, 2: pt, 3: pt})
    for bad in ({half: pt}, {-half: pt}, {1: pt, 1 - half: pt}, {}):
        with pytest.raises(ValueError):
            bm.split(P, bad, 4)
    with pytest.raises(ValueError):
        bm.split(P, {1: pt}, 0)


def _brute(log_n, ks):
    half = (1 << log_n) // 2
    costs = []
    for s in range(log_n):
        n1, bs, gs = 1 << s, set(), set()
        for k in ks:
            e = k % half
            bs.add(e % n1), gs.add(e // n1)
        costs.append((len(bs - {0}) + len(gs - {0}), n1))
    return min(costs)[1]


CASES = [(8, list(range(8))), (10, list(range(64))), (10, list(range(16))), (8, [0]), (8, [1]), (8, [1, 6, -1]), (8, [4, 8]), (14, list(range(256))),
         (10, [0, 1, 2, 3, 5]), (8, [-1, -2, -3]), (8, [127]), (15, [0, 3, 9, 27, 81, 243, 729])]


@pytest.mark.parametrize("log_n,ks", CASES)
def test_best_baby_steps(log_n, ks):
    from lumenos_amd import hip
    want = _brute(log_n, ks)
    assert bm.best_baby_steps(log_n, ks) == want
    assert want & (want - 1) == 0 and 1 <= want <= (1 << log_n) // 2
    assert hip.lintrans_best_baby_steps(log_n, ks) == want


def test_dense_sets_take_about_the_square_root():
    assert bm.best_baby_steps(14, list(range(16))) == 4 and bm.best_baby_steps(14, list(range(64))) == 8


# ------------------------------------------------------------------ the ABI and the kernels, without a GPU
def test_library_exports_and_binds_the_bsgs_form():
    from lumenos_amd import hip
    lib = hip.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in hip.SYMBOLS, n
    assert callable(hip.Context.lintrans_load) and callable(hip.lintrans_best_baby_steps)
    k = np.array([0, 1, 2, 3], dtype=np.int64)
    kp = k.ctypes.data_as(C.POINTER(C.c_int64))
    assert lib.lumen_lintrans_best_baby_steps(10, kp, 4) == 2
    assert lib.lumen_lintrans_best_baby_steps(10, None, 4) == 0
    assert lib.lumen_lintrans_best_baby_steps(10, kp, 0) == 0
    assert lib.lumen_lintrans_best_baby_steps(0, kp, 4) == 0 and lib.lumen_lintrans_best_baby_steps(40, kp, 4) == 0
    bad = np.array([0, 512], dtype=np.int64)  # outside (-N/2, N/2) at N = 2^10
    assert lib.lumen_lintrans_best_baby_steps(10, bad.ctypes.data_as(C.POINTER(C.c_int64)), 2) == 0
    h = C.c_void_p()
    assert lib.lumen_lintrans_load_bsgs(None, kp, None, 4, 3, 2, C.byref(h)) != 0
    assert "NULL argument" in lib.lumen_last_error(None).decode()


def test_bsgs_kernels_are_in_the_no_spill_report():
    from lumenos_amd import _build
    _build.build()
    hits = {k: v for k, v in _build.resource_report().items() if "k_bsgs_" in k}
    assert {n for n in ("k_bsgs_giant", "k_bsgs_plain", "k_bsgs_pt_gather") if any(n in k for k in hits)} == {"k_bsgs_giant", "k_bsgs_plain",
                                                                                                            "k_bsgs_pt_gather"}, sorted(hits)
    for k, r in hits.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (k, r)
