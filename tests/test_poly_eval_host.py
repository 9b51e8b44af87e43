"""The claimed value of GET /prove?point=z (cmd/server/main.go:255-258: core.NewDensePolyFromMatrix(matrix).Evaluate)
through the C++ host mirror.  CPU: core::DensePoly::Evaluate against Horner in Python integers over the row-major
flattening.  GPU: tests/cpp/test_poly_eval_host.cpp proves at a random z != 1 and holds the verifier's claim
InnerProduct(MatZ, [1, z, z^2, ...]) (fhe/ligero.go:569) to the device P(z) and the host Horner."""
import random

import numpy as np
import pytest

from helpers import twin

T = 144115188075593729  # fhe/ligero_test.go:16


def horner(coefficients, z, t=T):
    """core/poly.go:21-30 in Python integers"""
    r = 0
    for c in reversed(coefficients):
        r = (r * z + c) % t
    return r


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (512, 16), (2048, 64)])
@pytest.mark.parametrize("kind", ["random", "max"])
def test_dense_poly_evaluate_matches_python_horner(tmp_path, rows, cols, kind):
    """DensePoly::Evaluate of NewDensePolyFromMatrix(RandomMatrixRowMajor) -- and of an all-(T-1) matrix -- at
    z = 0, 1, T-1 and a random point, against Horner in Python integers over the row-major flattening."""
    points = [0, 1, T - 1, random.Random(rows * 131 + cols).randrange(2, T - 1)]
    path = tmp_path / "m.bin"
    out = twin("test_poly_eval_host", "host", rows, cols, kind, path, *points, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = np.fromfile(path, dtype=np.uint64)
    assert m.size == rows * cols and int(m.max()) < T
    if kind == "max":
        assert (m == T - 1).all()
    coeffs = [int(x) for x in m]  # coefficient i*cols + j = M[i][j]
    got = dict(tuple(int(v) for v in l.split()[1:]) for l in out.stdout.splitlines() if l.startswith("value "))
    assert sorted(got) == sorted(points)
    for z in points:
        assert got[z] == horner(coeffs, z), (rows, cols, kind, z)
    assert got[1] == sum(coeffs) % T and got[0] == coeffs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(12, 2048, 1024, 10, 2), (14, 16384, 4096, 12, 1)])
def test_claimed_value_at_a_random_point_end_to_end(shape):
    """TestLigeroE2E's shape (2048 x 1024, LogN 12; also over a ServerGroup of two ranks on the one GPU) and the
    headline one (16384 x 4096, LogN 14): encrypt on the device, Commit, Prove at a random z != 1, decrypt MatZ with
    lumen_decrypt; sum_j z^j MatZ[j] = device P(z) (whole and in uneven column blocks) = host Horner."""
    res = twin("test_poly_eval_host", "e2e", *shape, timeout=1500)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    print(res.stdout)  # the span times (device and host evaluation), shown with -s
    assert "PASS claimed value" in res.stdout
    assert "Evaluate polynomial (" in res.stdout  # the reference's span name around the device call
    if shape[4] > 1:
        assert f"PASS ServerGroup W={shape[4]}" in res.stdout
