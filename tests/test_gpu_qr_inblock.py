"""R-only QR of the workgroup engine on shapes that take the four-panel (quad) path - the panel, Gram and in-block tile
update passes of wg::qr_r: R^T R must reproduce A^T A (rank deficiency and 1e-150 columns included), and the sign-free
summary of R (|diag R| and the row norms of R) of full-rank inputs must match tests/golden/qr_inblock_parent.npz, written
by this kernel from the same inputs - a reorganisation of the in-block passes must leave R unchanged to rounding."""
import ctypes as C
import os

import numpy as np
import pytest

import mpbp_amd

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qr_inblock_parent.npz")

# quad path: rows - j0 <= 2048 for the register panel, j0 + 64 <= min(rows, cols) and a trailing matrix behind
SHAPES = [(1600, 400), (700, 208), (2048, 130), (500, 500), (300, 320), (1600, 80)]
VARIANTS = ["random", "rank_deficient", "tiny_columns"]


def inputs(rows, cols, variant):
    rng = np.random.default_rng(rows * 7919 + cols)
    A = np.asfortranarray(rng.standard_normal((rows, cols)))
    if variant == "rank_deficient":
        # exact dependences inside one panel, across the panels of one quad and across quads
        A[:, 3] = 2.0 * A[:, 1]
        A[:, 40] = A[:, 20] - A[:, 33]
        A[:, 70] = A[:, 5] + 0.5 * A[:, 60]
    elif variant == "tiny_columns":
        # 1e-150 columns in panel b, c and d of the first quad and a whole tiny panel in the second
        for j in (17, 36, 50, 51):
            A[:, j] *= 1e-150
        A[:, 64:80] *= 1e-150
    return A


def summary(R):
    return np.abs(np.diag(R)), np.sqrt((R * R).sum(axis=1))


def qr_r(A):
    rows, cols = A.shape
    R = np.zeros((min(rows, cols), cols), order="F")
    rc = mpbp_amd._lib.lib().mpbp_selftest_qr(0, rows, cols, A.ctypes.data_as(C.POINTER(C.c_double)),
                                              R.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0 and np.isfinite(R).all()
    return R


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_qr_inblock_gram(rows, cols, variant):
    A = inputs(rows, cols, variant)
    R = qr_r(A)
    G = A.T @ A
    assert np.abs(R.T @ R - G).max() <= 1e-12 * np.abs(G).max()


# not "rank_deficient": the reflector of a dependent column is built from rounding noise, and so are the rows of R
# it touches - only R^T R is defined there
@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("variant", ["random", "tiny_columns"])
def test_qr_inblock_matches_parent(rows, cols, variant):
    A = inputs(rows, cols, variant)
    d, n = summary(qr_r(A))
    ref = np.load(GOLDEN)
    d0, n0 = ref[f"{rows}x{cols}_{variant}_diag"], ref[f"{rows}x{cols}_{variant}_rownorm"]
    scale = n0.max()
    assert np.abs(d - d0).max() <= 1e-10 * scale
    assert np.abs(n - n0).max() <= 1e-10 * scale
