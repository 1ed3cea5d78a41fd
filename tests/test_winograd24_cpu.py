"""CPU: the F(2x4,3x3) transforms of csrc/conv_wino24.hip -- F(2,3) along H, F(4,3) at the points {0, 1, -1, 1/2, -2} along W --
are exact in rational arithmetic, and an f32 model of the pipeline stays within a serial direct f32 sum's error (the numerics gate
of tools/winograd_numerics.py)."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import winograd_numerics as wn  # noqa: E402

H = Fr(1, 2)
# the matrices the kernel and its pack hard-code
BX = [[2, -3, -4, 3, 2, 0], [0, -2, 1, 5, 2, 0], [0, -2, 5, -1, -2, 0], [0, 2, 1, -2, -1, 0], [0, 1, -2, -1, 2, 0], [0, 2, -3, -4, 3, 2]]
AX = [[1, 1, 1, 1, 1, 0], [0, 1, -1, H, -2, 0], [0, 1, 1, H * H, 4, 0], [0, 1, -1, H ** 3, -8, 1]]
GX = [[H, 0, 0], [Fr(1, 6), Fr(1, 6), Fr(1, 6)], [Fr(1, 6), Fr(-1, 6), Fr(1, 6)], [Fr(16, 15), Fr(8, 15), Fr(4, 15)],
      [Fr(1, 30), Fr(-1, 15), Fr(2, 15)], [0, 0, H]]
BY = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]]
AY = [[1, 1, 1, 0], [0, 1, -1, 1]]
GY = [[1, 0, 0], [H, H, H], [H, -H, H], [0, 0, 1]]


def _mm(a, b):
    return [[sum(Fr(a[i][k]) * Fr(b[k][j]) for k in range(len(b))) for j in range(len(b[0]))] for i in range(len(a))]


def _t(a):
    return [list(r) for r in zip(*a)]


def test_matrices_are_the_numerics_tools():
    for (at, g, bt), (m, pts) in (((AX, GX, BX), (4, (0, 1, -1, H, -2))), ((AY, GY, BY), (2, (0, 1, -1)))):
        rat, rg, rbt = wn.matrices(pts, m, 3)
        assert np.array_equal(rat, np.array([[float(v) for v in r] for r in at]))
        assert np.allclose(rg, np.array([[float(v) for v in r] for r in g]), rtol=0, atol=1e-15)
        assert np.array_equal(rbt, np.array([[float(v) for v in r] for r in bt]))


def test_transforms_are_exact_in_rational_arithmetic():
    rng = np.random.default_rng(0)
    for _ in range(5):
        d = [[Fr(int(v)) for v in row] for row in rng.integers(-50, 50, size=(4, 6))]
        g = [[Fr(int(v), 7) for v in row] for row in rng.integers(-20, 20, size=(3, 3))]
        U = _mm(_mm(GY, g), _t(GX))
        V = _mm(_mm(BY, d), _t(BX))
        M = [[U[i][j] * V[i][j] for j in range(6)] for i in range(4)]
        Y = _mm(_mm(AY, M), _t(AX))
        ref = [[sum(g[a][b] * d[i + a][j + b] for a in range(3) for b in range(3)) for j in range(4)] for i in range(2)]
        assert Y == ref


def test_f32_pipeline_within_serial_direct_error():
    """The setup of the issue's table: 256-channel sums, inputs ~N(0, 2), weights ~N(0, 0.05), 60 trials."""
    ew_max, ew_mean, ed_max, ed_mean, products = wn.run_2d_mixed(2, 4, (0, 1, -1), (0, 1, -1, H, -2))
    assert products == 1.0 / 3.0
    assert ew_max <= ed_max and ew_mean < 1.5 * ed_mean, (ew_max, ed_max, ew_mean, ed_mean)
    # the rejected point set {0, +-1, +-2} is worse than the direct sum
    assert wn.run_2d_mixed(2, 4, (0, 1, -1), (0, 1, -1, 2, -2), trials=20)[0] > ew_max
