"""CPU: the SE(3) tests' float64 reference (tests/se3_ref.py) against 50-digit mpmath, and oracle/se3.py -- the CPU twin of
csrc/se3_device.h that every other test compares the kernels with -- against that reference at every rotation angle decade.

The decades are the point.  oracle/se3.py and the device header share one algorithm, so a weakness of the algorithm shows on both sides
and a comparison between them cannot see it: lietorch's (1 - cos theta) / theta^2 just above its Taylor guard (theta^2 = 1e-6) loses
almost all of a float32 mantissa, and the translation of se3_exp was 1.3e-4 off at 1 mrad when it was 4e-7 off everywhere else."""
import math

import pytest
import torch

import se3_ref as ref
from oracle import se3

mpmath = pytest.importorskip('mpmath')
F64 = torch.float64
N = 4000                                          # twists per decade


# ------------------------------------------------------------------------------------------------- the reference against mpmath
def _mp_twists():
    """A few dozen twists: every decade, both sides of theta^2 = 1e-6, next to pi, tau of order 1 and of order 250."""
    gen = torch.Generator().manual_seed(7)
    rows = []
    for k, a in enumerate(ref.ANGLES + (0.0, 9.999999e-4, 1.0000001e-3, 0.5 * math.pi, math.pi - 1e-9)):
        axis = ref.unit_axes(1, gen)[0]
        tau = torch.randn(3, dtype=F64, generator=gen) * (250.0 if k % 2 else 1.0)
        rows.append(torch.cat((tau, axis * a)))
    return torch.stack(rows)


def _mp_exp(xi):
    """50-digit pose of one twist: the translation from mpmath's matrix exponential of the 4x4 twist, the quaternion in closed form."""
    mp = mpmath.mp
    x = [mp.mpf(float(v)) for v in xi]
    A = mp.matrix(4, 4)
    A[0, 1], A[0, 2], A[1, 0], A[1, 2], A[2, 0], A[2, 1] = -x[5], x[4], x[5], -x[3], -x[4], x[3]
    A[0, 3], A[1, 3], A[2, 3] = x[0], x[1], x[2]
    M = mp.expm(A, method='taylor')
    th = mp.sqrt(x[3] ** 2 + x[4] ** 2 + x[5] ** 2)
    k = mp.sin(th / 2) / th if th > 0 else mp.mpf(0.5)
    return M, [M[0, 3], M[1, 3], M[2, 3], k * x[3], k * x[4], k * x[5], mp.cos(th / 2)]


def _mp_matrix(T):
    """50-digit 4x4 matrix of a pose given as 7 mpf (a unit quaternion)."""
    mp = mpmath.mp
    tx, ty, tz, x, y, z, w = T
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), tx],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x), ty],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y), tz],
                      [0, 0, 0, 1]])


def _f(v):
    return torch.tensor([float(e) for e in v], dtype=F64)


def test_reference_matches_mpmath():
    """exp, log, mul, inv and act of se3_ref agree with 50-digit arithmetic to 1e-14 of max(1, |tau|_inf, |t|_inf)."""
    xis = _mp_twists()
    old = mpmath.mp.dps
    mpmath.mp.dps = 50
    try:
        truth, mats = [], []
        for xi in xis:
            M, T = _mp_exp(xi)
            # the closed-form quaternion and the matrix exponential describe one rotation (the 50-digit side checks itself)
            assert max(abs(e) for e in (_mp_matrix(T) - M)) < mpmath.mpf(10) ** -40
            truth.append(_f(T))
            mats.append(M)
        truth = torch.stack(truth)
        scale = ref.scale_of(xis[:, :3], truth[:, :3])
        got = ref.exp(xis)
        e_t = (got[:, :3] - truth[:, :3]).abs().amax(1) / scale
        e_q = (got[:, 3:] - truth[:, 3:]).abs().amax(1)                      # both have w >= 0: no sign freedom
        e_log = (ref.log(truth) - xis).abs().amax(1) / scale
        print(f'se3_ref vs mpmath over {len(xis)} twists: exp t {e_t.max():.2e} q {e_q.max():.2e}, log {e_log.max():.2e}')
        assert e_t.max() < 1e-14 and e_q.max() < 1e-14, (e_t, e_q)
        assert e_log.max() < 1e-14, e_log
        # products, inverses and actions of neighbouring poses
        A, B = truth, truth.roll(1, 0)
        pts = torch.randn(len(xis), 5, 3, dtype=F64, generator=torch.Generator().manual_seed(8))
        mul_t, inv_t, act_t = [], [], []
        for i in range(len(xis)):
            # the float64-rounded poses are the inputs of both sides
            Ma = _mp_matrix([mpmath.mpf(float(v)) for v in A[i]])
            Mb = _mp_matrix([mpmath.mpf(float(v)) for v in B[i]])
            na = mpmath.sqrt(sum(mpmath.mpf(float(v)) ** 2 for v in A[i, 3:]))    # se3_ref normalises the rounded quaternion
            assert abs(na - 1) < 1e-15
            C, Ai = Ma * Mb, Ma ** -1
            mul_t.append(_f([C[r, c] for r in range(4) for c in range(4)]).reshape(4, 4))
            inv_t.append(_f([Ai[r, c] for r in range(4) for c in range(4)]).reshape(4, 4))
            P = [Ma * mpmath.matrix([float(p[0]), float(p[1]), float(p[2]), 1]) for p in pts[i]]
            act_t.append(torch.stack([_f([p[0], p[1], p[2]]) for p in P]))
        mul_t, inv_t, act_t = torch.stack(mul_t), torch.stack(inv_t), torch.stack(act_t)
        s2 = ref.scale_of(A[:, :3], B[:, :3])[:, None, None]
        e_mul = ((ref.to_matrix(ref.mul(A, B)) - mul_t).abs() / s2).max()
        e_inv = ((ref.to_matrix(ref.inv(A)) - inv_t).abs() / s2).max()
        e_act = ((ref.act(A, pts) - act_t).abs() / s2).max()
        print(f'se3_ref vs mpmath: mul {e_mul:.2e} inv {e_inv:.2e} act {e_act:.2e}')
        assert e_mul < 1e-14 and e_inv < 1e-14 and e_act < 1e-14, (e_mul, e_inv, e_act)
    finally:
        mpmath.mp.dps = old


def test_reference_round_trips_and_chain():
    """log(exp(xi)) = xi at every decade, and chain() is the running product of the tracker's convention."""
    for a in ref.ANGLES:
        for ts in ref.TAU_SCALES:
            xi = ref.decade_twists(a, ts, 500, F64, 11)
            T = ref.exp(xi)
            err = ((ref.log(T) - xi).abs().amax(1) / ref.scale_of(xi[:, :3], T[:, :3])).max()
            assert err < 1e-13, (a, ts, float(err))
    rel = ref.exp(ref.decade_twists(5e-3, 1e-3, 40, F64, 12))
    init = ref.exp(ref.decade_twists(0.3, 1.0, 1, F64, 13))
    out = ref.chain(rel, 250.0, init)
    P = init
    for k in range(40):
        r = rel[k:k + 1].clone()
        r[:, :3] *= 250.0
        P = ref.mul(P, ref.inv(r))
        assert (P[0] - out[k]).abs().max() < 1e-13
    assert (ref.chain(rel, 250.0)[0] - ref.inv(torch.cat((rel[:1, :3] * 250.0, rel[:1, 3:]), 1))[0]).abs().max() < 1e-13


# ------------------------------------------------------------------------------------------------- oracle/se3.py per decade
def oracle_decade_errors(dtype, tau_scale):
    """{angle: (exp error, log error)}: the largest error of oracle se3_exp (translation and quaternion) and of se3_log on the reference's
    own exp(xi), each over N twists and divided by max(1, |tau|_inf, |t|_inf) of its twist."""
    out = {}
    for a in ref.angles_for(dtype):
        xi = ref.decade_twists(a, tau_scale, N, dtype, 100)
        want = ref.exp(xi)
        got = se3.se3_exp(xi)
        scale = ref.scale_of(xi[:, :3], want[:, :3])
        e_exp = torch.maximum((got[:, :3].double() - want[:, :3]).abs().amax(1) / scale, ref.quat_err(got[:, 3:], want[:, 3:])).max()
        e_log = ((se3.se3_log(want.to(dtype)).double() - xi.double()).abs().amax(1) / scale).max()
        out[a] = (float(e_exp), float(e_log))
    return out


@pytest.mark.parametrize('tau_scale', ref.TAU_SCALES)
@pytest.mark.parametrize('dtype', (torch.float32, F64), ids=('f32', 'f64'))
def test_oracle_matches_reference_per_decade(dtype, tau_scale):
    """oracle/se3.py se3_exp and se3_log against float64 truth, one figure per rotation angle, so that one bad band cannot hide in a
    maximum over all samples.  Bars: the ones test_se3_kernels_match_oracle applies (2e-6 / 2e-5 in float32, 1e-13 / 1e-12 in float64)
    times max(1, |tau|_inf, |t|_inf).  With lietorch's (1 - cos) / theta^2 the float32 exp rows of 1.001e-3, 2e-3 and 5e-3 rad fail
    (3.3e-5, 2.3e-5, 4.7e-6 on that scale)."""
    bars = ref.BARS[dtype]
    errs = oracle_decade_errors(dtype, tau_scale)
    bad = []
    print(f'\noracle/se3.py vs float64 truth, {dtype}, tau x {tau_scale:g}: angle, exp error, log error (bars {bars["exp"]:g}, {bars["other"]:g})')
    for a, (e_exp, e_log) in errs.items():
        print(f'  {a:<22.10g} {e_exp:.2e} {e_log:.2e}')
        if not e_exp <= bars['exp']:
            bad.append(f'exp at {a:.10g} rad: {e_exp:.2e} > {bars["exp"]:g}')
        if not e_log <= bars['other']:
            bad.append(f'log at {a:.10g} rad: {e_log:.2e} > {bars["other"]:g}')
    assert not bad, '; '.join(bad)


@pytest.mark.parametrize('dtype', (torch.float32, F64), ids=('f32', 'f64'))
def test_oracle_group_ops_match_reference(dtype):
    """mul, inv and act of oracle/se3.py against the 4x4 matrix products, rotations of every size, translations of order 1 and 250."""
    bar = ref.BARS[dtype]['other']
    for ts in ref.TAU_SCALES:
        A = torch.cat([ref.exp(ref.decade_twists(a, ts, 200, F64, 200 + i)) for i, a in enumerate(ref.angles_for(dtype))]).to(dtype)
        B = A[torch.randperm(A.shape[0], generator=torch.Generator().manual_seed(3))]
        pts = torch.randn(A.shape[0], 7, 3, dtype=F64, generator=torch.Generator().manual_seed(4)).to(dtype)
        C, Cr = se3.se3_mul(A, B), ref.mul(A, B)
        s = ref.scale_of(A[:, :3], B[:, :3], Cr[:, :3])
        assert ((C[:, :3].double() - Cr[:, :3]).abs().amax(1) / s).max() <= bar
        assert ref.quat_err(C[:, 3:], Cr[:, 3:]).max() <= bar
        I, Ir = se3.se3_inv(A), ref.inv(A)
        s = ref.scale_of(A[:, :3])
        assert ((I[:, :3].double() - Ir[:, :3]).abs().amax(1) / s).max() <= bar
        assert ref.quat_err(I[:, 3:], Ir[:, 3:]).max() <= bar
        P, Pr = se3.se3_act(A[:, None], pts), ref.act(A, pts)
        assert ((P.double() - Pr).abs().amax((1, 2)) / s).max() <= bar
