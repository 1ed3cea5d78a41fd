"""GPU: the SE(3) kernels (rpe_se3_exp / _log / _mul / _inv / _act / _chain, rpe_pose_gate_chain, rpe_pose_gate_chain_rows) against
float64 truth (tests/se3_ref.py: 4x4 matrix exponential and matrix products, itself checked against 50-digit arithmetic in
tests/test_se3_cpu.py) -- never against oracle/se3.py, which shares the kernels' algorithm and so their weaknesses.

Errors are taken per rotation angle decade (one bad band cannot hide in a maximum over all samples) and divided by the size of the
translations involved, max(1, |tau|_inf, |t|_inf) per sample.  The bars are those of test_gpu_pose.py::test_se3_kernels_match_oracle:
float32 2e-6 for exp and 2e-5 for log / mul / inv / act, float64 1e-13 and 1e-12.

Measured on the MI355X (largest scaled error of a decade, either translation scale; the tests print the whole tables with -s):
  float32 exp  with lietorch's (1 - cos) / theta^2: 3.3e-5 at 1.001e-3 rad, 1.8e-5 at 2e-3, 4.7e-6 at 5e-3, 1.2e-6 at 1e-2, <= 5.2e-7 elsewhere;
               with the cancellation-free left Jacobian: 1.1e-7 at those decades, 3.1e-7 at worst (3 rad)
  float32 log  3.9e-7 at worst (pi - 1e-3), unchanged
  float64 exp  6.5e-14 at 1.001e-3 rad and 2.4e-14 at 2e-3 before, 1.4e-15 at worst after
  float64 log  1.0e-6 at pi - 1e-6 before (lietorch's branch for |qw| < 1e-6 returns pi itself), 2.4e-15 at worst after
No decade is within a factor 2 of its bar.
"""
import math

import pytest
import torch

import se3_ref as ref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = pytest.mark.parametrize('dtype', (F32, F64), ids=('f32', 'f64'))
N = 2048                                          # twists per decade
SENTINEL = -7.0


def _t_err(got, want, scale):
    """(n,) translation-sized error |got - want|_inf / scale."""
    return (got.double().cpu() - want).abs().amax(1) / scale


def _pose_err(got, want, scale):
    """(n,) error of (n,7) poses: the translation over scale, the quaternion as a rotation (sign-free) unscaled."""
    got = got.cpu()
    return torch.maximum(_t_err(got[:, :3], want[:, :3], scale), ref.quat_err(got[:, 3:], want[:, 3:]))


def _report(title, rows, bar):
    """rows: [(label, error)].  Prints the table and returns the rows over the bar as text."""
    print(f'\n{title} (bar {bar:g})')
    bad = []
    for label, e in rows:
        e = float(e)
        print(f'  {label:<36} {e:.2e}' + ('   within 2x of the bar' if bar / 2 < e <= bar else ''))
        if not e <= bar:
            bad.append(f'{label}: {e:.2e} > {bar:g}')
    return bad


# ------------------------------------------------------------------------------------------------- exp and log per decade
@pytest.mark.parametrize('tau_scale', ref.TAU_SCALES)
@DTYPES
def test_exp_per_decade(rpe, dtype, tau_scale):
    """se3_exp at every rotation angle decade against the matrix exponential."""
    from rpe_amd import ops
    rows = []
    for a in ref.angles_for(dtype):
        xi = ref.decade_twists(a, tau_scale, N, dtype, 1000)
        want = ref.exp(xi)
        got = ops.se3_exp(xi.cuda())
        assert got.dtype == dtype and got.shape == (N, 7)
        rows.append((f'{a:.10g} rad', _pose_err(got, want, ref.scale_of(xi[:, :3], want[:, :3])).max()))
    bad = _report(f'se3_exp vs float64 truth, {dtype}, tau x {tau_scale:g}', rows, ref.BARS[dtype]['exp'])
    assert not bad, '; '.join(bad)


@pytest.mark.parametrize('tau_scale', ref.TAU_SCALES)
@DTYPES
def test_log_per_decade(rpe, dtype, tau_scale):
    """se3_log of the REFERENCE's exp(xi) (an error of the kernel's exp cannot cancel in the kernel's log) against the twist xi."""
    from rpe_amd import ops
    rows = []
    for a in ref.angles_for(dtype):
        xi = ref.decade_twists(a, tau_scale, N, dtype, 2000)
        T = ref.exp(xi)
        got = ops.se3_log(T.to(dtype).cuda())
        rows.append((f'{a:.10g} rad', _t_err(got, xi.double(), ref.scale_of(xi[:, :3], T[:, :3])).max()))
    bad = _report(f'se3_log(exp_ref(xi)) vs xi, {dtype}, tau x {tau_scale:g}', rows, ref.BARS[dtype]['other'])
    assert not bad, '; '.join(bad)


# ------------------------------------------------------------------------------------------------- both sides of every guard
@DTYPES
def test_both_sides_of_the_taylor_guard(rpe, dtype):
    """theta^2 just below and just above 1e-6 (so3_exp, left_jacobian_mul, left_jacobian_inv_mul switch between series and closed form
    there), as close as the dtype resolves: |phi| = 1e-3 (1 -+ 16 eps)."""
    from rpe_amd import ops
    eps = torch.finfo(dtype).eps
    rows_e, rows_l = [], []
    for side, a in (('below', 1e-3 * (1 - 16 * eps)), ('above', 1e-3 * (1 + 16 * eps))):
        for ts in ref.TAU_SCALES:
            xi = ref.decade_twists(a, ts, N, dtype, 3000)
            th2 = (xi[:, 3:] * xi[:, 3:]).sum(1)                                  # in dtype, as the kernel forms it
            assert bool((th2 < 1e-6).all()) if side == 'below' else bool((th2 >= 1e-6).all()), side
            want = ref.exp(xi)
            scale = ref.scale_of(xi[:, :3], want[:, :3])
            rows_e.append((f'exp {side}, tau x {ts:g}', _pose_err(ops.se3_exp(xi.cuda()), want, scale).max()))
            rows_l.append((f'log {side}, tau x {ts:g}', _t_err(ops.se3_log(want.to(dtype).cuda()), xi.double(), scale).max()))
    bad = _report(f'theta^2 = 1e-6 guard, {dtype}', rows_e, ref.BARS[dtype]['exp'])
    bad += _report(f'theta^2 = 1e-6 guard, {dtype}', rows_l, ref.BARS[dtype]['other'])
    assert not bad, '; '.join(bad)


def _quat_poses(nv, w_sign, n, ts, dtype, seed, w=None):
    """n poses whose quaternion has |qv| = nv about random axes and qw = w_sign * sqrt(1 - nv^2), or qv of norm sqrt(1 - w^2) and the
    given qw; t ~ N(0,1) * ts.  Rounded to dtype."""
    gen = torch.Generator().manual_seed(seed)
    axes = ref.unit_axes(n, gen)
    if w is None:
        w = w_sign * math.sqrt(1.0 - nv * nv)
    else:
        nv = math.sqrt(1.0 - w * w)
    t = torch.randn(n, 3, dtype=F64, generator=gen) * ts
    return torch.cat((t, axes * nv, torch.full((n, 1), w, dtype=F64)), dim=1).to(dtype)


@DTYPES
def test_log_guards(rpe, dtype):
    """so3_log's branches, both sides of each: |qv|^2 < 1e-12 (series in |qv|^2), |qw| < 1e-6 (a rotation next to pi, both signs of qw),
    qw < 0 (the quaternion of the long way round: the logarithm is the short rotation vector, |phi| <= pi).  Truth is the reference's log
    of the very pose the kernel was given.  At qw = 0 exactly, +pi and -pi about the axis are one rotation: either twist is accepted."""
    from rpe_amd import ops
    cases = []
    for ts in ref.TAU_SCALES:
        for sign in (1.0, -1.0):
            s = '+' if sign > 0 else '-'
            cases += [(f'|qv| 0.9e-6 qw {s}, t x {ts:g}', _quat_poses(0.9e-6, sign, 512, ts, dtype, 4000)),
                      (f'|qv| 1.1e-6 qw {s}, t x {ts:g}', _quat_poses(1.1e-6, sign, 512, ts, dtype, 4001)),
                      (f'|qv| 1e-9 qw {s}, t x {ts:g}', _quat_poses(1e-9, sign, 512, ts, dtype, 4002)),
                      (f'qw {s}5e-7, t x {ts:g}', _quat_poses(0, 0, 512, ts, dtype, 4003, w=sign * 5e-7)),
                      (f'qw {s}0.99e-6, t x {ts:g}', _quat_poses(0, 0, 512, ts, dtype, 4004, w=sign * 0.99e-6)),
                      (f'qw {s}1.01e-6, t x {ts:g}', _quat_poses(0, 0, 512, ts, dtype, 4005, w=sign * 1.01e-6)),
                      (f'qw {s}1e-3, t x {ts:g}', _quat_poses(0, 0, 512, ts, dtype, 4006, w=sign * 1e-3)),
                      (f'qw {s}0.5 (theta 2pi/3), t x {ts:g}', _quat_poses(0, 0, 512, ts, dtype, 4007, w=sign * 0.5))]
        cases.append((f'qw 0, t x {ts:g}', _quat_poses(0, 0, 512, ts, dtype, 4008, w=0.0)))
    rows = []
    for label, T in cases:
        got = ops.se3_log(T.cuda())
        wants = [ref.log(T)]
        if label.startswith('qw 0,'):
            wants.append(ref.log(torch.cat((T[:, :3], -T[:, 3:6], T[:, 6:]), dim=1)))
        errs = [_t_err(got, want, ref.scale_of(T[:, :3], want[:, :3])) for want in wants]
        assert bool((got[:, 3:].double().norm(dim=1) <= math.pi * (1 + 4 * torch.finfo(dtype).eps)).all()), label   # the short way
        rows.append((label, torch.stack(errs).amin(0).max()))
    bad = _report(f'se3_log branch guards vs float64 truth, {dtype}', rows, ref.BARS[dtype]['other'])
    assert not bad, '; '.join(bad)


# ------------------------------------------------------------------------------------------------- mul, inv, act and the group laws
def _mixed_poses(dtype, ts, per, seed):
    """Poses of every rotation size (per of each angle of the decade list), translations ~ N(0,1) * ts, rounded to dtype."""
    return torch.cat([ref.exp(ref.decade_twists(a, ts, per, F64, seed + i)) for i, a in enumerate(ref.angles_for(dtype))]).to(dtype)


@DTYPES
def test_mul_inv_act_match_matrix_products(rpe, dtype):
    """se3_mul, se3_inv and se3_act against 4x4 matrix products, and the group laws against the reference's values (not merely
    against each other): mul(T, inv(T)) = identity, act(mul(A, B), p) = act(A, act(B, p)), inv(inv(T)) = T."""
    from rpe_amd import ops
    bar = ref.BARS[dtype]['other']
    rows = []
    for ts in ref.TAU_SCALES:
        A = _mixed_poses(dtype, ts, 256, 5000)
        n = A.shape[0]
        B = A[torch.randperm(n, generator=torch.Generator().manual_seed(5))]
        pts = torch.randn(n, 33, 3, dtype=F64, generator=torch.Generator().manual_seed(6)).to(dtype)
        Ag, Bg, pg = A.cuda(), B.cuda(), pts.cuda()
        sA = ref.scale_of(A[:, :3])
        sAB = ref.scale_of(A[:, :3], B[:, :3])
        rows.append((f'mul, t x {ts:g}', _pose_err(ops.se3_mul(Ag, Bg), ref.mul(A, B), sAB).max()))
        rows.append((f'inv, t x {ts:g}', _pose_err(ops.se3_inv(Ag), ref.inv(A), sA).max()))
        rows.append((f'act, t x {ts:g}', ((ops.se3_act(Ag, pg).double().cpu() - ref.act(A, pts)).abs().amax((1, 2)) / sA).max()))
        # group laws
        Ai = ops.se3_inv(Ag)
        ident = torch.zeros(n, 7, dtype=F64)
        ident[:, 6] = 1.0
        E = ops.se3_mul(Ag, Ai)
        rows.append((f'mul(T, inv T) vs ref, t x {ts:g}', _pose_err(E, ref.mul(A, ref.inv(A)), sA).max()))
        rows.append((f'mul(T, inv T) vs identity, t x {ts:g}', _pose_err(E, ident, sA).max()))
        lhs = ops.se3_act(ops.se3_mul(Ag, Bg), pg)
        rhs = ops.se3_act(Ag, ops.se3_act(Bg, pg))
        want = ref.act(A, ref.act(B, pts))
        rows.append((f'act(mul(A, B), p), t x {ts:g}', ((lhs.double().cpu() - want).abs().amax((1, 2)) / sAB).max()))
        rows.append((f'act(A, act(B, p)), t x {ts:g}', ((rhs.double().cpu() - want).abs().amax((1, 2)) / sAB).max()))
        II = ops.se3_inv(Ai)
        rows.append((f'inv(inv T) vs ref, t x {ts:g}', _pose_err(II, ref.inv(ref.inv(A)), sA).max()))
        rows.append((f'inv(inv T) vs T, t x {ts:g}', _pose_err(II, A.double(), sA).max()))
    bad = _report(f'mul / inv / act and group laws vs float64 truth, {dtype}', rows, bar)
    assert not bad, '; '.join(bad)


# ------------------------------------------------------------------------------------------------- launch shapes
def _padded_out(n_out, dtype):
    """A sentinel-filled buffer with room for n_out values in its middle: (buffer, the middle as a view, pad)."""
    pad = 97
    buf = torch.full((n_out + 2 * pad,), SENTINEL, dtype=dtype, device='cuda')
    return buf, buf[pad:pad + n_out], pad


def _untouched(buf, pad):
    return bool((buf[:pad] == SENTINEL).all()) and bool((buf[-pad:] == SENTINEL).all())


@pytest.mark.parametrize('n', (1, 63, 64, 65, 255, 257, 100003))
@DTYPES
def test_launch_shapes_unary_and_mul(rpe, dtype, n):
    """n on both sides of the wave (64) and workgroup (256) sizes and far above: every row computed, nothing written beside the n rows
    (the outputs sit in the middle of a sentinel-filled buffer).  Through the C ABI directly, since the wrappers allocate their outputs."""
    from rpe_amd import _lib, ops
    L, dt = _lib.lib(), ops._DT[dtype]
    xi = ref.decade_twists(5e-3, 1.0, n, F64, 6000 + n)
    xi[: n // 2, 3:] *= 200.0                                                      # half of the rows at 1 rad
    xi = xi.to(dtype)
    T = ref.exp(xi).to(dtype)
    B = T.flip(0).contiguous()
    xg, Tg, Bg = xi.cuda(), T.cuda(), B.cuda()
    bars = ref.BARS[dtype]
    sT = ref.scale_of(xi[:, :3], T[:, :3])

    buf, out, pad = _padded_out(n * 7, dtype)
    _lib.check(L.rpe_se3_exp(_lib.ptr(xg), _lib.ptr(out), n, dt, _lib.stream_ptr()), 'rpe_se3_exp')
    assert _untouched(buf, pad)
    assert _pose_err(out.reshape(n, 7), ref.exp(xi), sT).max() <= bars['exp']

    buf, out, pad = _padded_out(n * 6, dtype)
    _lib.check(L.rpe_se3_log(_lib.ptr(Tg), _lib.ptr(out), n, dt, _lib.stream_ptr()), 'rpe_se3_log')
    assert _untouched(buf, pad)
    assert _t_err(out.reshape(n, 6), ref.log(T), sT).max() <= bars['other']

    buf, out, pad = _padded_out(n * 7, dtype)
    _lib.check(L.rpe_se3_inv(_lib.ptr(Tg), _lib.ptr(out), n, dt, _lib.stream_ptr()), 'rpe_se3_inv')
    assert _untouched(buf, pad)
    assert _pose_err(out.reshape(n, 7), ref.inv(T), sT).max() <= bars['other']

    buf, out, pad = _padded_out(n * 7, dtype)
    _lib.check(L.rpe_se3_mul(_lib.ptr(Tg), _lib.ptr(Bg), _lib.ptr(out), n, dt, _lib.stream_ptr()), 'rpe_se3_mul')
    assert _untouched(buf, pad)
    assert _pose_err(out.reshape(n, 7), ref.mul(T, B), ref.scale_of(T[:, :3], B[:, :3])).max() <= bars['other']


@pytest.mark.parametrize('m', (1, 33, 900, 4097))
@pytest.mark.parametrize('n', (1, 3, 65))
@DTYPES
def test_launch_shapes_act(rpe, dtype, n, m):
    """se3_act on (n, m, 3) points: point i takes pose i // m; nothing written beside the n * m points."""
    from rpe_amd import _lib, ops
    L, dt = _lib.lib(), ops._DT[dtype]
    T = ref.exp(ref.decade_twists(0.7, 1.0, n, F64, 7000 + n)).to(dtype)
    pts = torch.randn(n, m, 3, dtype=F64, generator=torch.Generator().manual_seed(7100 + m)).to(dtype)
    Tg, pg = T.cuda(), pts.cuda()
    buf, out, pad = _padded_out(n * m * 3, dtype)
    _lib.check(L.rpe_se3_act(_lib.ptr(Tg), _lib.ptr(pg), _lib.ptr(out), n, m, dt, _lib.stream_ptr()), 'rpe_se3_act')
    assert _untouched(buf, pad)
    err = (out.reshape(n, m, 3).double().cpu() - ref.act(T, pts)).abs().amax((1, 2)) / ref.scale_of(T[:, :3])
    assert err.max() <= ref.BARS[dtype]['other']
    assert torch.equal(ops.se3_act(Tg, pg), out.reshape(n, m, 3))                   # the wrapper is the same launch


# ------------------------------------------------------------------------------------------------- chain and gate
CHAIN_M = 3000
CHAIN_SCALE = 250.0


def _tracker_rel(dtype, seed=8000):
    """3000 frame-to-frame motions of a tracker: rotations of a few milliradians, translations of a few millimetres in units of the
    depth scale (times 250 they are of order 1)."""
    gen = torch.Generator().manual_seed(seed)
    xi = torch.cat((torch.randn(CHAIN_M, 3, dtype=F64, generator=gen) * 2e-3, torch.randn(CHAIN_M, 3, dtype=F64, generator=gen) * 3e-3), dim=1)
    xi[:, 2] += 2e-3                                                              # a steady advance along z besides the jitter
    return ref.exp(xi).to(dtype)


def _chain_errors(got, want):
    """(m,) error of chained poses: translation over max(1, largest |t| so far), quaternion sign-free."""
    scale = torch.cummax(want[:, :3].abs().amax(1).clamp(min=1.0), dim=0).values
    return _pose_err(got, want, scale)


@DTYPES
def test_chain_against_float64_running_product(rpe, dtype):
    """rpe_se3_chain over 3000 relative poses of a few milliradians and millimetres (translation scale 250, |t| reaches 1480) against the
    float64 running product of 4x4 matrices.  A chain of m poses may drift m per-pose bars; measured on the MI355X the largest error of any
    pose, over the largest |t| so far, is 1.7e-6 in float32 (3.5e-6 through the gate kernel, whose chain starts from a pose) and 2.7e-15 /
    6.2e-15 in float64: the rounding errors of the steps do not add up in one direction, and the translation they are measured against grows
    with the chain.  So the bar is ONE per-pose bar (2e-5, 1e-12) for every pose of the chain, 5.6 times the measured float32 drift."""
    from rpe_amd import ops
    rel = _tracker_rel(dtype)
    want = ref.chain(rel, CHAIN_SCALE)
    got = ops.se3_chain(rel.cuda(), scale=CHAIN_SCALE)
    err = _chain_errors(got, want)
    bar = ref.BARS[dtype]['other']
    print(f'\nse3_chain {dtype}: scaled error at pose 10 / 100 / 1000 / 3000 = {err[9]:.2e} / {err[99]:.2e} / {err[999]:.2e} / {err[-1]:.2e}, '
          f'largest {err.max():.2e}; |t| reaches {want[:, :3].abs().max():.1f}')
    assert err.max() <= bar, (int(err.argmax()), float(err.max()))
    # with an initial pose
    init = ref.exp(ref.decade_twists(0.4, 3.0, 1, F64, 8001)).to(dtype)
    got = ops.se3_chain(rel[:200].cuda(), scale=CHAIN_SCALE, init=init.cuda())
    err = _chain_errors(got, ref.chain(rel[:200], CHAIN_SCALE, init))
    assert err.max() <= bar, float(err.max())


@DTYPES
def test_gate_chain_against_truth_and_step_by_step(rpe, dtype):
    """rpe_pose_gate_chain over the same 3000 poses, some of them over the gate (|log| > 0.1) or NaN: the flags are those float64 truth
    gives (no row sits near the threshold), the absolute poses follow the float64 running product of the gated poses, and -- as
    include/rpe.h promises -- every bit equals rpe_se3_log / _inv / _mul applied step by step."""
    from rpe_amd import ops
    rel = _tracker_rel(dtype)
    big = ref.exp(ref.decade_twists(0.3, 0.01, 3, F64, 8002)).to(dtype)
    rel[100], rel[1500], rel[2999] = big[0], big[1], big[2]
    rel[777, 1] = float('nan')
    rel[2000, 6] = float('nan')
    init = ref.exp(ref.decade_twists(0.4, 3.0, 1, F64, 8003)).to(dtype)
    thr = 0.1
    got_rel, got_abs, ok = ops.pose_gate_chain(rel.cuda(), init.cuda(), CHAIN_SCALE, thr)
    # truth
    nan = torch.isnan(rel).any(1)
    lg = ref.log(torch.where(nan[:, None], torch.tensor([0, 0, 0, 0, 0, 0, 1.0], dtype=dtype), rel))
    bad = nan | (lg.abs() > thr).any(1)
    assert sorted(bad.nonzero()[:, 0].tolist()) == [100, 777, 1500, 2000, 2999]
    assert float((lg.abs().amax(1) - thr).abs().min()) > 1e-3                            # nothing near the threshold: the flags are not a rounding matter
    assert ok.cpu().tolist() == (~bad).int().tolist()
    gated = rel.clone()
    gated[bad] = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], dtype=dtype)
    assert torch.equal(got_rel.cpu(), gated)
    err = _chain_errors(got_abs, ref.chain(gated, CHAIN_SCALE, init))
    bar = ref.BARS[dtype]['other']                                                 # see test_chain_against_float64_running_product
    print(f'\npose_gate_chain {dtype}: largest scaled error {err.max():.2e}, at the last pose {err[-1]:.2e}')
    assert err.max() <= bar, float(err.max())
    # step by step with the separate kernels: bit for bit
    relg = rel.cuda()
    ident = torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]], dtype=dtype, device='cuda')
    logs = ops.se3_log(relg)
    bad_k = (torch.isnan(relg).any(1) | (logs.abs() > thr).any(1)).cpu().tolist()
    assert bad_k == bad.tolist()
    P = init.cuda()
    s = torch.tensor(CHAIN_SCALE, dtype=dtype, device='cuda')
    steps = []
    for k in range(CHAIN_M):
        r = ident if bad_k[k] else relg[k:k + 1]
        r = torch.cat((r[:, :3] * s, r[:, 3:]), dim=1)
        P = ops.se3_mul(P, ops.se3_inv(r))
        steps.append(P)
    assert torch.equal(got_abs, torch.cat(steps))
    # the chain kernel without the gate gives the same bits on the gated poses
    assert torch.equal(ops.se3_chain(got_rel, scale=CHAIN_SCALE, init=init.cuda()), got_abs)


@DTYPES
def test_gate_chain_rows_against_truth_and_step_by_step(rpe, dtype):
    """rpe_pose_gate_chain_rows: m independent rows, row k onto its own initial pose.  Against float64 truth (one inverse and one product
    per row), bit-identical to log / inv / mul row-wise and to rpe_pose_gate_chain with m = 1, for m on both sides of the wave size."""
    from rpe_amd import ops
    thr = 0.1
    for m in (1, 63, 64, 65, 257, 3000):
        rel = _tracker_rel(dtype, 8100 + m)[:m].clone()
        if m > 2:
            rel[m // 2] = ref.exp(ref.decade_twists(0.3, 0.01, 1, F64, 8200)).to(dtype)[0]
            rel[m - 1, 3] = float('nan')
        init = ref.exp(ref.decade_twists(1.0, 3.0, m, F64, 8300 + m)).to(dtype)
        got_rel, got_abs, ok = ops.pose_gate_chain_rows(rel.cuda(), init.cuda(), CHAIN_SCALE, thr)
        nan = torch.isnan(rel).any(1)
        identity = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], dtype=dtype)
        lg = ref.log(torch.where(nan[:, None], identity, rel))
        bad = nan | (lg.abs() > thr).any(1)
        assert ok.cpu().tolist() == (~bad).int().tolist()
        assert int(bad.sum()) == (2 if m > 2 else 0)
        gated = rel.clone()
        gated[bad] = identity
        assert torch.equal(got_rel.cpu(), gated)
        scaled = torch.cat((gated[:, :3].double() * CHAIN_SCALE, gated[:, 3:].double()), dim=1)
        want = ref.mul(init, ref.inv(scaled))
        err = _pose_err(got_abs, want, ref.scale_of(init[:, :3], scaled[:, :3], want[:, :3]))
        assert err.max() <= ref.BARS[dtype]['other'], (m, float(err.max()))
        # the separate kernels, row-wise
        g = gated.cuda()
        s = torch.tensor(CHAIN_SCALE, dtype=dtype, device='cuda')
        step = ops.se3_mul(init.cuda(), ops.se3_inv(torch.cat((g[:, :3] * s, g[:, 3:]), dim=1)))
        assert torch.equal(got_abs, step)
        for k in sorted({0, m // 2, m - 1}):
            r1, a1, ok1 = ops.pose_gate_chain(rel[k:k + 1].cuda(), init[k].cuda(), CHAIN_SCALE, thr)
            assert torch.equal(r1[0], got_rel[k]) and torch.equal(a1[0], got_abs[k]) and int(ok1[0]) == int(ok[k])
