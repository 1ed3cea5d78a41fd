"""GPU: the pose layer's backward kernels (csrc/pose_backward.hip: k_bwd_moments + k_bwd_finish, k_bwd_grads) and the forward reduce
(csrc/pose.hip) at their edges, through ops.pose_backward_moments / pose_backward_grads / pose_reduce with T and u given, against the
float64 autograd truth of tests/pose_grad_truth.py -- which shares no algebra with the kernels or with oracle/pose_grad.py and is pinned
to the reference's own autograd results by tests/test_pose_grad_truth_cpu.py.

Bars.  Moments (float64 from float64 arithmetic): 1e-9 of the row's max |H|, and of max |g| for g2u and g3u.  Per-pixel gradients (float32
casts of float64 arithmetic), every element: |got - truth| <= 2^-23 |truth| + floor, floor = ten times the float64 disagreement of the two
CPU evaluations (pose_grad_truth.F64_DISAGREEMENT: flow 1.3e-14, pcl1 1.1e-14, pcl2 1.9e-15, w1 3.7e-11, w2 1.2e-11) times the PIXEL's own largest
|gradient| -- so a clamped pixel, 1e20 times its neighbours, is held to its own size and they to theirs.  Forward reduce: 1e-11 relative.

Non-finite inputs: see ``test_nonfinite_inputs`` for the two places where the kernels' values are pinned and not the autograd result."""
import warnings

import pytest
import torch

import pose_grad_truth as pt

pytestmark = pytest.mark.gpu
ALL = list(pt.GRADS)
FINITE = [k for k in pt.CASES if k != 'nonfinite']


def _rowmax(t):
    return t.reshape(t.shape[0], -1).abs().amax(1)


def _moments_ok(got, want, label):
    """1e-9 of the row's largest |want|, row by row."""
    got = got.cpu()
    d, s = _rowmax(got - want), _rowmax(want)
    print(label, 'worst row: %.2e of its max' % float(torch.where(s > 0, d / s, d).max()))
    assert not bool(torch.isnan(got).any()) and bool((d <= 1e-9 * s).all()), label


def _run(c, want=ALL):
    from rpe_amd import ops
    dargs = [a.cuda() for a in pt.args_of(c)]
    T, u = c['T'].cuda(), c['u'].cuda()
    return ops.pose_backward_moments(*dargs, T), ops.pose_backward_grads(*dargs, T, u, want), dargs


def _check_grads(got, t, label, rows=slice(None), keep=None):
    for k in ALL:
        want = pt.nan_rule(t['g_' + k])[rows]
        g = got[k][rows]
        assert g.dtype == torch.float32 and g.shape == want.shape, (label, k)
        if keep is not None:
            g, want = torch.where(keep[rows], g.cpu(), torch.zeros_like(g.cpu())), torch.where(keep[rows], want, torch.zeros_like(want))
        miss = pt.pixel_misses(g, want, k)
        s = pt.pixel_scale(want)
        print(label, k, 'worst element: %.2e of its pixel' % float(((g.cpu().double() - want).abs() / torch.where(s > 0, s, torch.ones_like(s))).max()))
        assert miss == 0, (label, k, miss)


@pytest.mark.parametrize('name', FINITE)
def test_moments_and_grads_match_autograd(rpe, name):
    """Large motion and general K (also K[1,0] and K's last row), loss weights (0.3, 2) and (1, 0); the strict image bounds from both
    sides, the four mask combinations, zero weights; the depth clamp with a_z < 0 and a_z == 0, gated in and out; every shape class of
    the two launches (1x1, h w < 64, 255 / 258, 1023 / 1025, odd widths, 3 x 33x41 with more than one block per row, 1025 rows of 2x3).
    That each class is present in its case is asserted on the host (test_pose_grad_truth_cpu.py::test_every_planted_class_is_present);
    the zero-weight gradients are asserted non-zero here as well."""
    c, t = pt.case(name)
    (g2u, g3u, H), got, _ = _run(c)
    _moments_ok(g2u, t['g2u'], name + ' g2u')
    _moments_ok(g3u, t['g3u'], name + ' g3u')
    _moments_ok(H, t['H'], name + ' H')
    assert torch.equal(H, H.transpose(1, 2))
    _check_grads(got, t, name)
    if name == 'gates':
        P = c['planted']
        assert all(float(got['w1'][r, 0, y, x]) != 0.0 for r, y, x in P['w1_zero'] + P['w12_zero'])
        assert all(float(got['w2'][r, 0, y, x]) != 0.0 for r, y, x in P['w2_zero'] + P['w12_zero'])
        for nm in ('fx_on_0', 'fx_on_W', 'fy_on_0', 'fy_on_H'):
            assert all(float(got['flow'][r, :, y, x].abs().max()) == 0.0 and float(got['w1'][r, 0, y, x]) == 0.0 for r, y, x in P[nm]), nm
        for nm in ('fx_inside_0', 'fx_inside_W', 'fy_inside_0', 'fy_inside_H'):
            assert all(float(got['flow'][r, :, y, x].abs().min()) > 0.0 for r, y, x in P[nm]), nm


@pytest.mark.parametrize('name', ['motion', 'clamp', 'gates'])
def test_forward_reduce_matches_autograd(rpe, name):
    """ops.pose_reduce: f and the unclipped tangent gradient against the truth's f and fY -- general K, poses far from identity and from
    the solution, clamped depths (g relative to the larger of its two terms' gradients, which cancel in fY near a solution)."""
    from rpe_amd import ops
    c, t = pt.case(name)
    out = ops.pose_reduce(*[a.cuda() for a in pt.args_of(c)], c['T'].cuda())
    f, g = out['f'].cpu(), out['g'].cpu()
    lw = c['loss_weight'].double()
    scale = torch.maximum(_rowmax(t['g2u']) * lw[:, 1], _rowmax(t['g3u']) * lw[:, 0])
    print(name, 'f %.2e g %.2e' % (float(((f - t['f']).abs() / t['f'].abs()).max()), float((_rowmax(g - t['fY']) / scale).max())))
    assert bool(((f - t['f']).abs() <= 1e-11 * t['f'].abs()).all())
    assert bool((_rowmax(g - t['fY']) <= 1e-11 * scale).all())


def test_any_subset_of_outputs_has_the_same_bits(rpe):
    from rpe_amd import ops
    c, _ = pt.case('gates')
    _, full, dargs = _run(c)
    T, u = c['T'].cuda(), c['u'].cuda()
    for bits in range(1, 31):
        want = [k for i, k in enumerate(ALL) if bits >> i & 1]
        got = ops.pose_backward_grads(*dargs, T, u, want)
        assert list(got) == want and all(torch.equal(got[k], full[k]) for k in want), want


def test_nonfinite_inputs(rpe):
    """NaN and inf in each of flow, w1, pcl2, w2, gated in and gated out, one per row (pose_grad_truth.case_nonfinite, 16 rows).
    Autograd (the reference: 0 * NaN = NaN) has a NaN in fY in every such row, so the reference's backward fails its optimality check and
    returns zeros with a warning; its per-pixel gradients are NaN throughout such a row, zeros after the NaN -> 0 rule.  The kernels:
      * w1, pcl2, w2 not finite (rows 4..15): g2u resp. g3u and H are not finite in exactly the rows where the truth's are not -- the same
        outcome, since the optimality check fails on any NaN or inf.  Entry by entry the kernels' pattern is pinned
        (``pt.MOMENT_ENTRIES``): their sums keep a NaN in one coordinate of pcl2 to the entries that coordinate enters, and an inf stays an
        inf, where autograd's matrix products spread NaN over all six.
      * flow not finite (rows 0..3): PINNED DEVIATION.  The kernels cut a non-finite 2D residual off by selection (``bad ? 0.0 : ...``), so
        their moments and gradients are finite: those of the same input with that pixel's flow outside the image (``pt.sanitised``),
        checked at the full bars at every pixel.
      * at the planted pixel of rows 4..15: PINNED VALUES (``pt.PLANTED_PIXEL``), element by element against the closed forms of
        oracle/pose_grad.py: zeros after the rule or the pixel's other, finite term -- and +-inf in grad_pcl1 / grad_w2 for an inf in pcl2,
        in grad_pcl2 for an inf in w2, at an open 3D gate: SECOND PINNED DEVIATION (the reference's value after its rule is 0; inf is not
        NaN, so ``nan0`` lets it through).  No NaN anywhere.  Away from the planted pixel every row is the finite truth of ``sanitised``
        (a pixel's gradient does not depend on another pixel once T and u are given).
      * neither deviation reaches the layer's output.  ``DeclarativeLayerLie`` is run on each of the 16 rows alone: its forward multiplies
        the NaN or inf into the pose like autograd does, and its backward warns and returns zeros; the truth at the returned pose says
        the same (``reference_returns_zeros``)."""
    from oracle import pose_grad
    from rpe_amd import pose_head as ph
    c, t = pt.case('nonfinite')
    s = pt.sanitised(c)
    ts = pt.truth(pt.args_of(s), s['T'], s['u'])
    (g2u, g3u, H), got, dargs = _run(c)
    g2u, g3u, H = g2u.cpu(), g3u.cpu(), H.cpu()
    rows = lambda m: (~torch.isfinite(m)).reshape(16, -1).any(1).tolist()
    assert rows(g2u)[4:] == rows(t['g2u'])[4:] == [True] * 4 + [False] * 8 and rows(g3u) == rows(t['g3u']) == [False] * 8 + [True] * 8
    assert rows(H) == [False] * 4 + rows(t['H'])[4:] == [False] * 4 + [True] * 12
    for r, name in enumerate(pt.NONFINITE):
        want = pt.MOMENT_ENTRIES[name]
        assert pt.classes(g2u[r], want[:6]) + ' ' + pt.classes(g3u[r], want[7:]) == want, name
    _moments_ok(g2u[pt.FLOW_ROWS], ts['g2u'][pt.FLOW_ROWS], 'flow rows g2u')
    _moments_ok(g3u[pt.FLOW_ROWS], ts['g3u'][pt.FLOW_ROWS], 'flow rows g3u')
    _moments_ok(H[pt.FLOW_ROWS], ts['H'][pt.FLOW_ROWS], 'flow rows H')
    assert all(not bool(torch.isnan(v).any()) for v in got.values())
    _check_grads(got, ts, 'flow rows', rows=pt.FLOW_ROWS)
    planted = pt.planted_mask(c)
    _check_grads(got, ts, 'away from the planted pixel', keep=~planted)
    assert pt.planted_classes(got, c) == pt.PLANTED_PIXEL
    closed, _, _ = pose_grad.layer_backward(*pt.args_of(c), c['T'], None, u=c['u'])
    _check_grads(got, {'g_' + k: v for k, v in closed.items()}, 'the planted pixel', keep=planted)
    # the layer, row by row: warning and zeros, and the truth at the returned pose says the same
    layer = ph.DeclarativeLayerLie(ph.DPoseSE3Head(None, lbgfs_iters=100))
    for r, name in enumerate(pt.NONFINITE):
        xs = [a[r:r + 1].clone() for a in dargs]
        for i in (0, 1, 2, 3, 4, 8):
            xs[i].requires_grad_(True)
        vec7, log6 = layer(*xs)
        with pytest.warns(UserWarning, match='Non-zero objective'):
            log6.sum().backward()
        assert all(float(xs[i].grad.abs().max()) == 0.0 for i in (0, 1, 2, 3, 4, 8)), name
        at_pose = pt.truth([a[r:r + 1] for a in pt.args_of(c)], vec7.detach().cpu().reshape(1, 7).double())
        assert pt.reference_returns_zeros(at_pose['fY']), name


def test_layer_backward_at_large_motion_and_general_K(rpe):
    """DeclarativeLayerLie (L-BFGS 100) on the large-motion rows with general K, .backward() of a tangent loss: the input gradients against
    the truth evaluated at the pose the GPU forward returned, u = -H^-1 v from the truth's own H; 1e-5 relative, as the layer tests of
    tests/test_gpu_pose_backward.py."""
    from rpe_amd import pose_head as ph
    c, _ = pt.case('motion')
    args = pt.args_of(c)
    xs = [a.cuda() for a in args]
    for i in (0, 1, 2, 3, 4, 8):
        xs[i].requires_grad_(True)
    layer = ph.DeclarativeLayerLie(ph.DPoseSE3Head(None, lbgfs_iters=100))
    vec7, log6 = layer(*xs)
    v = torch.randn(3, 1, 6, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                                           # converged, H positive definite
        (log6 * v.float().cuda()).sum().backward()
    T = vec7.detach().cpu().reshape(3, 7).double()
    assert float(pt_angle(T).max()) > 0.45
    H = pt.truth(args, T)['H']
    u = torch.linalg.solve(H, -v.reshape(3, 6, 1).float().double())[..., 0]
    t = pt.truth(args, T, u)
    for i, k in ((0, 'flow'), (1, 'pcl1'), (2, 'pcl2'), (3, 'w1'), (4, 'w2'), (8, 'loss_weight')):
        want = t['g_' + k]
        got = xs[i].grad.cpu().double()
        print(k, '%.2e' % float((got - want).abs().max() / want.abs().max()))
        assert float((got - want).abs().max()) < 1e-5 * float(want.abs().max()), k


def pt_angle(T):
    return 2 * torch.atan2(T[:, 3:6].norm(dim=1), T[:, 6].abs())
