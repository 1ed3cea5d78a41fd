"""Host only: the autograd truth of tests/pose_grad_truth.py against (1) the reference's own autograd results and (2) the closed-form
oracle, oracle/pose_grad.py, on every edge case the GPU tests of csrc/pose_backward.hip run.

Measured float64 disagreement between the truth and oracle/pose_grad.py, the largest over all finite cases (per-pixel outputs: as a fraction
of the pixel's own largest |gradient|; moments: of the row's largest entry):
    flow 1.3e-14   pcl1 1.1e-14   pcl2 1.9e-15   w1 3.7e-11   w2 1.2e-11   (w1, w2: a dot product J u . g that nearly cancels at a few pixels;
    fY 3.2e-14   g2u 5.7e-14   g3u 2.7e-14   H 8.5e-16   loss_weight 1.1e-13    the figure moves with the host: w1 was 7.6e-12 on another)
``pose_grad_truth.F64_DISAGREEMENT`` holds the per-pixel figures as measured; ten times them is the conditioning floor of the GPU
comparison.  Margin policy: the figures depend on the host's float64 library, so this file holds a run to that floor (ten times the
recorded figure), and in every case to a tenth of half a float32 ulp of the pixel's gradient (2^-24 = 6e-8 relative, the smallest an ulp
gets); the recorded floor itself is at most 3.7e-10, a factor 160 below it.

No disagreement beyond rounding was found in a finite case: depth clamp, gates, K with every entry filled, 0.5 rad rotations and zero
weights included.  With a non-finite input the two differ as documented at ``test_nonfinite_rows``."""
import warnings

import pytest
import torch

import pose_grad_truth as pt
from conftest import SOLVER_KEYS, load_golden
from oracle import pose_grad
from oracle.pose_head import _prep

FINITE = [k for k in pt.CASES if k != 'nonfinite']


def _rowmax(t):
    return t.reshape(t.shape[0], -1).abs().amax(1)


def _rel_rows(a, b):
    """max over rows of max|a - b| / max|b| (rows of zeros must match exactly)."""
    d, s = _rowmax(a - b), _rowmax(b)
    return float(torch.where(s > 0, d / s, d).max())


def _rel_pixels(a, t):
    s = pt.pixel_scale(t)
    return float(((a - t).abs() / torch.where(s > 0, s, torch.ones_like(s))).max())


@pytest.mark.parametrize('name', ['backward_a', 'backward_b'])
def test_truth_reproduces_the_reference_autograd_golden(name):
    """fY, the symmetrised fYY and every input gradient the reference's own DeclarativeNodeLie produced in float64, at the stored vec7 with
    u solved from the stored fYY.  float64 on both sides, two different graphs: 1e-12 of each quantity's scale (fY: of the per-term
    gradients, which cancel at the solution).  (The kernels take vec7 as it is, without renormalising: 1e-8 relative, below the float32
    rounding of the pose itself; tests/test_gpu_pose_backward.py compares them with these goldens at 1e-6.)"""
    g = load_golden(name + '.npz')
    args = [g[k] for k in SOLVER_KEYS]
    n = args[0].shape[0]
    Href = 0.5 * (g['fYY_f64'] + g['fYY_f64'].transpose(1, 2))
    u = torch.linalg.solve(Href, -g['v'].reshape(n, 6, 1).double())[..., 0]
    T = g['vec7'].reshape(n, 7).double()
    off_unit = float((T[:, 3:].norm(dim=1) ** 2 - 1).abs().max())      # ~1e-8: vec7 is a float32 quaternion
    T[:, 3:] /= T[:, 3:].norm(dim=1, keepdim=True)        # the reference's retraction exp(xi) * SE3(vec7) renormalises it
    t = pt.truth(args, T, u)
    assert float((t['fY'] - g['fY_f64']).abs().max()) < 1e-12 * float(max(t['g2u'].abs().max(), t['g3u'].abs().max()))
    assert float((t['H'] - Href).abs().max()) < 1e-12 * float(Href.abs().max())
    assert float((t['H'] - t['H'].transpose(1, 2)).abs().max()) < 1e-12 * float(Href.abs().max())
    for k in pt.GRADS + ('loss_weight',):
        ref = g[f'g_{k}_f64']
        # pcl1: the reference's Transform.backward (pinhole_transforms.py:47-51) rotates the gradient back with the matrix of the quaternion
        # as stored, not renormalised; that matrix is off a rotation by | |q|^2 - 1 |
        tol = 1e-12 + (2 * off_unit if k == 'pcl1' else 0.0)
        assert float((t['g_' + k].reshape(ref.shape) - ref).abs().max()) < tol * float(ref.abs().max()), k


def test_truth_of_a_batch_is_the_truth_of_its_rows():
    c, t = pt.case('clamp')
    for r in range(3):
        one = pt.truth([a[r:r + 1] for a in pt.args_of(c)], c['T'][r:r + 1], c['u'][r:r + 1])
        for k in ('f', 'fY', 'g2u', 'g3u', 'H') + tuple('g_' + k for k in pt.GRADS):
            assert float((one[k] - t[k][r:r + 1]).abs().max()) <= 1e-13 * float(t[k][r].abs().max()), (r, k)


def test_every_planted_class_is_present():
    """What each case claims to hold, read off the truth's own gates (float64, the flow as the float32 the kernels get)."""
    c, t = pt.case('motion')
    assert float(ose_angle(c['T']).max()) > 0.45 and float(c['T'][:, :3].norm(dim=1).max()) > 0.08
    assert bool((c['K'][:, 0, 1] != 0).all()) and bool((c['K'][2, 2] != torch.tensor([0.0, 0.0, 1.0])).all()) and float(c['K'][2, 1, 0]) != 0
    assert torch.equal(c['loss_weight'][:2], torch.tensor([[0.3, 2.0], [1.0, 0.0]]))
    for name in FINITE:
        c, t = pt.case(name)
        n, _, h, w = c['flow'].shape
        gated_in = (~t['bad']).reshape(n, -1).double().mean(1)
        assert float(gated_in.min()) >= (0.25 if h * w > 1 else 1.0), name       # every row has real reprojection terms
        assert float(t['a_z'].min()) > 0.05 or name == 'clamp'
    c, t = pt.case('gates')
    bad, ok3 = t['bad'].reshape(2, 9, 13), t['ok3'].reshape(2, 9, 13)
    P = c['planted']
    for name in ('fx_on_0', 'fx_on_W', 'fy_on_0', 'fy_on_H'):
        assert all(bool(bad[r, y, x]) and bool(c['mask1'][r, 0, y, x]) for r, y, x in P[name]), name
    fo = c['flow'].double() + torch.stack(torch.meshgrid(torch.arange(9) + 0.5, torch.arange(13) + 0.5, indexing='ij')[::-1])[None]
    assert [float(fo[r, 0, y, x]) for r, y, x in P['fx_on_0'] + P['fx_on_W']] == [0.0, 0.0, 13.0, 13.0]
    assert [float(fo[r, 1, y, x]) for r, y, x in P['fy_on_0'] + P['fy_on_H']] == [0.0, 0.0, 9.0, 9.0]
    for name, ch, lo, hi in (('fx_inside_0', 0, 0.0, 1e-6), ('fx_inside_W', 0, 13 - 1e-6, 13.0), ('fy_inside_0', 1, 0.0, 1e-6), ('fy_inside_H', 1, 9 - 1e-6, 9.0)):
        assert all(not bool(bad[r, y, x]) and lo < float(fo[r, ch, y, x]) < hi for r, y, x in P[name]), name
    for a in (True, False):
        for b in (True, False):
            for r, y, x in P['mask_%d%d' % (a, b)]:
                assert bool(bad[r, y, x]) == (not a) and bool(ok3[r, y, x]) == (a and b)
    gw1, gw2 = t['g_w1'], t['g_w2']
    for r, y, x in P['w1_zero'] + P['w12_zero']:
        assert float(c['w1'][r, 0, y, x]) == 0.0 and not bool(bad[r, y, x]) and abs(float(gw1[r, 0, y, x])) > 1e-3 * float(gw1[r].abs().max())
    for r, y, x in P['w2_zero'] + P['w12_zero']:
        assert float(c['w2'][r, 0, y, x]) == 0.0 and bool(ok3[r, y, x]) and abs(float(gw2[r, 0, y, x])) > 1e-3 * float(gw2[r].abs().max())
    c, t = pt.case('clamp')
    az, bad = t['a_z'].reshape(3, 6, 7), t['bad'].reshape(3, 6, 7)
    P = c['planted']
    assert all(float(az[r, y, x]) < -0.1 for r, y, x in P['behind_in'] + P['behind_out'])
    assert all(float(az[r, y, x]) == 0.0 for r, y, x in P['on_plane_in'] + P['on_plane_out'])
    assert all(not bool(bad[r, y, x]) for r, y, x in P['behind_in'] + P['on_plane_in'])
    assert all(bool(bad[r, y, x]) for r, y, x in P['behind_out'] + P['on_plane_out'])
    assert int((az < 1e-12).sum()) == 6
    for r in range(3):                                   # the clamped pixels outweigh the rest of their row by many orders of magnitude
        m = pt.planted_mask(c)[r, 0]
        assert float(t['g_pcl1'][r][:, m].abs().max()) > 1e15 * float(t['g_pcl1'][r][:, ~m].abs().max())
    c, t = pt.case('nonfinite')
    assert len(c['planted']) == 16 and set(c['planted']) == set(pt.NONFINITE)
    for row, k in enumerate(pt.NONFINITE):
        key, val, gate_name = k.split('_')
        (r, y, x), = c['planted'][k]
        bad_entries = ~torch.isfinite(c[key][r])
        assert r == row and int(bad_entries.sum()) == 1 and bool(bad_entries[:, y, x].any())
        assert bool((torch.isnan if val == 'nan' else torch.isinf)(c[key][r, :, y, x]).any())
        assert all(bool(torch.isfinite(c[o][r]).all()) for o in ('flow', 'pcl1', 'pcl2', 'w1', 'w2') if o != key)
        gate = c['mask1'][r, 0, y, x] & (c['mask2'][r, 0, y, x] if key in ('pcl2', 'w2') else True)
        assert bool(gate) == (gate_name == 'in')
        if key != 'flow':
            assert bool(t['inimg'].reshape(16, 5, 7)[r, y, x])


def ose_angle(T):
    return 2 * torch.atan2(T[:, 3:6].norm(dim=1), T[:, 6].abs())


@pytest.mark.parametrize('name', FINITE)
def test_truth_agrees_with_the_closed_form_oracle(name):
    """objective_derivatives and the closed forms of layer_backward (u supplied) against autograd, case by case.  Moments: 1e-11 of the
    row's largest entry (float64 sums of at most 1353 terms, a hundredth of the GPU test's bar); per-pixel gradients: within the floor the
    GPU comparison gets (ten times the recorded disagreement) and within a tenth of half a float32 ulp of the pixel's gradient, so the
    case is well conditioned; exactly zero where the truth is."""
    c, t = pt.case(name)
    args = pt.args_of(c)
    fY, fYY, g2u, g3u, _, _ = pose_grad.objective_derivatives(_prep(*args), c['T'])
    out, _, _ = pose_grad.layer_backward(*args, c['T'], None, u=c['u'])
    scale = torch.maximum(_rowmax(t['g2u']) * c['loss_weight'][:, 1].abs().double(), _rowmax(t['g3u']) * c['loss_weight'][:, 0].abs().double())
    assert float((_rowmax(fY - t['fY']) / scale).max()) < 1e-11                  # fY cancels between its two terms near a solution
    for nm, a, b in (('g2u', g2u, t['g2u']), ('g3u', g3u, t['g3u']), ('H', 0.5 * (fYY + fYY.transpose(1, 2)), t['H']),
                     ('loss_weight', out['loss_weight'], t['g_loss_weight'])):
        assert _rel_rows(a, b) < 1e-11, nm
    for k in pt.GRADS:
        tk = t['g_' + k]
        assert not bool(torch.isnan(tk).any()) and bool(torch.isfinite(tk.float()).all()), k      # and it fits a float32
        print(name, k, 'disagreement %.1e of the pixel' % _rel_pixels(out[k], tk))
        assert _rel_pixels(out[k], tk) <= 10.0 * pt.F64_DISAGREEMENT[k], k
        assert 10.0 * _rel_pixels(out[k], tk) < 2.0 ** -24 and 10.0 * pt.F64_DISAGREEMENT[k] < 2.0 ** -24 / 100, k
        assert bool((out[k][tk == 0] == 0).all()), k


def test_nonfinite_rows():
    """NaN and inf in flow, w1, pcl2 and w2, gated in and gated out: 16 rows.  Autograd (0 * NaN = NaN, as in the reference) gives a NaN fY
    in every such row -- so the reference's backward fails its optimality check and returns zeros with a warning, whatever the rest holds
    -- and, by double backward, NaN for every per-pixel gradient of the row (zeros after the reference's NaN -> 0 rule).
    The closed forms (and the kernels, which they mirror):
      * w1, pcl2, w2 not finite: fY is not finite either, in the same rows.  At the planted pixel they hold ``pt.PLANTED_PIXEL`` -- zeros
        or that pixel's other term for most, but +-inf where an inf in pcl2 or w2 meets an open 3D gate (inf is not NaN, so the NaN -> 0
        rule lets it through).  The layer never returns those: fY of such a row is not finite, so its backward returns zeros.
      * flow not finite (rows 0..3): the 2D residual is cut off by selection, so g2u, H and the gradients are finite, those of the same input
        with that pixel's flow outside the image (``sanitised``).  That changes nothing for the layer: its forward propagates the NaN into
        the pose (tests/test_gpu_pose.py::test_nan_poisons_pose_like_reference), and at a NaN pose every moment is NaN on both sides."""
    c, t = pt.case('nonfinite')
    args = pt.args_of(c)
    assert bool(torch.isnan(t['fY']).any(dim=1).all()) and pt.reference_returns_zeros(t['fY'])
    assert all(pt.reference_returns_zeros(t['fY'][r:r + 1]) for r in range(16))
    assert all(bool(torch.isnan(t['g_' + k]).all()) for k in pt.GRADS)
    fY, fYY, g2u, g3u, _, _ = pose_grad.objective_derivatives(_prep(*args), c['T'])
    Hs = 0.5 * (fYY + fYY.transpose(1, 2))
    rows = lambda m: (~torch.isfinite(m)).reshape(16, -1).any(1).tolist()
    assert rows(fY) == [False] * 4 + [True] * 12 and all(pt.reference_returns_zeros(fY[r:r + 1]) for r in range(4, 16))
    assert rows(g2u)[4:] == rows(t['g2u'])[4:] == [True] * 4 + [False] * 8 and rows(g3u) == rows(t['g3u']) == [False] * 8 + [True] * 8
    assert rows(Hs)[4:] == rows(t['H'])[4:] == [True] * 12
    s = pt.sanitised(c)
    ts = pt.truth(pt.args_of(s), s['T'], s['u'])
    assert _rel_rows(g2u[pt.FLOW_ROWS], ts['g2u'][pt.FLOW_ROWS]) < 1e-11 and _rel_rows(Hs[pt.FLOW_ROWS], ts['H'][pt.FLOW_ROWS]) < 1e-11
    out, _, _ = pose_grad.layer_backward(*args, c['T'], None, u=c['u'])
    assert pt.planted_classes(out, c) == pt.PLANTED_PIXEL
    away = ~pt.planted_mask(c)
    zero = lambda x: torch.zeros_like(x)
    for k in pt.GRADS:                                    # away from the planted pixel a gradient does not depend on it
        assert not bool(torch.isnan(out[k]).any())
        assert _rel_pixels(torch.where(away, out[k], zero(out[k])), torch.where(away, ts['g_' + k], zero(out[k]))) <= 10.0 * pt.F64_DISAGREEMENT[k], k
        assert _rel_pixels(out[k][pt.FLOW_ROWS], ts['g_' + k][pt.FLOW_ROWS]) <= 10.0 * pt.F64_DISAGREEMENT[k], k
    nanT = torch.full((16, 7), float('nan'), dtype=torch.float64)
    assert bool(torch.isnan(pt.truth(args, nanT)['fY']).all())
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        zeros, fYn, _ = pose_grad.layer_backward(*args, nanT, c['u'])
    assert bool(torch.isnan(fYn).all()) and all(float(v.abs().max()) == 0.0 for v in zeros.values())

