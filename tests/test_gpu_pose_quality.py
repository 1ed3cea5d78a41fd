"""GPU: rpe_pose_quality (csrc/pose_quality.hip, ops.pose_quality) against the float64 CPU truth of tests/quality_ref.py.

Shapes: 37x53 with n = 1 (no multiple of anything, two workgroups) and 96x160 with n = 3 (15 workgroups per row).  Seeded inputs
(quality_ref.make_inputs): partial masks, non-unit weights, flows that leave the image on every border, one NaN flow value (case A row 0,
case B row 1 -- its 0 * NaN reaches g and max|g| as in the reference, nothing else), one point behind the camera (iz < 1e-12: case A
with its flow outside the image, case B row 2 kept by the reprojection term with w1 = 0).  Every check runs at the identity and at a
solved pose (the CPU oracle's 12-iteration L-BFGS on the inputs without the NaN).

Bounds.  Counts and m: exact.  Sums, f, g, both RMS: 1e-10 relative -- positive f64 sums of at most 15 360 terms differ by at most
N eps ~ 2e-12 between summation orders.  g is a signed sum, its error scales with the sum of the |terms|, not with g: the test takes
1e-10 relative to max|g| of the row, which is still 8 decimal digits below what a solve's stopping tests look at.  Covariance:
max |C H_ref (m - 6) / (2 f_ref) - I| <= 1e-8; cond(H_ref) of the inputs, printed by the test from the CPU reference:
    case A (37x53):   114 at the identity, 113 at the solved pose
    case B (96x160):  106 / 236 / 113 at the identity, 106 / 233 / 113 at the solved pose
so cond * 1e-16 <= 2.4e-14, five orders below the bound."""
import ctypes

import pytest
import torch

from quality_ref import make_inputs, reference

pytestmark = pytest.mark.gpu
F64 = torch.float64
CASES = {'A-37x53-n1': dict(n=1, h=37, w=53, seed=11, nan_rows=(0,), z_rows=(0,)),
         'B-96x160-n3': dict(n=3, h=96, w=160, seed=12, nan_rows=(1,), z_rows=(2,), z_in_image=True)}
_CACHE = {}


def _identity(n):
    T = torch.zeros(n, 7, dtype=F64)
    T[:, 6] = 1.0
    return T


def _case(name):
    """Inputs, the two poses and the CPU reference at each: computed once, shared by every test, never modified."""
    if name not in _CACHE:
        from oracle import pose_head as oph
        c = dict(CASES[name])
        n, h, w, seed = c.pop('n'), c.pop('h'), c.pop('w'), c.pop('seed')
        args = make_inputs(n, h, w, seed, **c)
        clean = list(args)
        clean[0] = torch.nan_to_num(args[0])
        poses = dict(identity=_identity(n), solved=oph.lbfgs_solve(*clean, iters=12)[0])
        assert bool(torch.isfinite(poses['solved']).all()) and float((poses['solved'] - poses['identity']).abs().max()) > 1e-3
        _CACHE[name] = dict(args=args, dev=[a.cuda() for a in args], poses=poses, ref={k: reference(*args, T) for k, T in poses.items()})
    return _CACHE[name]


def _rel(a, b):
    return float(((a - b).abs() / b.abs()).max())


@pytest.mark.parametrize('pose', ['identity', 'solved'])
@pytest.mark.parametrize('name', list(CASES))
def test_parity_with_the_float64_reference(rpe, name, pose):
    from rpe_amd import ops
    c = _case(name)
    ref, T = c['ref'][pose], c['poses'][pose]
    out = ops.pose_quality(*c['dev'], T.cuda()).cpu()
    q = ops.quality_fields(out)
    n = T.shape[0]
    print(f'{name} {pose}: cond(H_ref) = {[round(float(x), 1) for x in ref["cond"]]}')
    # counts: exact
    assert torch.equal(q['n2d'], ref['n2d'].to(F64)) and torch.equal(q['n3d'], ref['n3d'].to(F64)) and torch.equal(q['m'], ref['m'].to(F64))
    assert bool((ref['n2d'] > 0).all()) and bool((ref['n2d'] < c['args'][0].shape[2] * c['args'][0].shape[3]).all())
    assert torch.equal(out[:, 54:], torch.zeros(n, 10, dtype=F64)) and torch.equal(q['pd'], torch.ones(n, dtype=F64)) and bool(ref['pd'].all())
    for k in ('sum_w1', 'sum_w2', 'sse2d', 'sse3d', 'rms2d_px', 'rms3d', 'f'):
        err = _rel(q[k], ref[k])
        print(f'  {k}: rel err {err:.3e}')
        assert err <= 1e-10, (k, err)
    for i in range(n):
        if bool(torch.isnan(ref['g'][i]).any()):               # the NaN row: 0 * NaN reaches g, in the same components
            assert torch.equal(torch.isnan(q['g'][i]), torch.isnan(ref['g'][i])) and bool(torch.isnan(q['grad_max'][i]))
            continue
        scale = float(ref['g'][i].abs().max())
        err = float((q['g'][i] - ref['g'][i]).abs().max()) / scale
        print(f'  g row {i}: err / max|g| {err:.3e}, max|g| {scale:.3e}')
        assert err <= 1e-10 and abs(float(q['grad_max'][i]) - scale) <= 1e-10 * scale
        # covariance through the identity C H_ref (m - 6) / (2 f_ref) = I
    eye = torch.eye(6, dtype=F64)
    for i in range(n):
        resid = q['cov'][i] @ ref['H'][i] * (float(ref['m'][i]) - 6.0) / (2.0 * float(ref['f'][i])) - eye
        err = float(resid.abs().max())
        print(f'  C H_ref (m-6)/(2f) - I row {i}: {err:.3e}')
        assert err <= 1e-8, (i, err)
        assert float(ref['cond'][i]) * 1e-16 * 100 < 1e-8
        assert torch.equal(q['cov'][i], q['cov'][i].T)
    if name.startswith('B'):
        assert float(q['rms2d_px'][2]) > 1e9                    # the clamped point (u = ix / 1e-12) is in the unweighted RMS of row 2


def test_rows_do_not_depend_on_the_batch(rpe):
    from rpe_amd import ops
    c = _case('B-96x160-n3')
    T = c['poses']['solved'].cuda()
    both = ops.pose_quality(*c['dev'], T)
    for k in range(3):
        alone = ops.pose_quality(*[a[k:k + 1].contiguous() for a in c['dev']], T[k:k + 1])
        same = (alone == both[k:k + 1]) | (torch.isnan(alone) & torch.isnan(both[k:k + 1]))
        assert bool(same.all()), k
        assert torch.equal(alone.view(torch.int64), both[k:k + 1].view(torch.int64)), k           # NaN payloads included


@pytest.mark.parametrize('name', list(CASES))
def test_covariance_is_invariant_to_the_scale_of_the_weights(rpe, name):
    from rpe_amd import ops
    c = _case(name)
    T = c['poses']['solved'].cuda()
    a = ops.quality_fields(ops.pose_quality(*c['dev'], T))
    scaled = list(c['dev'])
    scaled[3], scaled[4] = scaled[3] * 0.25, scaled[4] * 0.25
    b = ops.quality_fields(ops.pose_quality(*scaled, T))
    assert _rel(b['cov'], a['cov']) <= 1e-10
    assert _rel(b['f'], 0.25 * a['f']) <= 1e-12 and torch.equal(a['m'], b['m'])


@pytest.mark.parametrize('name', list(CASES))
def test_masking_half_of_the_pixels_increases_the_trace(rpe, name):
    from rpe_amd import ops
    c = _case(name)
    T = c['poses']['solved'].cuda()
    a = ops.quality_fields(ops.pose_quality(*c['dev'], T))
    half = list(c['dev'])
    half[5] = half[5].clone()
    half[5][:, :, :, 1::2] = False
    b = ops.quality_fields(ops.pose_quality(*half, T))
    tr = lambda q: torch.diagonal(q['cov'], dim1=1, dim2=2).sum(-1)
    assert bool((b['n3d'] < 0.6 * a['n3d']).all()) and bool((tr(b) > tr(a)).all()) and bool((tr(a) > 0).all())


def test_degenerate_row_beside_a_good_one(rpe):
    from rpe_amd import ops
    c = _case('B-96x160-n3')
    T = c['poses']['identity'].cuda()
    base = ops.pose_quality(*c['dev'], T)
    args = list(c['dev'])
    args[5] = args[5].clone()
    args[5][1] = False                                              # row 1 (the NaN row) loses every pixel
    out = ops.pose_quality(*args, T)
    q = ops.quality_fields(out)
    assert float(q['n2d'][1]) == 0.0 and float(q['n3d'][1]) == 0.0 and float(q['pd'][1]) == 0.0 and float(q['m'][1]) == 0.0
    assert bool(torch.isnan(q['cov'][1]).all()) and bool(torch.isnan(q['rms2d_px'][1])) and bool(torch.isnan(q['rms3d'][1]))
    assert float(q['f'][1]) == 0.0
    for k in (0, 2):
        assert torch.equal(out[k].view(torch.int64), base[k].view(torch.int64)), k


def test_bad_arguments_return_the_status_of_pose_reduce(rpe):
    from rpe_amd import ops
    from rpe_amd._lib import ptr
    L = rpe.lib()
    c = _case('A-37x53-n1')
    args, n, h, w = ops._pose_inputs(*c['dev'])
    T = c['poses']['identity'].cuda()
    out, out32 = torch.empty(1, 64, dtype=F64, device='cuda'), torch.empty(1, 32, dtype=F64, device='cuda')
    wq = torch.empty(L.rpe_pose_quality_workspace_bytes(n, h, w), dtype=torch.uint8, device='cuda')
    wr = torch.empty(L.rpe_pose_workspace_bytes(n, h, w), dtype=torch.uint8, device='cuda')
    null = ctypes.c_void_p(0)
    P = [ptr(a) for a in args] + [ptr(T)]
    for k in range(10):
        bad = list(P)
        bad[k] = null
        assert L.rpe_pose_quality(*bad, n, h, w, ptr(out), ptr(wq), null) == L.rpe_pose_reduce(*bad, n, h, w, 1, ptr(out32), ptr(wr), null) == -1
    for dims in ((0, h, w), (n, -1, w), (n, h, 0)):
        assert L.rpe_pose_quality(*P, *dims, ptr(out), ptr(wq), null) == L.rpe_pose_reduce(*P, *dims, 1, ptr(out32), ptr(wr), null) == -1
    assert L.rpe_pose_quality(*P, n, h, w, null, ptr(wq), null) == L.rpe_pose_reduce(*P, n, h, w, 1, null, ptr(wr), null) == -1
    assert L.rpe_pose_quality(*P, n, h, w, ptr(out), null, null) == L.rpe_pose_reduce(*P, n, h, w, 1, ptr(out32), null, null) == -1
    assert L.rpe_pose_quality(*P, n, h, w, ptr(out), ptr(wq), ops.stream_ptr()) == 0
    torch.cuda.synchronize()


def test_head_quality_defaults_to_the_last_solve(rpe):
    """DPoseSE3Head.quality: the report at the float64 pose of the last solve, whose info it keeps on the device."""
    from rpe_amd import ops, pose_head
    c = _case('A-37x53-n1')
    clean = list(c['dev'])
    clean[0] = torch.nan_to_num(clean[0])
    head = pose_head.DPoseSE3Head(lbgfs_iters=12)
    with pytest.raises(ValueError):
        head.quality(*clean)
    Tse3, _ = head.solve(*clean)
    assert head.last_info.is_cuda and tuple(head.last_info.shape) == (1, 4) and head.last_T.dtype == F64
    assert float((head.last_T.cpu() - c['poses']['solved']).abs().max()) < 1e-8
    assert torch.equal(head.quality(*clean), ops.pose_quality(*clean, head.last_T))
    assert torch.equal(head.quality(*clean, T=Tse3), head.quality(*clean))
