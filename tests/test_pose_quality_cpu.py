"""CPU: the solve-quality report without a GPU -- the float64 truth the GPU tests hold rpe_pose_quality to (tests/quality_ref.py) has the
two properties a covariance must have, the ABI additions are declared, bound and exported and check their arguments, the trackers'
``report_quality`` switch defaults to off, and trajectory.save_quality / read_quality round-trip."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT
from quality_ref import make_inputs, reference
from test_checkpoint_paths import INFER_F2F_YAML, H, W, _checkpoint

NEW = ('rpe_pose_quality', 'rpe_pose_quality_workspace_bytes')
IDENT = torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]], dtype=torch.float64)


def test_quality_abi_declared_bound_exported(rpe):
    from rpe_amd import _lib
    L = rpe.lib()
    header = open(os.path.join(ROOT, 'include', 'rpe.h')).read()
    for name in NEW:
        assert re.search(r'\b(int|size_t) ' + name + r'\(', header) and name in _lib.SIGNATURES and hasattr(L, name), name
    assert 'formal covariance' in ' '.join(header.lower().split()) and 'seeded' in header       # what the header must say about C
    assert L.rpe_pose_quality_workspace_bytes(1, 512, 640) > 0 and L.rpe_pose_quality_workspace_bytes(3, 0, 640) == 0


def test_bad_arguments_return_the_status_of_pose_reduce_without_a_gpu(rpe):
    """Null pointers and non-positive sizes: RPE_E_BADARG before anything touches the device, exactly where rpe_pose_reduce says so."""
    L = rpe.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)          # never dereferenced: the argument checks fail first
    for k in range(10):                                           # each of the nine inputs and T
        ptrs = [one] * 10
        ptrs[k] = null
        assert L.rpe_pose_quality(*ptrs, 1, 8, 8, one, one, null) == -1 == L.rpe_pose_reduce(*ptrs, 1, 8, 8, 1, one, one, null), k
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert L.rpe_pose_quality(*([one] * 10), n, h, w, one, one, null) == -1 == L.rpe_pose_reduce(*([one] * 10), n, h, w, 1, one, one, null)
    assert L.rpe_pose_quality(*([one] * 10), 1, 8, 8, null, one, null) == -1 == L.rpe_pose_reduce(*([one] * 10), 1, 8, 8, 1, null, one, null)   # out
    assert L.rpe_pose_quality(*([one] * 10), 1, 8, 8, one, null, null) == -1 == L.rpe_pose_reduce(*([one] * 10), 1, 8, 8, 1, one, null, null)   # workspace


def test_reference_covariance_is_invariant_to_the_scale_of_the_weights():
    """sigma^2 (J^T W J)^-1 does not change when every weight is scaled: a wrong factor of 2 or a wrong h*w normalisation would."""
    args = make_inputs(1, 37, 53, seed=3)
    a = reference(*args, IDENT)
    scaled = list(args)
    scaled[3], scaled[4] = args[3] * 0.25, args[4] * 0.25
    b = reference(*scaled, IDENT)
    assert bool(a['pd'].all()) and bool(b['pd'].all())
    assert float(((a['cov'] - b['cov']).abs() / a['cov'].abs()).max()) <= 1e-10
    assert float((b['f'] / a['f'] - 0.25).abs().max()) < 1e-12 and torch.equal(a['m'], b['m'])


def test_reference_covariance_grows_when_half_of_the_pixels_are_masked_out():
    args = make_inputs(1, 37, 53, seed=3)
    a = reference(*args, IDENT)
    half = list(args)
    half[5] = args[5].clone()
    half[5][:, :, :, 1::2] = False                                # every other column: the same geometry with half the data
    b = reference(*half, IDENT)
    assert int(b['n3d']) < 0.6 * int(a['n3d']) and int(b['n2d']) < 0.6 * int(a['n2d'])
    tr = lambda r: float(torch.diagonal(r['cov'], dim1=1, dim2=2).sum())
    assert tr(b) > tr(a) > 0.0


def test_reference_degenerate_row():
    args = make_inputs(2, 37, 53, seed=4)
    args[5][0] = False
    r = reference(*args, IDENT.repeat(2, 1))
    assert r['n2d'].tolist()[0] == 0 and r['n3d'].tolist()[0] == 0 and r['pd'].tolist() == [False, True]
    assert bool(torch.isnan(r['cov'][0]).all()) and math.isnan(float(r['rms2d_px'][0])) and math.isnan(float(r['rms3d'][0]))
    assert bool(torch.isfinite(r['cov'][1]).all())


def _slam(f2f=True, **kw):
    slam = yaml.safe_load(INFER_F2F_YAML)['slam']
    slam['frame2frame'] = f2f
    slam.update(kw)
    return slam


def test_report_quality_defaults_to_off(tmp_path):
    from rpe_amd import pose_estimator, synth, trajectory
    path, _, _ = _checkpoint(tmp_path)
    K = synth.intrinsics(H, W)
    assert 'report_quality' not in yaml.safe_load(INFER_F2F_YAML)['slam']
    off = pose_estimator.from_config(_slam(True), K, 1800.0, path, (W, H))
    on = pose_estimator.from_config(_slam(True, report_quality=True), K, 1800.0, path, (W, H))
    assert off.report_quality is False and off.last_quality is None and off._quality_kw() == {}
    assert on.report_quality is True and on._quality_kw() == {'ret_quality': True}
    assert pose_estimator.from_config(_slam(False), K, 1800.0, path, (W, H)).report_quality is False
    assert pose_estimator.from_config(_slam(False, report_quality=True), K, 1800.0, path, (W, H)).report_quality is True
    with pytest.raises(ValueError, match='report_quality'):
        trajectory.track_sequence(off, iter(()), quality=True)
    assert 'quality' not in trajectory.track_sequence(off, iter(()))[0]
    # the initial pose of a run has no solve: NaN covariance, pd = 0
    q = trajectory.track_sequence(on, iter(()), quality=True)[0]['quality']
    assert tuple(q['cov'].shape) == (6, 6) and bool(torch.isnan(q['cov']).all()) and int(q['pd']) == 0 and int(q['n_iter']) == 0
    with pytest.raises(ValueError, match='ret_details'):
        on.model.infer(*([None] * 9), ret_quality=True)


def test_denormalise_quality_scales_the_translation_block_like_the_pose():
    from rpe_amd import pose_estimator
    g = torch.Generator().manual_seed(0)
    A = torch.randn(2, 6, 6, generator=g, dtype=torch.float64)
    q = pose_estimator.blank_quality(2, 'cpu')
    q['cov'], q['rms3d'] = A @ A.transpose(1, 2), torch.tensor([0.01, 0.02], dtype=torch.float64)
    d = pose_estimator.denormalise_quality(q, 250.0)
    s = torch.tensor([250.0] * 3 + [1.0] * 3, dtype=torch.float64)
    assert torch.allclose(d['cov'], q['cov'] * s[None, :, None] * s[None, None, :], rtol=1e-15, atol=0)      # (two roundings against one)
    assert torch.equal(d['rms3d'], q['rms3d'] * 250.0) and d['pd'] is q['pd'] and q['cov'] is not d['cov']


def test_save_quality_and_read_quality_round_trip(tmp_path):
    from rpe_amd import pose_estimator, trajectory
    g = torch.Generator().manual_seed(1)
    traj = []
    for t in range(4):
        A = torch.randn(6, 6, generator=g, dtype=torch.float64)
        q = {k: v[0] for k, v in pose_estimator.blank_quality(1, 'cpu').items()}
        if t > 0:                                                  # (item 0: a frame without a solve, NaN throughout)
            q.update(cov=A @ A.T * 1e-7, pd=torch.tensor(1.0, dtype=torch.float64), n2d=torch.tensor(1000.0 + t, dtype=torch.float64),
                     n3d=torch.tensor(900.0 - t, dtype=torch.float64), rms2d_px=torch.rand((), generator=g, dtype=torch.float64),
                     rms3d=torch.rand((), generator=g, dtype=torch.float64) / 3.0, n_iter=torch.tensor(8, dtype=torch.int32),
                     stop_reason=torch.tensor(3 + t, dtype=torch.int32))
        traj.append({'camera-pose': torch.zeros(7), 'timestamp': 100 + t, 'quality': q})
    traj.append({'camera-pose': torch.zeros(7), 'timestamp': 999})          # an item without a report is left out
    fn = trajectory.save_quality(traj, str(tmp_path))
    assert os.path.basename(fn) == 'trajectory.quality.txt'
    lines = open(fn).read().strip().split('\n')
    assert lines[0].startswith('# stamp pd stop_reason n_iter n2d n3d rms2d_px rms3d_mm cov00 cov01') and len(lines) == 5
    assert all(len(ln.split()) == 8 + 21 for ln in lines[1:])
    r = trajectory.read_quality(fn)
    assert r['timestamp'] == [100, 101, 102, 103]
    assert r['pd'].tolist() == [0, 1, 1, 1] and r['stop_reason'].tolist() == [0, 4, 5, 6] and r['n_iter'].tolist() == [0, 8, 8, 8]
    assert r['n2d'].tolist() == [0, 1001, 1002, 1003] and r['n3d'].tolist() == [0, 899, 898, 897]
    assert np.isnan(r['cov'][0]).all() and np.isnan(r['rms2d_px'][0]) and np.isnan(r['rms3d_mm'][0])
    for t in range(1, 4):
        q = traj[t]['quality']
        want = q['cov'].numpy()
        want = np.triu(want) + np.triu(want, 1).T                  # the file keeps the upper triangle
        assert np.array_equal(r['cov'][t], want)                   # repr round-trips a float64 bit for bit
        assert r['rms2d_px'][t] == float(q['rms2d_px']) and r['rms3d_mm'][t] == float(q['rms3d'])
