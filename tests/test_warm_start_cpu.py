"""CPU: warm start of the trackers from the previous frame's flow -- the rpe_flow_forward_interpolate / rpe_flow_seed ABI (declared,
bound, exported, argument checks without a GPU; RPE_ABI_MINOR unchanged), the seeding op's struct on both sides, the numpy restatement
the GPU tests hold the kernel to (against scipy's griddata where scipy is present), and the tracker modes that refuse warm_start."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT
from flow_interp_ref import forward_interpolate_row, make_flows as _flows
from test_checkpoint_paths import INFER_F2F_YAML, H, W, _checkpoint

NEW = ('rpe_flow_forward_interpolate', 'rpe_flow_seed')


def _slam(f2f=True, **kw):
    slam = yaml.safe_load(INFER_F2F_YAML)['slam']
    slam['frame2frame'] = f2f
    slam.update(kw)
    return slam


def test_warm_start_abi_declared_bound_exported(rpe):
    from rpe_amd import _lib
    L = rpe.lib()
    header = open(os.path.join(ROOT, 'include', 'rpe.h')).read()
    for name in NEW:
        assert re.search(r'\bint ' + name + r'\(', header) and name in _lib.SIGNATURES and hasattr(L, name), name
    assert int(re.search(r'#define RPE_ABI_MINOR (\d+)', header).group(1)) == 4 == L.rpe_abi_minor()
    assert int(re.search(r'#define RPE_OP_FLOW_SEED (\d+)', header).group(1)) == _lib.OP_FLOW_SEED
    assert _lib.LIST_OPS[_lib.OP_FLOW_SEED] == ('rpe_flow_seed', _lib.FlowSeedArgs)


def test_flow_seed_struct_agrees_on_both_sides():
    from rpe_amd import _lib
    assert ctypes.sizeof(_lib.FlowSeedArgs) == 72 and _lib.FlowSeedArgs.coords_out.offset == 24 and _lib.FlowSeedArgs.dst2_batch_stride.offset == 64
    src = open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'oplist.hip')).read()
    assert 'static_assert(sizeof(rpe_flow_seed_args) == 72,' in src and 'case RPE_OP_FLOW_SEED:' in src


def test_bad_arguments_return_badarg_without_a_gpu(rpe):
    L = rpe.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)          # never dereferenced: the argument checks fail first
    assert L.rpe_flow_forward_interpolate(null, 1, 8, 8, one, null) == -1
    assert L.rpe_flow_forward_interpolate(one, 1, 8, 8, null, null) == -1
    assert L.rpe_flow_forward_interpolate(one, 0, 8, 8, one, null) == -1
    assert L.rpe_flow_forward_interpolate(one, 1, 8, -1, one, null) == -1
    assert L.rpe_flow_forward_interpolate(one, 65536, 8, 8, one, null) == -1
    assert L.rpe_flow_seed(null, 1, 8, 8, one, one, null, 0, null, 0, null) == -1
    assert L.rpe_flow_seed(one, 1, 8, 8, one, one, one, 100, null, 0, null) == -1              # slice stride below two planes


def test_restatement_properties():
    f = _flows('zero', 7, 9)[0]
    assert not forward_interpolate_row(f).any()                               # zero flow stays zero (border points land outside)
    assert not forward_interpolate_row(_flows('invalid', 6, 10)[0]).any()    # no valid point: zeros
    f = _flows('shift', 6, 10)[0]
    assert np.array_equal(forward_interpolate_row(f), f)                     # a constant flow is copied everywhere
    # a tie: grid point (1, 0) is equidistant from the points landing at (0.5, 0.5) and (1.5, 0.5) -> the lower source index wins
    f = np.zeros((2, 2, 3), np.float32)
    f[:, 0, 0] = (0.5, 0.5)            # source 0 -> (0.5, 0.5)
    f[:, 0, 1] = (0.5, 0.5)            # source 1 -> (1.5, 0.5)
    f[0, 0, 2] = 9.0                   # the other points land outside
    f[0, 1, :] = 9.0
    out = forward_interpolate_row(f)
    assert np.array_equal(out[:, 0, 0], f[:, 0, 0]) and np.array_equal(out[:, 0, 1], f[:, 0, 0])


@pytest.mark.parametrize('h,w,kind,seed', [(8, 10, 'subpixel', 1), (13, 11, 'subpixel', 2), (16, 20, 'outward', 3), (9, 7, 'subpixel', 4)])
def test_restatement_agrees_with_scipy_griddata(h, w, kind, seed):
    """Upstream's forward_interpolate on tie-free random flows (random sub-pixel landing points: no two at the same distance)."""
    interpolate = pytest.importorskip('scipy.interpolate')
    f = _flows(kind, h, w, seed)[0]
    dx, dy = f[0].astype(np.float64), f[1].astype(np.float64)
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1, y1 = (x0 + dx).reshape(-1), (y0 + dy).reshape(-1)
    valid = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    assert valid.sum() >= 2
    pts = np.stack([x1[valid], y1[valid]], axis=1)
    up = np.stack([interpolate.griddata(pts, d.reshape(-1)[valid], (x0, y0), method='nearest', fill_value=0) for d in (dx, dy)]).astype(np.float32)
    assert np.array_equal(forward_interpolate_row(f), up)


def test_trackers_accept_warm_start_and_refuse_the_batched_modes(tmp_path):
    from rpe_amd import pose_estimator, sharding, synth, trajectory
    path, _, _ = _checkpoint(tmp_path)
    K = synth.intrinsics(H, W)
    img, mask = torch.zeros(2, 3, H, W), torch.ones(2, 1, H, W, dtype=torch.bool)
    warm = pose_estimator.from_config(_slam(True, warm_start=True), K, 1800.0, path, (W, H))
    cold = pose_estimator.from_config(_slam(True), K, 1800.0, path, (W, H))
    assert warm.warm_start is True and cold.warm_start is False
    assert pose_estimator.from_config(_slam(False, warm_start=True), K, 1800.0, path, (W, H)).warm_start is True
    # refused on entry, before the check that the sequence has a first frame (which a cold estimator meets here)
    with pytest.raises(ValueError, match='warm_start'):
        warm.forward_chunk(img, img, mask)
    with pytest.raises(RuntimeError, match='first frame'):
        cold.forward_chunk(img, img, mask)
    # SequenceTracker: refused before the sharding / scale checks a cold one meets
    with pytest.raises(ValueError, match='warm_start'):
        sharding.SequenceTracker(lambda: warm, lambda t: None).track(4, rank=0, world=1, scale=1.0)
    with pytest.raises(ValueError, match='warm_start'):
        sharding.SequenceTracker(lambda: warm, lambda t: None).run_block(0, 3)
    with pytest.raises(ValueError, match='scale'):
        sharding.SequenceTracker(lambda: cold, lambda t: None).track(4, rank=0, world=1, scale=1.0)
    with pytest.raises(ValueError, match='chunk'):
        trajectory.track_sequence(warm, iter(()), chunk=4)
    assert len(trajectory.track_sequence(cold, iter(()), chunk=4)) == 1
    assert len(trajectory.track_sequence(warm, iter(()), chunk=1)) == 1
    warm._flow_low = torch.zeros(1, 2, H // 8, W // 8)
    warm.reset()
    assert warm._flow_low is None
