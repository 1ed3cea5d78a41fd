"""CPU: the batched frame-to-model pieces -- the rpe_surfel_*_many / rpe_pose_gate_chain_rows ABI (declared, bound, argument checks
without a GPU, workspace sizes) and MultiSurfelPoseEstimator's construction and refusals."""
import ctypes
import os
import re

import pytest
import torch
import yaml

from conftest import ROOT
from test_checkpoint_paths import INFER_F2F_YAML, H, W, _checkpoint

MANY_ENTRIES = ('rpe_surfel_workspace_bytes_many', 'rpe_surfel_init_many', 'rpe_surfel_render_many', 'rpe_surfel_fuse_many',
                'rpe_pose_gate_chain_rows')
B, OK = -1, 0


def _slam(f2f):
    slam = yaml.safe_load(INFER_F2F_YAML)['slam']
    slam['frame2frame'] = f2f
    return slam


def test_many_abi_declared_bound_exported(rpe):
    from rpe_amd import _lib
    L = rpe.lib()
    for name in MANY_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    header = open(os.path.join(ROOT, 'include', 'rpe.h')).read()
    assert int(re.search(r'#define RPE_ABI_MINOR (\d+)', header).group(1)) == 4 == L.rpe_abi_minor() == _lib.ABI_MINOR_MANY
    assert int(re.search(r'#define RPE_SURFEL_MAX_MAPS (\d+)', header).group(1)) == _lib.SURFEL_MAX_MAPS == 64
    assert ctypes.sizeof(_lib.SurfelMapDesc * 3) == 3 * 56          # the descriptor arrays the batched calls take


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_many_workspace_covers_the_single_map_sizes(rpe):
    L = rpe.lib()
    for bounds, h, w in (([0], 4, 4), ([1000, 0, 4_000_000], 512, 640), ([7] * 64, 32, 48), ([10 ** 8, 5], 352, 384)):
        many = L.rpe_surfel_workspace_bytes_many(len(bounds), _i64(*bounds), h, w)
        assert many >= sum(L.rpe_surfel_workspace_bytes(b, h, w) for b in bounds), (bounds, h, w)
    assert L.rpe_surfel_workspace_bytes_many(0, _i64(0), 4, 4) == 0
    assert L.rpe_surfel_workspace_bytes_many(65, _i64(*([0] * 65)), 4, 4) == 0          # above RPE_SURFEL_MAX_MAPS
    assert L.rpe_surfel_workspace_bytes_many(2, _i64(0, -1), 4, 4) == 0
    assert L.rpe_surfel_workspace_bytes_many(1, None, 4, 4) == 0


def test_many_bad_arguments_return_badarg_without_a_gpu(rpe):
    from rpe_amd import _lib
    L = rpe.lib()
    fake = ctypes.c_void_p(0x1000)                      # never dereferenced: every call below fails its argument check first

    def desc(base, cap=16):
        return _lib.SurfelMapDesc(ctypes.c_void_p(base), fake, fake, fake, cap, ctypes.c_void_p(base + 8), fake)

    def arr(*d):
        return (_lib.SurfelMapDesc * len(d))(*d)

    def ptrs(n, p=fake):
        return (ctypes.c_void_p * n)(*([p] * n))

    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)                                  # noqa: E731
    two, two_other = arr(desc(0x2000), desc(0x3000)), arr(desc(0x4000), desc(0x5000))
    null_map = arr(desc(0x2000), _lib.SurfelMapDesc(None, fake, fake, fake, 16, fake, fake))
    nb = _i64(0, 0)

    # rpe_pose_gate_chain_rows: as rpe_pose_gate_chain
    assert L.rpe_pose_gate_chain_rows(None, None, None, fake, None, 4, 1.0, 0.1, 0, None) == B
    assert L.rpe_pose_gate_chain_rows(fake, None, None, fake, None, 4, 1.0, 0.1, 7, None) == B        # unknown dtype
    assert L.rpe_pose_gate_chain_rows(fake, None, None, fake, None, -1, 1.0, 0.1, 0, None) == B
    assert L.rpe_pose_gate_chain_rows(fake, None, None, fake, None, 0, 1.0, 0.1, 0, None) == OK

    # render: K = 0 is a no-op, K > 64, null tables, bad shapes
    r = (fake, fake, 1, 8, 8, fake, fake, fake, fake, fake, None)
    assert L.rpe_surfel_render_many(0, None, None, *r) == OK
    assert L.rpe_surfel_render_many(65, two, nb, *r) == B
    assert L.rpe_surfel_render_many(-1, two, nb, *r) == B
    assert L.rpe_surfel_render_many(2, None, nb, *r) == B
    assert L.rpe_surfel_render_many(2, two, None, *r) == B
    assert L.rpe_surfel_render_many(2, null_map, nb, *r) == B
    assert L.rpe_surfel_render_many(2, two, _i64(0, 17), *r) == B                       # bound past a capacity
    assert L.rpe_surfel_render_many(2, two, nb, fake, fake, 1, 2, 8, *r[5:]) == B       # h < 3
    assert L.rpe_surfel_render_many(2, two, nb, None, *r[1:]) == B

    # init
    i = (fake, fake, fake, fake, 8, 8, ptrs(2), fake, 7.0)
    assert L.rpe_surfel_init_many(0, None, None, None, None, 8, 8, None, None, 7.0, None, None, None) == OK
    assert L.rpe_surfel_init_many(65, *i, two, fake, None) == B
    assert L.rpe_surfel_init_many(2, *i, None, fake, None) == B
    assert L.rpe_surfel_init_many(2, *i, null_map, fake, None) == B
    assert L.rpe_surfel_init_many(2, *i[:6], ptrs(2, None), *i[7:], two, fake, None) == B            # a null kinv
    assert L.rpe_surfel_init_many(2, *i, arr(desc(0x2000), desc(0x2000)), fake, None) == B          # two maps share storage
    assert L.rpe_surfel_init_many(2, *i[:4], 0, *i[5:], two, fake, None) == B

    # fuse
    def fuse(n, src=two, bounds=nb, dst=two_other, ticks=i32(0, 3), rows=i32(0, 1), batch=2, h=8, w=8, kmat=ptrs(2), upscale=1, ws=fake):
        return L.rpe_surfel_fuse_many(n, src, bounds, dst, ticks, rows, batch, fake, fake, fake, h, w, kmat, ptrs(2), fake, 0.05, 1,
                                      upscale, 7.0, 15, ws, None)
    assert fuse(0, src=None, bounds=None, dst=None, ticks=None, rows=None) == OK
    assert fuse(65) == B
    assert fuse(2, src=None) == B and fuse(2, dst=None) == B and fuse(2, bounds=None) == B
    assert fuse(2, ticks=None) == B and fuse(2, rows=None) == B and fuse(2, kmat=None) == B and fuse(2, ws=None) == B
    assert fuse(2, dst=two) == B                                                        # src == dst
    assert fuse(2, dst=arr(desc(0x4000), desc(0x2000))) == B                            # map 1 writes into map 0's source
    assert fuse(2, src=null_map) == B
    assert fuse(2, bounds=_i64(0, 17)) == B and fuse(2, bounds=_i64(-1, 0)) == B
    assert fuse(2, rows=i32(0, 2)) == B and fuse(2, rows=i32(-1, 0)) == B              # frame rows outside the batch
    assert fuse(2, batch=0) == B and fuse(2, h=0) == B
    assert fuse(2, kmat=ptrs(2, None)) == B
    assert fuse(2, upscale=2) == -3                                                     # RPE_E_UNSUPPORTED, as rpe_surfel_fuse


def test_multi_estimator_construction_and_refusals(tmp_path):
    from rpe_amd import pose_estimator, synth
    from rpe_amd.se3 import SE3
    path, cfg, sd = _checkpoint(tmp_path)
    K = synth.intrinsics(H, W)
    Ks = torch.stack([K, K * 1.01, K])
    est = pose_estimator.MultiSurfelPoseEstimator(_slam(False), Ks, torch.tensor([1800.0, 1700.0, 1600.0]), path, (W, H),
                                                  init_poses=SE3.Identity(3))
    m = est.model
    assert tuple(m.config['image_shape']) == (H, W) and m.config['lbgfs_iters'] == 20
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    assert est.n_seq == 3 and est.scenes == [None] * 3 and est.success == [True] * 3
    assert tuple(est.intrinsics.shape) == (3, 3, 3) and torch.equal(est.baseline, torch.tensor([1800.0, 1700.0, 1600.0]))
    assert torch.equal(est.last_pose[1].data, SE3.Identity(1).data)
    with pytest.raises(ValueError, match='forward_chunk'):
        pose_estimator.MultiSurfelPoseEstimator(_slam(True), Ks, torch.ones(3), path, (W, H))
    with pytest.raises(ValueError, match='baselines'):
        pose_estimator.MultiSurfelPoseEstimator(_slam(False), Ks, torch.ones(2), path, (W, H))
    with pytest.raises(ValueError, match='init_poses'):
        pose_estimator.MultiSurfelPoseEstimator(_slam(False), Ks, torch.ones(3), path, (W, H), init_poses=torch.zeros(2, 7))
    with pytest.raises(ValueError, match='intrinsics'):
        pose_estimator.MultiSurfelPoseEstimator(_slam(False), K, torch.ones(3), path, (W, H))
    with pytest.raises(ValueError, match='1 to 64'):
        pose_estimator.MultiSurfelPoseEstimator(_slam(False), K.expand(65, 3, 3), torch.ones(65), path, (W, H))
    img = torch.zeros(2, 3, H, W)
    with pytest.raises(RuntimeError, match='chunked'):
        est.forward_chunk(img, img, torch.ones(2, 1, H, W, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='pipelined'):
        est.submit(img[:1], img[:1], torch.ones(1, 1, H, W, dtype=torch.bool))
    with pytest.raises(ValueError, match='rows'):
        est(img, img, torch.ones(2, 1, H, W, dtype=torch.bool), rows=[0, 0])
    with pytest.raises(ValueError, match='rows'):
        est(img, img, torch.ones(2, 1, H, W, dtype=torch.bool), rows=[0, 3])


def test_solve_rows_alone_sets_partition_rows_1_and_restores_it():
    """PoseNet._solve on a stand-in pose head (no GPU, no library): ``rows_alone`` solves with partition_rows = 1 and puts the value
    back, also when the solve raises; without it the value is left alone."""
    from types import SimpleNamespace
    from rpe_amd.pose_net import PoseNet
    problem = SimpleNamespace(partition_rows=7)
    seen = []

    def head(*inputs):
        seen.append(problem.partition_rows)
        if inputs[0] == 'raise':
            raise RuntimeError('solve failed')
        return inputs, None
    net = SimpleNamespace(pose_head=head)
    head.problem = problem
    assert PoseNet._solve(net, ('a', 'b'), rows_alone=True) == ('a', 'b') and seen == [1] and problem.partition_rows == 7
    with pytest.raises(RuntimeError, match='solve failed'):
        PoseNet._solve(net, ('raise',), rows_alone=True)
    assert seen == [1, 1] and problem.partition_rows == 7
    assert PoseNet._solve(net, ('c',)) == ('c',) and seen == [1, 1, 7] and problem.partition_rows == 7
