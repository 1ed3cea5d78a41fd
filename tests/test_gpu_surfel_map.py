"""GPU: the rpe_surfel_* kernels through SurfelMap against the reference's own surfel_map.py (tests/golden/surfel_map.npz) and against
the plain-torch restatement (tests/surfel_ref.py) at 640x512; capacity growth, run-to-run determinism, the frame-to-model tracker's
fuse-only-on-success and an end-to-end track_sequence + save_ply."""
import hashlib
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import surfel_ref as sr

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CASES = {'a': dict(d_thresh=3.0, average_pts=True, t_max=15), 'b': dict(d_thresh=0.05, average_pts=False, t_max=6)}


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(GOLDEN, 'surfel_map.npz')))


def _sha(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _mom(t):
    t = torch.nan_to_num(t.detach().cpu().double(), nan=0.0, posinf=0.0, neginf=0.0)
    return torch.stack((t.sum(-1), t.abs().sum(-1), (t * t).sum(-1)), dim=-1).numpy()


def _frame(img, depth, mask, conf=None):
    from rpe_amd.pose_estimator import Frame
    return Frame(img.to(DEV), depth=depth.to(DEV), mask=mask.to(DEV), confidence=None if conf is None else conf.to(DEV))


def _run(K, frames, poses, steps, capacity=None, **kw):
    from rpe_amd.se3 import SE3
    from rpe_amd.surfel_map import SurfelMap
    img, depth, mask, conf = frames[0]
    m = SurfelMap(frame=_frame(img, depth, mask, conf), kmat=K.to(DEV), pmat=SE3(poses[0].reshape(1, 7).to(DEV)), upscale=1,
                  capacity=capacity, **kw)
    yield 0, m
    for s in range(1, steps + 1):
        img, depth, mask, _ = frames[s]
        m.fuse(_frame(img, depth, mask), SE3(poses[s].reshape(1, 7).to(DEV)))
        yield s, m


@pytest.mark.parametrize('case', ['a', 'b'])
def test_surfel_map_matches_reference_golden(rpe, gold, case):
    from rpe_amd import synth
    K, frames = synth.surfel_scene(32, 48, 20)
    poses = torch.from_numpy(gold['poses'])
    for s, m in _run(K, frames, poses, 20, **CASES[case]):
        assert m.n == gold[f'{case}_count'][s], s
        assert _sha(m.conf) + _sha(m.t_created) == gold[f'{case}_sha'][s], s       # conf, t_created, kept set and order: bit for bit
        np.testing.assert_allclose(np.concatenate((_mom(m.opts), _mom(m.rgb))), gold[f'{case}_mom'][s], rtol=1e-5)
        if f'{case}_opts{s}' in gold:
            np.testing.assert_allclose(m.opts.cpu().numpy(), gold[f'{case}_opts{s}'], rtol=1e-5, atol=1e-5 * 60)
            np.testing.assert_allclose(m.rgb.cpu().numpy(), gold[f'{case}_rgb{s}'], rtol=1e-5, atol=1e-5 * 255)
    assert m.overflowed == 0 and m.tick == 20


def _render_gpu(g, K, key):
    from rpe_amd.se3 import SE3
    from rpe_amd.surfel_map import SurfelMap
    m = SurfelMap(opts=torch.from_numpy(g['r_opts']).to(DEV), rgb=torch.from_numpy(g['r_rgb']).to(DEV),
                  conf=torch.from_numpy(g['r_conf']).to(DEV), kmat=K.to(DEV), img_shape=(32, 48))
    T = SE3(torch.from_numpy(g['T1' if key == '_cpy' else f'T{key}']).reshape(1, 7).to(DEV))
    fr = m.render_transformed(K.to(DEV), T)[0] if key == '_cpy' else m.render(K.to(DEV), T)[0]
    return fr.img[0].cpu(), fr.depth[0, 0].cpu(), fr.confidence[0, 0].cpu(), fr.mask[0, 0].cpu()


@pytest.mark.parametrize('case', ['a', 'b'])
def test_surfel_render_matches_reference_golden(rpe, gold, case):
    g = {k[2:]: v for k, v in gold.items() if k.startswith(case + '_')}
    K = torch.from_numpy(gold['K'])
    opts, rgb, conf = (torch.from_numpy(g[k]) for k in ('r_opts', 'r_rgb', 'r_conf'))
    for key in (0, 1, 2, '_cpy'):
        img, depth, confidence, mask = _render_gpu(g, K, key)
        T = torch.from_numpy(g['T1' if key == '_cpy' else f'T{key}'])
        rimg, rdepth, rconf, rmask, winner, tied = sr.render(opts, rgb, conf, K, T, (32, 48), key == '_cpy')
        free = ~tied.reshape(32, 48)
        # the golden, where the reference's pixel had one largest conf
        gi, gd = torch.from_numpy(g[f'img{key}'][0]), torch.from_numpy(g[f'depth{key}'][0, 0])
        assert torch.equal(confidence, torch.from_numpy(g[f'rconf{key}'][0, 0])), key
        assert torch.equal(mask, torch.from_numpy(g[f'rmask{key}'][0, 0])), key
        assert torch.allclose(depth[free], gd[free], rtol=1e-5, atol=0), key
        # everywhere, ties included: the documented rule (largest conf, ties to the largest index) as the restatement applies it
        assert torch.equal(confidence, rconf) and torch.equal(mask, rmask), key
        filled = torch.isnan(rgb[:, winner.clamp(min=0)]).reshape(3, 32, 48) & (winner >= 0).reshape(1, 32, 48)
        assert torch.equal(img[~filled], rimg[~filled]), key
        assert torch.allclose(img[filled], rimg[filled], rtol=1e-5, atol=1e-5), key
        assert torch.allclose(depth, rdepth, rtol=1e-5, atol=0), key
        calm = ~torch.nn.functional.max_pool2d((~free)[None, None].float(), 5, 1, 2)[0, 0].bool()
        assert torch.equal(img[:, free][~filled[:, free]], gi[:, free][~filled[:, free]]), key
        fill = filled & calm[None]
        assert torch.allclose(img[fill], gi[fill], rtol=1e-5, atol=1e-5), key
        print(f'case {case} render {key}: {int(tied.sum())} tied pixels, {int(filled.sum())} NaN-filled values ({int(fill.sum())} vs golden)')
        if case == 'b':
            assert int(tied.sum()) <= 0.01 * tied.numel(), key          # case b's distinct confidences: the golden pins nearly every pixel


def _ambiguous(ref, depth, mask, pose, d_thresh):
    """Surfels whose association the f32 rounding order could flip: within 1e-4 px of a pixel / image-border boundary or within 1e-6
    relative of d_thresh."""
    h, w = depth.shape[-2:]
    flags, pix, fopts, u, v, diff = ref.associate(depth, mask, pose)
    near = torch.zeros_like(flags)
    for c, lim in ((u, w - 1), (v, h - 1)):
        frac = (c - 0.5) - torch.floor(c - 0.5)
        near |= (frac - 0.5).abs() < 1e-4
        near |= (c.abs() < 1e-4) | ((c - lim).abs() < 1e-4)
    inb = (u >= 0) & (v >= 0) & (u < w - 1) & (v < h - 1)
    dd = torch.zeros_like(u)
    dd[inb] = diff.abs()
    near |= inb & ((dd - d_thresh).abs() <= 1e-6 * d_thresh)
    return near


@pytest.mark.parametrize('average', [False, True])
def test_surfel_map_matches_restatement_full_size(rpe, average):
    """640x512, 20 frames, a map of up to ~2.7 M surfels (the compaction scan runs over > 1024 blocks): every step restarts the
    restatement from the device map, so a differing decision cannot cascade.  Counts, t_created, the kept set and its order must be
    identical every step; conf may differ only at old surfels whose association a rounding could flip (``_ambiguous``), and those
    are counted and bounded."""
    from rpe_amd import synth
    from oracle import se3 as ose3
    H, W = 512, 640
    K, frames = synth.surfel_scene(H, W, 20, seed=11)
    poses = [ose3.se3_exp(synth.surfel_pose(k, 0.5)).reshape(7) for k in range(21)]
    kw = dict(d_thresh=0.5, average_pts=average, t_max=8)
    ref = None
    differing, largest = 0, 0
    for s, m in _run(K, frames, poses, 20, **kw):
        if ref is not None:
            img, depth, mask, _ = frames[s]
            amb = _ambiguous(ref, depth, mask, poses[s], kw['d_thresh'])
            n_old = ref.opts.shape[1]
            largest = max(largest, n_old + H * W)
            ref.fuse(img, depth, mask, poses[s])
            assert m.n == ref.opts.shape[1], f'step {s}: {m.n} surfels on the device, {ref.opts.shape[1]} in the restatement'
            assert torch.equal(m.t_created.cpu(), ref.t_created), f'step {s}: kept set / order differs'
            diff = torch.nonzero((m.conf.cpu() != ref.conf)[0]).reshape(-1)
            if diff.numel():
                old_kept = torch.nonzero(ref.last_keep[:n_old]).reshape(-1)
                assert bool((diff < old_kept.numel()).all()), f'step {s}: an appended surfel differs'
                assert bool(amb[old_kept[diff]].all()), f'step {s}: {diff.numel()} differing decisions, not all near a rounding boundary'
                differing += diff.numel()
            same = torch.ones(m.n, dtype=torch.bool)
            same[diff] = False
            assert torch.allclose(m.opts.cpu()[:, same], ref.opts[:, same], rtol=1e-5, atol=1e-4)
            assert torch.allclose(m.rgb.cpu()[:, same], ref.rgb[:, same], rtol=1e-5, atol=1e-3)
        ref = sr.RefMap(K, frames[0][0], frames[0][1], frames[0][2], frames[0][3], poses[0], conf_thr=7, **kw)
        ref.opts, ref.rgb, ref.conf, ref.t_created = (t.cpu().clone() for t in (m.opts, m.rgb, m.conf, m.t_created))
        ref.tick = m.tick
    print(f'average_pts={average}: final map {m.n} surfels, largest compaction {largest} items, {differing} differing decisions over 20 fuses')
    assert largest > 1024 * 1024                      # more than 1024 scan blocks of 1024 items
    assert differing <= 20
    assert m.overflowed == 0


def test_capacity_growth_and_determinism(rpe, gold):
    from rpe_amd import synth
    from rpe_amd.se3 import SE3
    K, frames = synth.surfel_scene(32, 48, 20)
    poses = torch.from_numpy(gold['poses'])

    def final(capacity):
        for s, m in _run(K, frames, poses, 20, capacity=capacity, **CASES['b']):
            pass
        fr = m.render_transformed(K.to(DEV), SE3(poses[20].reshape(1, 7).to(DEV)).inv())[0]
        return m, torch.cat((m.opts, m.rgb, m.conf, m.t_created)).cpu(), torch.cat((fr.img[0], fr.depth[0], fr.confidence[0])).cpu()

    small, a_map, a_img = final(None)                  # starts at h*w: grows several times (case b reaches ~7000 surfels)
    big, b_map, b_img = final(1 << 16)
    _, c_map, c_img = final(1 << 16)
    assert small.capacity < big.capacity and small.capacity >= 7135
    for x, y in ((a_map, b_map), (b_map, c_map), (a_img, b_img), (b_img, c_img)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


class _Scripted(torch.nn.Module):
    """Stands in for PoseNet as tools/gen_surfel_golden.py's gate case does: depth 0.25 (62.5 mm), prescribed relative poses."""

    def __init__(self, rel):
        super().__init__()
        self.rel, self.i = rel, 0

    def flow2depth(self, l, r, baseline):
        return torch.full_like(l[:, :1], 0.25), torch.zeros_like(l[:, :2]), torch.ones_like(l[:, :1], dtype=torch.bool)

    def infer(self, image1l, image2l, *a, **kw):
        from rpe_amd.se3 import SE3
        p = SE3(self.rel[self.i:self.i + 1].to(image1l.device))
        self.i += 1
        d = torch.full_like(image1l[:, :1], 0.25)
        return p, d, d, (d, d), torch.zeros_like(image1l[:, :2]), torch.zeros_like(image1l[:, :2])


F2M = dict(frame2frame=False, dist_thr=0.05, depth_clipping=[1, 250], lbgfs_iters=8, conf_weighing=True, average_pts=True)


def test_f2m_tracker_matches_reference(rpe):
    """The reference's PoseEstimator(frame2frame=False) with its own surfel map (tests/golden/tracker_f2m.npz): absolute poses within
    the 2e-3 mm of the f2f tracker test, identical success flags, map counts within the 50 stereo-mask pixels per frame it allows."""
    from oracle import pose_net as opn, synth as osynth
    from rpe_amd import pose_estimator, pose_net, synth
    g = dict(np.load(os.path.join(GOLDEN, 'tracker_f2m.npz')))
    cfg, sd, _ = osynth.posenet_case(synth, opn)
    model = pose_net.PoseNet(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.eval().to(DEV)
    frames, K, bf = osynth.tracker_case(synth, n_frames=4)
    H, W = osynth.MODULE_HW
    est = pose_estimator.SurfelPoseEstimator(F2M, K, bf, model, (W, H)).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i, (l, r, m) in enumerate(frames):
            P, scene, flow, weights = est(l.to(DEV), r.to(DEV), m.clone().to(DEV))
            d = float((P.data.cpu().reshape(7) - torch.from_numpy(g['abs_poses'][i])).abs().max())
            print(f'f2m frame {i}: abs pose diff {d:.2e} mm, map {scene.n} surfels (reference {int(g["count"][i])})')
            assert d <= 2e-3
            assert est.success == bool(g['success'][i])
            assert abs(scene.n - int(g['count'][i])) <= 50 * (i + 1)
            got = np.concatenate((_mom(scene.opts), _mom(scene.rgb), _mom(scene.conf)))
            np.testing.assert_allclose(got[:, :2], g['map_mom'][i][:, :2], rtol=2e-3)           # sums and absolute sums


def test_f2m_gate_case_matches_reference(rpe):
    """Prescribed relative poses through the tracker (the gate case of tracker.npz): the chained poses, the success flags and the map
    count after every frame -- a failed frame fuses nothing."""
    from oracle import synth as osynth
    from rpe_amd import pose_estimator, pose_net, synth
    g = dict(np.load(os.path.join(GOLDEN, 'tracker_f2m.npz')))
    _, K, bf = osynth.tracker_case(synth, n_frames=1)                  # the estimator the reference's gate case reused
    model = pose_net.PoseNet(synth.model_config(352, 384, iters=2, lbgfs_iters=8))
    est = pose_estimator.SurfelPoseEstimator(F2M, K, bf, model, (8, 8)).to(DEV)
    est.model = _Scripted(torch.from_numpy(g['gate_rel']))
    tiny = torch.from_numpy(g['gate_tiny']).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i in range(g['gate_rel'].shape[0]):
            before = est.scene.n if est.scene is not None else None
            P, scene, _, _ = est(tiny.clone(), tiny.clone(), torch.ones(1, 1, 8, 8, dtype=torch.bool, device=DEV))
            assert est.success == bool(g['gate_success'][i]), i
            assert scene.n == int(g['gate_count'][i]), i
            if not est.success:
                assert scene.n == before
            d = float((P.data.cpu().reshape(7) - torch.from_numpy(g['gate_abs'][i])).abs().max())
            assert d <= 1e-5 * max(1.0, float(np.abs(g['gate_abs'][i]).max())), (i, d)


def test_f2m_track_sequence_and_save_ply(rpe, tmp_path):
    from rpe_amd import pose_estimator, pose_net, synth, trajectory
    h, w = 352, 384
    cfg = dict(frame2frame=False, depth_clipping=[1, 250], lbgfs_iters=8, conf_weighing=True, dist_thr=0.05, average_pts=True)
    model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(h, w, iters=12, lbgfs_iters=8)))
    s = synth.stereo_frames(9, 3, h, w)
    est = pose_estimator.from_config(cfg, s['K'][0], float(s['baseline'][0]) * 250.0, model, (w, h)).to(DEV)
    frames = [(s['image2l'][i:i + 1].to(DEV), s['image2r'][i:i + 1].to(DEV), s['mask2'][i:i + 1].to(DEV), i) for i in range(3)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        traj = trajectory.track_sequence(est, frames, chunk=1)
    assert len(traj) == 4 and all(bool(torch.isfinite(t['camera-pose']).all()) for t in traj)
    fn = trajectory.save_trajectory(traj, str(tmp_path))
    assert len(open(fn).read().splitlines()) == 4
    assert est.scene.n > 0 and est.scene.overflowed == 0
    est.scene.save_ply(str(tmp_path / 'all_map.ply'), stable=False)
    head = open(tmp_path / 'all_map.ply').read().splitlines()
    assert head[0] == 'ply' and int(head[2].split()[-1]) > 0
