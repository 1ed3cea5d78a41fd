"""GPU: MultiSurfelPoseEstimator (K frame-to-model sequences in lockstep) and trajectory.track_sequences against SurfelPoseEstimator
runs of each sequence alone: bit-identical poses, success flags and maps whichever rows share the batch (different intrinsics,
baselines and lengths, a late start); the reference case as one row of a batch; the scripted gate case beside a passing row;
byte-identical Freiburg files per (start, end) scenario."""
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
H, W = 352, 384
CFG = dict(frame2frame=False, depth_clipping=[1, 250], lbgfs_iters=8, conf_weighing=True, dist_thr=0.05, average_pts=True)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t.view(torch.int32)


def _map_state(m):
    return m.n, m.overflowed, m.tick, _bits(torch.cat((m.opts, m.rgb, m.conf, m.t_created))).cpu()


def _same_state(a, b):
    return a[:3] == b[:3] and torch.equal(a[3], b[3])


@pytest.fixture(scope='module')
def model():
    from rpe_amd import pose_net, synth
    return synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(H, W, iters=12, lbgfs_iters=8))).eval().to(DEV)


def _sequences():
    """Three sequences: own frames, intrinsics and baselines; lengths 4, 3, 3; sequence 2 starts at lockstep step 2."""
    from rpe_amd import synth
    seqs, Ks, bfs = [], [], []
    for k, n in enumerate((4, 3, 3)):
        s = synth.stereo_frames(30 + k, n, H, W)
        seqs.append([(s['image2l'][i:i + 1], s['image2r'][i:i + 1], s['mask2'][i:i + 1]) for i in range(n)])
        Ks.append(s['K'][0] * torch.tensor([[1.0 + 0.02 * k], [1.0 - 0.01 * k], [1.0]]))
        bfs.append(float(s['baseline'][0]) * 250.0 * (1.0 + 0.1 * k))
    return seqs, Ks, bfs, (0, 0, 2)


def test_multi_tracker_matches_single_trackers(rpe, model):
    from rpe_amd import pose_estimator
    seqs, Ks, bfs, starts = _sequences()
    single = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for k, seq in enumerate(seqs):
            est = pose_estimator.SurfelPoseEstimator(CFG, Ks[k], bfs[k], model, (W, H)).to(DEV)
            out = []
            for l, r, m in seq:
                P, scene, _, _ = est(l.to(DEV), r.to(DEV), m.clone().to(DEV))
                out.append((P.data.cpu().clone(), est.success, _map_state(scene)))
            single.append(out)
        multi = pose_estimator.MultiSurfelPoseEstimator(CFG, torch.stack(Ks), torch.tensor(bfs), model, (W, H)).to(DEV)
        got = [[] for _ in seqs]
        for t in range(max(st + len(sq) for st, sq in zip(starts, seqs))):
            rows = [k for k in range(len(seqs)) if starts[k] <= t < starts[k] + len(seqs[k])]
            frames = [seqs[k][t - starts[k]] for k in rows]
            P, ok, scenes, flow, _ = multi(*(torch.cat([f[i] for f in frames]).to(DEV) for i in range(3)), rows=rows)
            assert P.data.shape == (len(rows), 7) and ok.shape == (len(rows),) and flow.shape[0] == len(rows)
            for j, k in enumerate(rows):
                assert scenes[j] is multi.scenes[k] and bool(ok[j]) == multi.success[k]
                assert torch.equal(multi.last_pose[k].data, P.data[j:j + 1])
                got[k].append((P.data[j:j + 1].cpu().clone(), bool(ok[j]), _map_state(scenes[j])))
    for k in range(len(seqs)):
        assert len(got[k]) == len(single[k])
        for i, (a, b) in enumerate(zip(single[k], got[k])):
            assert torch.equal(_bits(a[0]), _bits(b[0])), (k, i, a[0], b[0])
            assert a[1] == b[1], (k, i)
            assert _same_state(a[2], b[2]), (k, i, a[2][:3], b[2][:3])
    assert all(st[2][0] > 0 for out in got for st in out)


def test_reference_case_as_one_row_of_a_batch(rpe):
    """tests/golden/tracker_f2m.npz (the reference's own f2m tracker) as row 0 of a K = 2 batch: the tolerances of
    test_gpu_surfel_map.test_f2m_tracker_matches_reference."""
    from oracle import pose_net as opn, synth as osynth
    from rpe_amd import pose_estimator, pose_net, synth
    from test_gpu_surfel_map import F2M, _mom
    g = dict(np.load(os.path.join(GOLDEN, 'tracker_f2m.npz')))
    cfg, sd, _ = osynth.posenet_case(synth, opn)
    model = pose_net.PoseNet(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.eval().to(DEV)
    frames, K, bf = osynth.tracker_case(synth, n_frames=4)
    other, K2, bf2 = osynth.tracker_case(synth, seed=5, n_frames=4)
    Hm, Wm = osynth.MODULE_HW
    est = pose_estimator.MultiSurfelPoseEstimator(F2M, torch.stack([K, K2]), torch.tensor([bf, bf2]), model, (Wm, Hm)).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i, ((l, r, m), (l2, r2, m2)) in enumerate(zip(frames, other)):
            P, ok, scenes, _, _ = est(torch.cat((l, l2)).to(DEV), torch.cat((r, r2)).to(DEV), torch.cat((m, m2)).to(DEV))
            scene = scenes[0]
            d = float((P.data[0].cpu() - torch.from_numpy(g['abs_poses'][i])).abs().max())
            print(f'f2m row 0 frame {i}: abs pose diff {d:.2e} mm, map {scene.n} surfels (reference {int(g["count"][i])})')
            assert d <= 2e-3
            assert bool(ok[0]) == bool(g['success'][i])
            assert abs(scene.n - int(g['count'][i])) <= 50 * (i + 1)
            got = np.concatenate((_mom(scene.opts), _mom(scene.rgb), _mom(scene.conf)))
            np.testing.assert_allclose(got[:, :2], g['map_mom'][i][:, :2], rtol=2e-3)


class _ScriptedRows(torch.nn.Module):
    """PoseNet stand-in for the gate case, per row: depth 0.25, relative poses rel[row][call] (the rows of each call in order)."""

    def __init__(self, rels):
        super().__init__()
        self.rels, self.i = rels, 0

    def flow2depth(self, l, r, baseline):
        return torch.full_like(l[:, :1], 0.25), torch.zeros_like(l[:, :2]), torch.ones_like(l[:, :1], dtype=torch.bool)

    def infer(self, image1l, image2l, *a, **kw):
        from rpe_amd.se3 import SE3
        p = SE3(torch.stack([rel[self.i] for rel in self.rels]).to(image1l.device))
        self.i += 1
        d = torch.full_like(image1l[:, :1], 0.25)
        return p, d, d, (d, d), torch.zeros_like(image1l[:, :2]), torch.zeros_like(image1l[:, :2])


def test_gate_case_beside_a_passing_row(rpe):
    """Row 0 gets the golden gate case's prescribed relative poses, row 1 small ordinary ones: row 0's flags, poses and map counts are
    the reference's (a failed frame fuses nothing), row 1 fuses every frame."""
    from oracle import synth as osynth
    from rpe_amd import pose_estimator, pose_net, synth
    from rpe_amd.se3 import SE3
    from test_gpu_surfel_map import F2M
    g = dict(np.load(os.path.join(GOLDEN, 'tracker_f2m.npz')))
    _, K, bf = osynth.tracker_case(synth, n_frames=1)
    m = g['gate_rel'].shape[0]
    model = pose_net.PoseNet(synth.model_config(352, 384, iters=2, lbgfs_iters=8))
    est = pose_estimator.MultiSurfelPoseEstimator(F2M, torch.stack([K, K]), torch.tensor([bf, bf]), model, (8, 8)).to(DEV)
    passing = SE3.exp(torch.tensor([[1e-3, 0.0, 0.0, 0.0, 0.0, 0.0]]).repeat(m, 1).to(DEV)).data.cpu()
    est.model = _ScriptedRows([torch.from_numpy(g['gate_rel']), passing])
    tiny = torch.from_numpy(g['gate_tiny']).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i in range(m):
            before = [s.n if s is not None else None for s in est.scenes]
            ticks = [s.tick if s is not None else 0 for s in est.scenes]
            P, ok, scenes, _, _ = est(torch.cat((tiny, tiny)), torch.cat((tiny, tiny)), torch.ones(2, 1, 8, 8, dtype=torch.bool, device=DEV))
            assert bool(ok[0]) == bool(g['gate_success'][i]) and est.success[0] == bool(g['gate_success'][i]), i
            assert scenes[0].n == int(g['gate_count'][i]), i
            if not ok[0]:
                assert scenes[0].n == before[0] and scenes[0].tick == ticks[0], i
            assert bool(ok[1]) and scenes[1].tick == ticks[1] + 1, i
            d = float((P.data[0].cpu() - torch.from_numpy(g['gate_abs'][i])).abs().max())
            assert d <= 1e-5 * max(1.0, float(np.abs(g['gate_abs'][i]).max())), (i, d)
    assert not all(bool(v) for v in g['gate_success'])                    # the case does fail frames


def test_track_sequences_writes_the_files_of_single_runs(rpe, model, tmp_path):
    """The (start, end) scenarios of one recording, as scripts/benchmark_test.py runs them: each with its own initial pose, of different
    lengths and overlapping.  Every Freiburg file is byte-identical to the track_sequence run of that scenario alone."""
    from rpe_amd import pose_estimator, synth, trajectory
    from rpe_amd.se3 import SE3
    s = synth.stereo_frames(17, 7, H, W)
    K, bf = s['K'][0], float(s['baseline'][0]) * 250.0
    scenarios = [(0, 5), (2, 7), (3, 5)]
    inits = SE3.exp(torch.tensor([[0.0] * 6, [1.0, -2.0, 0.5, 0.01, 0.0, -0.02], [0.0, 3.0, 0.0, 0.0, 0.03, 0.0]]).to(DEV)).data.cpu()

    def frames(a, b):
        return [(s['image2l'][i:i + 1].to(DEV), s['image2r'][i:i + 1].to(DEV), s['mask2'][i:i + 1].clone().to(DEV), 100 + i) for i in range(a, b)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        single = []
        for j, (a, b) in enumerate(scenarios):
            est = pose_estimator.SurfelPoseEstimator(CFG, K, bf, model, (W, H), init_pose=SE3(inits[j:j + 1])).to(DEV)
            d = tmp_path / f'single{j}'
            d.mkdir()
            single.append(open(trajectory.save_trajectory(trajectory.track_sequence(est, frames(a, b), start_stamp=99 + a), str(d))).read())
        multi = pose_estimator.MultiSurfelPoseEstimator(CFG, K.expand(3, 3, 3), torch.tensor([bf] * 3), model, (W, H), init_poses=inits).to(DEV)
        trajs = trajectory.track_sequences(multi, [frames(a, b) for a, b in scenarios], start_stamps=[99 + a for a, _ in scenarios])
    for j, (a, b) in enumerate(scenarios):
        d = tmp_path / f'multi{j}'
        d.mkdir()
        text = open(trajectory.save_trajectory(trajs[j], str(d))).read()
        assert len(text.splitlines()) == b - a + 1
        assert text == single[j], j
