"""CPU: MultiPoseEstimator's construction and refusals, from_config_many's dispatch, trajectory.track_sequences' bookkeeping on a stub
estimator (ragged lengths, stamps, the quality flag), and ``forward``'s own bookkeeping on a scripted model with the three kernels it
launches restated on the host: what each sequence is fed, and gets, is what a PoseEstimator of its own is fed and gets."""
import pytest
import torch

H, W = 128, 160
F2F = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=8, conf_weighing=True)
F2M = dict(F2F, frame2frame=False, dist_thr=0.05, average_pts=True)


@pytest.fixture(scope='module')
def model():
    from rpe_amd import pose_net, synth
    return pose_net.PoseNet(synth.model_config(H, W, iters=2, lbgfs_iters=8))


@pytest.fixture(scope='module')
def Ks():
    from rpe_amd import synth
    K = synth.intrinsics(H, W)
    return torch.stack([K, K * 1.01, K])


def test_construction(model, Ks):
    from rpe_amd import pose_estimator
    from rpe_amd.se3 import SE3
    bl = torch.tensor([1800.0, 1700.0, 1600.0])
    est = pose_estimator.MultiPoseEstimator(dict(F2F, warm_start=True, report_quality=True), Ks, bl, model, (W, H), init_poses=SE3.Identity(3))
    assert isinstance(est, pose_estimator.PoseEstimator) and est.model is model
    assert est.n_seq == 3 and est.success == [True] * 3 and est.warm_start and est.report_quality and est.last_quality is None
    assert tuple(est.intrinsics.shape) == (3, 3, 3) and torch.equal(est.baseline, bl)
    assert all(torch.equal(est.last_pose[k].data, SE3.Identity(1).data) for k in range(3))
    inits = torch.tensor([[1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], [4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
    est = pose_estimator.MultiPoseEstimator(F2F, Ks, bl, model, (W, H), init_poses=inits)
    assert all(torch.equal(est.last_pose[k].data, inits[k:k + 1]) for k in range(3))
    est.last_pose[2] = SE3.Identity(1)
    est.success[0] = est.success[2] = False
    est.reset([2])
    assert torch.equal(est.last_pose[2].data, inits[2:3]) and est.success == [False, True, True]
    assert est.reset() is est and est.success == [True] * 3


def test_constructor_refusals(model, Ks):
    from rpe_amd import pose_estimator
    M = pose_estimator.MultiPoseEstimator
    with pytest.raises(ValueError, match='MultiSurfelPoseEstimator'):
        M(F2M, Ks, torch.ones(3), model, (W, H))
    with pytest.raises(ValueError, match='baselines'):
        M(F2F, Ks, torch.ones(2), model, (W, H))
    with pytest.raises(ValueError, match='init_poses'):
        M(F2F, Ks, torch.ones(3), model, (W, H), init_poses=torch.zeros(2, 7))
    with pytest.raises(ValueError, match='intrinsics'):
        M(F2F, Ks[0], torch.ones(3), model, (W, H))
    with pytest.raises(ValueError, match='intrinsics'):
        M(F2F, torch.zeros(3, 3, 4), torch.ones(3), model, (W, H))
    with pytest.raises(ValueError, match='1 to 64'):
        M(F2F, Ks[:1].expand(65, 3, 3), torch.ones(65), model, (W, H))
    with pytest.raises(ValueError, match='1 to 64'):
        M(F2F, torch.zeros(0, 3, 3), torch.ones(0), model, (W, H))
    assert pose_estimator.MULTI_MAX_SEQUENCES == 64
    assert M(F2F, Ks[:1].expand(64, 3, 3), torch.ones(64), model, (W, H)).n_seq == 64


def test_from_config_many_picks_the_class(model, Ks):
    from rpe_amd import pose_estimator
    f2f = pose_estimator.from_config_many(F2F, Ks, torch.ones(3), model, (W, H))
    assert type(f2f) is pose_estimator.MultiPoseEstimator and f2f.n_seq == 3
    f2f = pose_estimator.from_config_many({k: v for k, v in F2F.items() if k != 'frame2frame'}, Ks, torch.ones(3), model, (W, H))
    assert type(f2f) is pose_estimator.MultiPoseEstimator                  # (frame2frame defaults to True, as in from_config)
    inits = torch.tensor([[0.0, 0.0, float(k), 0.0, 0.0, 0.0, 1.0] for k in range(3)])
    f2m = pose_estimator.from_config_many(F2M, Ks, torch.ones(3), model, (W, H), init_poses=inits)
    assert type(f2m) is pose_estimator.MultiSurfelPoseEstimator and torch.equal(f2m.last_pose[2].data, inits[2:3])
    f2f = pose_estimator.from_config_many(F2F, Ks, torch.ones(3), model, (W, H), inits)
    assert torch.equal(f2f.last_pose[1].data, inits[1:2])


def test_rows_validation_and_refused_modes(model, Ks):
    from rpe_amd import pose_estimator
    est = pose_estimator.MultiPoseEstimator(F2F, Ks, torch.ones(3), model, (W, H))
    img, mask = torch.zeros(2, 3, H, W), torch.ones(2, 1, H, W, dtype=torch.bool)
    for rows in ([0, 0], [0, 3], [-1, 0], []):
        with pytest.raises(ValueError, match='rows'):
            est(img[:len(rows)], img[:len(rows)], mask[:len(rows)], rows=rows)
    with pytest.raises(ValueError, match='3 rows need 3 images'):
        est(img, img, mask)                                                # rows defaults to every sequence
    with pytest.raises(ValueError, match='2 rows need 2 images'):
        est(img, img[:1], mask, rows=[2, 0])
    with pytest.raises(ValueError, match='2 rows need 2 images'):
        est(img, img, mask[:1], rows=[2, 0])
    with pytest.raises(RuntimeError, match='chunked'):
        est.forward_chunk(img, img, mask)
    with pytest.raises(RuntimeError, match='pipelined'):
        est.submit(img[:1], img[:1], mask[:1])
    with pytest.raises(RuntimeError, match='without a submitted frame'):
        est.result()


class _Stub:
    """Stands in for a lockstep tracker: sequence k's pose after its i-th frame has translation (k, i, batch size of the call)."""

    def __init__(self, n, report_quality=False):
        from rpe_amd.se3 import SE3
        self.n_seq, self.report_quality, self.device = n, report_quality, torch.device('cpu')
        self.last_pose = [SE3(torch.tensor([[10.0 * k, 0, 0, 0, 0, 0, 1]])) for k in range(n)]
        self.count, self.calls, self.last_quality = [0] * n, [], None

    def __call__(self, limgs, rimgs, masks, rows=None):
        from rpe_amd import pose_estimator
        from rpe_amd.se3 import SE3
        assert limgs.shape[0] == rimgs.shape[0] == masks.shape[0] == len(rows)
        self.calls.append((list(rows), [int(v) for v in limgs[:, 0, 0, 0]]))
        out = []
        for k in rows:
            self.count[k] += 1
            out.append([float(k), float(self.count[k]), float(len(rows)), 0, 0, 0, 1])
        if self.report_quality:
            self.last_quality = pose_estimator.blank_quality(len(rows), self.device)
            self.last_quality['pd'] = torch.tensor([100.0 * k + self.count[k] for k in rows], dtype=torch.float64)
        return SE3(torch.tensor(out)), torch.ones(len(rows), dtype=torch.bool), None, None


def _frames(k, n):
    """n frames of sequence k; pixel (0,0,0) of the left image carries 100 k + i."""
    return [(torch.full((1, 3, 2, 2), 100.0 * k + i), torch.zeros(1, 3, 2, 2), torch.ones(1, 1, 2, 2, dtype=torch.bool), 1000 * k + i)
            for i in range(n)]


def test_track_sequences_bookkeeping_with_ragged_lengths():
    from rpe_amd import trajectory
    est = _Stub(4)
    lengths = (3, 1, 0)                                                    # (fewer sequences than the estimator has rows is fine)
    trajs = trajectory.track_sequences(est, [_frames(k, n) for k, n in enumerate(lengths)], start_stamps=[7, 8, 9])
    assert est.calls == [([0, 1], [0, 100]), ([0], [1]), ([0], [2])]       # a sequence that ends drops out of rows; frames in row order
    assert [len(t) for t in trajs] == [4, 2, 1]
    assert [[it['timestamp'] for it in t] for t in trajs] == [[7, 0, 1, 2], [8, 1000], [9]]
    assert [it['camera-pose'][:3].tolist() for it in trajs[0]] == [[0, 0, 0], [0, 1, 2], [0, 2, 1], [0, 3, 1]]
    assert [it['camera-pose'][:3].tolist() for it in trajs[1]] == [[10, 0, 0], [1, 1, 2]]
    assert trajs[2][0]['camera-pose'].tolist() == [20, 0, 0, 0, 0, 0, 1] and all('quality' not in it for t in trajs for it in t)
    assert trajectory.track_sequences(_Stub(2), [_frames(0, 1), _frames(1, 2)])[1][0]['timestamp'] == 0     # stamps default to 0
    with pytest.raises(ValueError, match='3 sequences for an estimator of 2'):
        trajectory.track_sequences(_Stub(2), [_frames(k, 1) for k in range(3)])
    with pytest.raises(ValueError, match='start stamps'):
        trajectory.track_sequences(_Stub(2), [_frames(k, 1) for k in range(2)], start_stamps=[0])


def test_track_sequences_quality_rows_follow_the_rows_of_each_call():
    import math
    from rpe_amd import trajectory
    with pytest.raises(ValueError, match='report_quality'):
        trajectory.track_sequences(_Stub(2), [_frames(0, 1)], quality=True)
    trajs = trajectory.track_sequences(_Stub(3, report_quality=True), [_frames(0, 1), _frames(1, 3), _frames(2, 2)], quality=True)
    for k, t in enumerate(trajs):
        assert float(t[0]['quality']['pd']) == 0.0 and math.isnan(float(t[0]['quality']['cov'][0, 0]))      # the initial pose: no solve
        assert [float(it['quality']['pd']) for it in t[1:]] == [100.0 * k + i for i in range(1, len(t))]
        assert all(tuple(it['quality']['cov'].shape) == (6, 6) for it in t)


# ------------------------------------------------------------------------------------------------ forward's bookkeeping, without a GPU
class _Scripted(torch.nn.Module):
    """PoseNet stand-in: every map is the frame's id (pixel (0,0,0) of its left image), so each row of an ``infer`` call can be logged
    as (id of frame 1, id of frame 2, what arrived as depth1 / stereo_flow1 / cached features / flow_init / intrinsics / baseline).  The
    relative pose is a translation of id2 / 1000 along x, or 1 (far past the gate) for the ids in ``reject``."""
    use_weights = True

    def __init__(self, reject=()):
        super().__init__()
        self.reject, self.log, self.first = set(reject), [], []

    def flow2depth(self, l, r, baseline, ret_cache=False):
        ids = l[:, :1, :1, :1]
        self.first.append([int(v) for v in ids.flatten()])
        return l[:, :1] * 2, l[:, :2] * 3, torch.ones_like(l[:, :1], dtype=torch.bool), dict(fmap=ids * 5, cnet=ids * 7)

    def infer(self, image1l, image2l, intrinsics, baseline, depth1, image2r, mask1, mask2, stereo_flow1, ret_details=False, cache1=None,
              ret_cache=False, flow_init=None, ret_lowres=False, ret_quality=False, rows_alone=False):
        from rpe_amd import pose_estimator
        from rpe_amd.se3 import SE3
        n = image1l.shape[0]
        ids = image2l[:, :1, :1, :1]
        assert ret_details and ret_cache and cache1 is not None and intrinsics.shape[0] == baseline.shape[0] == n
        assert flow_init is None or flow_init.shape[0] == n
        self.log.append([(int(image1l[i, 0, 0, 0]), int(ids[i]), float(depth1[i, 0, 0, 0]), float(stereo_flow1[i, 0, 0, 0]),
                          float(cache1['fmap'][i]), float(cache1['cnet'][i]), 0.0 if flow_init is None else float(flow_init[i, 0, 0, 0]),        # (a zero start IS the cold pass)
                          float(intrinsics[i, 0, 0]), float(baseline[i]), bool(mask1[i].all()), rows_alone or n == 1) for i in range(n)])
        mask2[:, :, 0, 0] = False                                          # (`mask2 &= valid` in place)
        rel = torch.zeros(n, 7)
        rel[:, 6] = 1.0
        rel[:, 0] = torch.tensor([1.0 if int(v) in self.reject else int(v) / 1000.0 for v in ids.flatten()])
        out = (SE3(rel), depth1, image2l[:, :1] * 2, (image2l[:, :1] * 0 + 0.5,) * 2, image2l[:, :2] * 11, image2l[:, :2] * 3)
        if ret_quality:
            q = pose_estimator.blank_quality(n, image1l.device)
            q['pd'] = ids.flatten().double()
            out = (*out, q)
        cache = dict(fmap=ids * 5, cnet=ids * 7)
        if ret_lowres:
            cache['time_flow_low'] = image2l[:, :2, :1, :1] * 13
        return (*out, cache)


def _host_ops(monkeypatch):
    """The three kernels the trackers' own code launches, restated for pure translations on the host."""
    from rpe_amd import ops

    def gate_rows(rel, init, scale, thr=0.1):
        rel, init = rel.reshape(-1, 7), init.reshape(-1, 7)
        ok = (rel[:, :3].norm(dim=1) <= thr)
        rel_g = torch.where(ok[:, None], rel, torch.tensor([0.0, 0, 0, 0, 0, 0, 1]))
        pose = init.clone()
        pose[:, :3] -= rel_g[:, :3] * scale
        return rel_g, pose, ok.int()
    monkeypatch.setattr(ops, 'pose_gate_chain_rows', gate_rows)
    monkeypatch.setattr(ops, 'pose_gate_chain', lambda rel, init, scale, thr=0.1: gate_rows(rel, init.reshape(1, 7), scale, thr))
    monkeypatch.setattr(ops, 'forward_interpolate', lambda f: torch.where(f == 0, f, f + 0.25))


def _frame(k, i):
    return torch.full((1, 3, 4, 4), 10.0 * k + i + 1), torch.zeros(1, 3, 4, 4), torch.ones(1, 1, 4, 4, dtype=torch.bool)


@pytest.mark.parametrize('opts', [{}, dict(warm_start=True), dict(report_quality=True), dict(warm_start=True, report_quality=True)])
def test_forward_feeds_each_sequence_what_its_own_tracker_would(monkeypatch, model, opts):
    """Three sequences over a schedule with every kind of call: all rows new, all tracked, a subset, rows out of order, a first frame
    beside tracked rows, a rejected row (sequence 1's frame 2) and a reset of one sequence.  Per sequence, the rows its frames make in
    the stand-in's log, the poses, flags, flow and quality rows are those of a PoseEstimator fed the same frames alone."""
    import warnings
    from rpe_amd import pose_estimator, synth
    _host_ops(monkeypatch)
    cfg = dict(F2F, **opts)
    K = synth.intrinsics(4, 4)
    Ks = torch.stack([K, K * 2, K * 3])
    bl = [1000.0, 2000.0, 3000.0]
    reject = {10 * 1 + 2 + 1}
    #           call: rows (the next frame of each)
    schedule = [[0, 1], [0, 1], [1, 0, 2], [2], [0, 1, 2], 'reset 0', [0, 1, 2], [2, 0]]
    single = {}
    frames_of = {0: 4, 1: 5, 2: 5}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for k in range(3):
            stub = _Scripted(reject)
            est = pose_estimator.PoseEstimator(cfg, Ks[k], bl[k], model, (4, 4))
            est.model = stub
            out, n_before_reset = [], 4
            for i in range(frames_of[k] + (2 if k == 0 else 0)):
                if k == 0 and i == n_before_reset:
                    est.reset()
                l, r, m = _frame(k, i)
                P, _, flow, w = est(l, r, m)
                out.append(dict(P=P.data.clone(), ok=est.success, flow=flow, w=w, m=m, q=est.last_quality))
            single[k] = (out, [row for call in stub.log for row in call])
        stub = _Scripted(reject)
        multi = pose_estimator.MultiPoseEstimator(cfg, Ks, torch.tensor(bl), model, (4, 4))
        multi.model = stub
        nxt, got = [0, 0, 0], {k: [] for k in range(3)}
        for step in schedule:
            if step == 'reset 0':
                multi.reset([0])
                continue
            fr = [_frame(k, nxt[k]) for k in step]
            l, r, m = (torch.cat([f[i] for f in fr]) for i in range(3))
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter('always')
                P, ok, flow, w = multi(l, r, m, rows=step)
            assert len(caught) == int((~ok).sum())                        # one warning per rejected row
            assert P.data.shape == (len(step), 7) and ok.dtype == torch.bool and flow.shape == (len(step), 2, 4, 4)
            assert w[0].shape == w[1].shape == (len(step), 1, 4, 4)
            for j, k in enumerate(step):
                q = None if multi.last_quality is None else {key: v[j:j + 1] for key, v in multi.last_quality.items()}
                got[k].append(dict(P=P.data[j:j + 1], ok=bool(ok[j]), flow=flow[j:j + 1], w=(w[0][j:j + 1], w[1][j:j + 1]), m=m[j:j + 1], q=q))
                assert multi.success[k] == bool(ok[j]) and torch.equal(multi.last_pose[k].data, P.data[j:j + 1])
                nxt[k] += 1
    assert stub.first == [[1, 11], [21], [5]]                            # one flow2depth per call that has first frames, for those rows only
    assert [len(c) for c in stub.log] == [2, 2, 1, 3, 2, 2]                  # one pass per call over its tracked rows
    rows_of = {k: [row for call in stub.log for row in call if row[1] // 10 == k] for k in range(3)}
    for k in range(3):
        want, want_rows = single[k]
        assert rows_of[k] == want_rows, k
        assert len(got[k]) == len(want)
        for i, (a, b) in enumerate(zip(want, got[k])):
            assert torch.equal(a['P'], b['P']) and a['ok'] == b['ok'] and torch.equal(a['m'], b['m']), (k, i)
            if a['flow'] is None:                                          # a first frame: zeros in the batched tracker
                assert not b['flow'].any() and not b['w'][0].any() and not b['w'][1].any(), (k, i)
            else:
                assert torch.equal(a['flow'], b['flow']) and torch.equal(a['w'][0], b['w'][0]) and torch.equal(a['w'][1], b['w'][1]), (k, i)
            assert (a['q'] is None) == (b['q'] is None) == ('report_quality' not in opts)
            if a['q'] is not None:
                assert sorted(a['q']) == sorted(b['q'])
                for key in a['q']:
                    assert a['q'][key].dtype == b['q'][key].dtype and torch.equal(a['q'][key].nan_to_num(-1.0), b['q'][key].nan_to_num(-1.0)), (k, i, key)
    assert [o['ok'] for o in got[1]] == [True, True, False, True, True] and torch.equal(got[1][2]['P'], got[1][1]['P'])
    if 'warm_start' in opts:                                              # cold on the first pair, after the rejected frame and after the reset
        assert [row[6] == 0.0 for row in rows_of[1]] == [True, False, True, False]
        assert [row[6] == 0.0 for row in rows_of[0]] == [True, False, False, True]
