"""GPU: ``report_quality`` through the trackers (352x384, seeded weights, 4 synthetic frames).

The report changes nothing it does not add: poses, relative poses and success flags are torch.equal with the option on and off, in
PoseEstimator.forward, forward_chunk, SurfelPoseEstimator and MultiSurfelPoseEstimator; ``last_quality`` is the same bit for bit however
the frames were batched; its covariance is ops.pose_quality on the frame's solver inputs at the solve's float64 pose, de-normalised
like the pose; the solver's bookkeeping is the solve's ``info``; the first frame, which has no solve, reports pd = 0 and NaN; the
quality path does not synchronise; and with the option off a frame makes the library calls it made before the option existed."""
import collections
import inspect
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
H, W = 352, 384
F2F = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=8, conf_weighing=True)
F2M = dict(frame2frame=False, depth_clipping=[1, 250], lbgfs_iters=8, conf_weighing=True, dist_thr=0.05, average_pts=True)
BF = 7.2 * 250.0
KEYS = ('cov', 'pd', 'n2d', 'n3d', 'rms2d_px', 'rms3d', 'f', 'grad_max', 'n_iter', 'func_evals', 'stop_reason')
# Library calls of ONE steady-state PoseEstimator.forward (cold, reuse_features on) before report_quality existed, counted with
# _lib.CountingLib: entry-point calls from Python and the ops launch lists enqueue on top.  The figures are the ones NOTES.md records for
# the cold tracker ("Warm start from the previous frame's flow", tools/bench_warm_start.py: 9 library calls, 273 list ops per frame); the
# files that decide a frame's launches (pose_estimator.py, pose_net.py, raft.py) are unchanged from that measurement to the commit this
# feature was added on, and a launch list's length does not depend on the image size.
PARENT_CALLS, PARENT_LIST_OPS = 9, 273


def _bits(t):
    return t.detach().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    """Bit for bit, NaNs included."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _clone(q):
    return {k: v.clone() for k, v in q.items()}


@pytest.fixture(scope='module')
def seq(rpe):
    from rpe_amd import pose_net, synth
    model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(H, W, iters=12, lbgfs_iters=8))).eval().to(DEV)
    fr = synth.stereo_frames(21, 10, H, W)                     # (the sequence of tests/test_gpu_chunked_tracker.py: its first pairs pass the gate)
    return model, fr['K'][0], (fr['image2l'][:4].to(DEV), fr['image2r'][:4].to(DEV), fr['mask2'][:4].to(DEV))


def _frame(seq, t):
    L, R, M = seq[2]
    return L[t:t + 1], R[t:t + 1], M[t:t + 1].clone()


@pytest.fixture(scope='module')
def walk(seq):
    """The four frames through PoseEstimator.forward with the report off and on: computed once, shared, left unchanged."""
    from rpe_amd import pose_estimator
    model, K, _ = seq
    problem = model.pose_head.problem
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for on in (False, True):
            est = pose_estimator.PoseEstimator(dict(F2F, report_quality=on), K, BF, model, (W, H)).to(DEV)
            rows = []
            for t in range(4):
                P = est(*_frame(seq, t))[0]
                rows.append(dict(pose=P.data.clone(), rel=est.last_rel_pose.data.clone(), ok=est.success,
                                 quality=_clone(est.last_quality) if on else est.last_quality,
                                 info=problem.last_info.clone() if t else None))
            out[on] = rows
    return out


def test_poses_are_unchanged_by_the_report(walk):
    for a, b in zip(walk[False], walk[True]):
        assert torch.equal(a['pose'], b['pose']) and torch.equal(a['rel'], b['rel']) and a['ok'] == b['ok']
        assert a['quality'] is None and sorted(b['quality']) == sorted(KEYS)
    assert all(r['ok'] for r in walk[True][1:])


def test_first_frame_reports_no_solve_and_later_frames_the_solve(walk):
    q0 = walk[True][0]['quality']
    assert float(q0['pd'][0]) == 0.0 and bool(torch.isnan(q0['cov']).all()) and tuple(q0['cov'].shape) == (1, 6, 6)
    assert int(q0['n_iter'][0]) == 0 and int(q0['stop_reason'][0]) == 0
    for t in range(1, 4):
        q, info = walk[True][t]['quality'], walk[True][t]['info']
        assert all(v.is_cuda for v in q.values())
        assert float(q['pd'][0]) == 1.0 and bool(torch.isfinite(q['cov']).all()) and 0.0 < float(q['n2d'][0]) <= H * W
        assert torch.equal(q['n_iter'], info[:, 0]) and torch.equal(q['func_evals'], info[:, 1]) and torch.equal(q['stop_reason'], info[:, 2])
        assert int(q['n_iter'][0]) > 0 and int(q['stop_reason'][0]) != 0
        d = torch.diagonal(q['cov'][0])
        assert bool((d > 0).all()) and 0.0 < float(q['rms2d_px'][0]) < float('inf') and 0.0 < float(q['rms3d'][0]) < float('inf')


def test_covariance_is_pose_quality_on_the_solver_inputs_denormalised(seq, walk):
    """Frame 1, by hand: the arguments PoseEstimator gives PoseNet.infer, the stages in front of the solve, the solve, then
    ops.pose_quality on exactly those inputs at the solve's float64 pose -- and rows / columns 0..2 times 1 / scale."""
    from rpe_amd import ops, pose_estimator
    model, K, _ = seq
    problem = model.pose_head.problem
    est = pose_estimator.PoseEstimator(F2F, K, BF, model, (W, H)).to(DEV)
    est(*_frame(seq, 0))
    L1, R1, M1 = _frame(seq, 1)
    a = dict(image1l=est.frame.img, image2l=L1, intrinsics=est.intrinsics, baseline=est.baseline * est.scale, depth1=est.frame.depth * est.scale,
             image2r=R1, mask1=est.frame.mask, stereo_flow1=est.frame.flow)
    cache = est._enc_cache                                        # (the encoder outputs of frame 0, as the tracker reuses them)
    r = model.infer(mask2=M1.clone(), ret_details=True, ret_quality=True, cache1=cache, ret_cache=True, **a)
    assert len(r) == 8 and sorted(r[6]) == sorted(KEYS) and sorted(r[7]) == ['cnet', 'fmap']
    plain = model.infer(mask2=M1.clone(), ret_details=True, cache1=cache, ret_cache=True, **a)
    assert len(plain) == 7 and torch.equal(plain[0].data, r[0].data)
    T = problem.last_T.clone()
    s = model.stages(mask2=M1.clone(), cache1=cache, **a)
    lw = model.loss_weight.detach()[None, :].repeat(1, 1)
    inputs = (s['time_flow'], s['pcl1'], s['pcl2w'], s['w2d'], s['w3d'], est.frame.mask.bool(), s['mask2w'], s['intrinsics'], lw)
    direct = ops.quality_fields(ops.pose_quality(*inputs, T))
    assert _same(direct['cov'], r[6]['cov']) and _same(direct['rms3d'], r[6]['rms3d']) and float(direct['pd'][0]) == 1.0
    inv = est._inv_scale
    cov = direct['cov'].clone()
    cov[:, :3, :] *= inv
    cov[:, :, :3] *= inv
    got = walk[True][1]['quality']
    assert _same(got['cov'], cov) and _same(got['rms3d'], direct['rms3d'] * inv)
    for k in ('pd', 'n2d', 'n3d', 'rms2d_px', 'f', 'grad_max'):
        assert _same(got[k], direct[k]), k
    assert float(got['cov'][0, 0, 0]) > 1e4 * float(direct['cov'][0, 0, 0])               # (mm^2 against normalised units: inv = 250)


def test_forward_chunk_gives_the_rows_of_single_calls(seq, walk):
    from rpe_amd import pose_estimator
    model, K, (L, R, M) = seq
    est = pose_estimator.PoseEstimator(dict(F2F, report_quality=True), K, BF, model, (W, H)).to(DEV)
    off = pose_estimator.PoseEstimator(F2F, K, BF, model, (W, H)).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        est(*_frame(seq, 0))
        off(*_frame(seq, 0))
        P = est.forward_chunk(L[1:4], R[1:4], M[1:4].clone())[0]
        P_off = off.forward_chunk(L[1:4], R[1:4], M[1:4].clone())[0]
    single = walk[True][1:]
    assert torch.equal(P, torch.cat([r['pose'] for r in single])) and torch.equal(P, P_off) and off.last_quality is None
    assert torch.equal(est.last_rel_poses, torch.cat([r['rel'] for r in single])) and torch.equal(est.last_rel_poses, off.last_rel_poses)
    assert est.successes.tolist() == [r['ok'] for r in single] == off.successes.tolist()
    for k in KEYS:
        assert _same(est.last_quality[k], torch.cat([r['quality'][k] for r in single])), k


def _f2m_runs(seq, report):
    """Two frame-to-model sequences (frames 0,1 and 2,3) on single trackers."""
    from rpe_amd import pose_estimator
    model, K, _ = seq
    out = []
    for first in (0, 2):
        est = pose_estimator.SurfelPoseEstimator(dict(F2M, report_quality=report), K, BF, model, (W, H)).to(DEV)
        rows = []
        for t in (first, first + 1):
            P = est(*_frame(seq, t))[0]
            rows.append(dict(pose=P.data.clone(), rel=est.last_rel_pose.data.clone(), ok=est.success,
                             quality=_clone(est.last_quality) if report else est.last_quality))
        out.append(rows)
    return out


def test_surfel_trackers_single_and_batched(seq):
    from rpe_amd import pose_estimator
    model, K, (L, R, M) = seq
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        off, on = _f2m_runs(seq, False), _f2m_runs(seq, True)
        multi = pose_estimator.MultiSurfelPoseEstimator(dict(F2M, report_quality=True), torch.stack((K, K)), torch.tensor([BF, BF]), model,
                                                        (W, H)).to(DEV)
        got = []
        for step in range(2):
            idx = [step, 2 + step]
            P, ok, _, _, _ = multi(torch.cat([L[i:i + 1] for i in idx]), torch.cat([R[i:i + 1] for i in idx]),
                                   torch.cat([M[i:i + 1] for i in idx]).clone())
            got.append((P.data.clone(), ok.clone(), multi.last_rel_poses.clone(), _clone(multi.last_quality)))
    for k in range(2):
        for step in range(2):
            a, b = off[k][step], on[k][step]
            assert torch.equal(a['pose'], b['pose']) and torch.equal(a['rel'], b['rel']) and a['ok'] == b['ok'] and a['quality'] is None
            q = b['quality']                                    # frame to model: the first frame too is solved, against its own map
            assert all(v.is_cuda for v in q.values()) and bool(torch.isfinite(q['cov']).all()) == (float(q['pd'][0]) == 1.0)
            P, ok, rel, mq = got[step]
            assert torch.equal(P[k:k + 1], b['pose']) and bool(ok[k]) == b['ok'] and torch.equal(rel[k:k + 1], b['rel'])
            for key in KEYS:
                assert _same(mq[key][k:k + 1], q[key]), (k, step, key)
    assert any(float(r['quality']['pd'][0]) == 1.0 for run in on for r in run)


def test_the_quality_path_does_not_synchronise(seq):
    from rpe_amd import pose_estimator, pose_net
    model, K, _ = seq
    est = pose_estimator.PoseEstimator(dict(F2F, report_quality=True), K, BF, model, (W, H)).to(DEV)
    est(*_frame(seq, 0))
    L1, R1, M1 = _frame(seq, 1)
    s = model.stages(est.frame.img, L1, est.intrinsics, est.baseline * est.scale, est.frame.depth * est.scale, R1, est.frame.mask, M1,
                     est.frame.flow, cache1=est._enc_cache)
    lw = model.loss_weight.detach()[None, :].repeat(1, 1)
    inputs = (s['time_flow'], s['pcl1'], s['pcl2w'], s['w2d'], s['w3d'], est.frame.mask.bool(), s['mask2w'], s['intrinsics'], lw)
    model.pose_head(*inputs)
    model._quality(inputs)                                        # (first use outside the guarded region: code objects, allocator)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            mode_works = False
        except RuntimeError:
            mode_works = True
        if mode_works:                                            # the whole opt-in path: kernel, named views, de-normalisation, blank report
            q = model._quality(inputs)
            est._set_quality(q, 1, DEV)
            est._set_quality(None, 1, DEV)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    if not mode_works:
        # torch's synchronisation guard does nothing in this build: the same statement from the source -- the new code path keeps device
        # tensors and never asks for a host value
        est._set_quality(model._quality(inputs), 1, DEV)
        for fn in (pose_net.PoseNet._quality, pose_estimator.denormalise_quality, pose_estimator.blank_quality, pose_estimator.PoseEstimator._set_quality):
            src = inspect.getsource(fn)
            assert '.cpu(' not in src and '.item(' not in src and 'synchronize' not in src and 'bool(' not in src
    assert all(v.is_cuda for v in est.last_quality.values())


def test_library_calls_per_frame_are_unchanged_when_off_and_one_more_when_on(seq):
    from rpe_amd import _lib, pose_estimator
    model, K, _ = seq
    counts = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for on in (False, True):
            est = pose_estimator.PoseEstimator(dict(F2F, report_quality=on), K, BF, model, (W, H)).to(DEV)
            for t in range(3):
                est(*_frame(seq, t))
            with _lib.CountingLib() as c:
                est(*_frame(seq, 3))
            torch.cuda.synchronize()
            counts[on] = c
    off, on = counts[False], counts[True]
    print('library calls of a frame, report off:', off.calls, off.list_ops, dict(collections.Counter(off.names)))
    assert (off.calls, off.list_ops) == (PARENT_CALLS, PARENT_LIST_OPS)
    assert 'rpe_pose_quality' not in off.names
    assert on.calls == off.calls + 1 and on.list_ops == off.list_ops
    assert collections.Counter(on.names) - collections.Counter(off.names) == collections.Counter({'rpe_pose_quality': 1})


def test_warm_start_and_quality_together_in_the_three_trackers(seq):
    """``warm_start`` and ``report_quality`` at once, four frames: the K = 2 MultiSurfelPoseEstimator against a SurfelPoseEstimator per
    sequence -- poses, success flags, the kept 1/8 flows and every field of last_quality bit for bit, row for row (NaNs in the same
    places) --, and PoseEstimator.forward against submit / result on sequence 0."""
    from rpe_amd import pose_estimator, synth
    model, K, (L, R, M) = seq
    fr = synth.stereo_frames(22, 4, H, W)
    Ls, Rs, Ms = (L, fr['image2l'].to(DEV)), (R, fr['image2r'].to(DEV)), (M, fr['mask2'].to(DEV))
    Ks = (K, fr['K'][0])
    both = dict(warm_start=True, report_quality=True)

    def same_low(a, b):
        return (a is None) == (b is None) and (a is None or _same(a, b))

    def left(est, P):
        return dict(pose=P.data.clone(), rel=est.last_rel_pose.data.clone(), ok=est.success, quality=_clone(est.last_quality),
                    low=None if est._flow_low is None else est._flow_low.clone())
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        single = []
        for k in range(2):
            est = pose_estimator.SurfelPoseEstimator(dict(F2M, **both), Ks[k], BF, model, (W, H)).to(DEV)
            single.append([left(est, est(Ls[k][t:t + 1], Rs[k][t:t + 1], Ms[k][t:t + 1].clone())[0]) for t in range(4)])
        multi = pose_estimator.MultiSurfelPoseEstimator(dict(F2M, **both), torch.stack(Ks), torch.tensor([BF, BF]), model, (W, H)).to(DEV)
        for t in range(4):
            P, ok, _, _, _ = multi(*(torch.cat([x[k][t:t + 1] for k in range(2)]).clone() for x in (Ls, Rs, Ms)))
            for k in range(2):
                a = single[k][t]
                assert _same(P.data[k:k + 1], a['pose']) and bool(ok[k]) == a['ok'] and _same(multi.last_rel_poses[k:k + 1], a['rel']), (k, t)
                assert same_low(multi._flow_lows[k], a['low']), (k, t)
                for key in KEYS:
                    assert _same(multi.last_quality[key][k:k + 1], a['quality'][key]), (k, t, key)
        est = pose_estimator.PoseEstimator(dict(F2F, **both), K, BF, model, (W, H)).to(DEV)
        walked = [left(est, est(*_frame(seq, t))[0]) for t in range(4)]
        est.reset()
        est.submit(*_frame(seq, 0))
        piped = []
        for t in range(4):
            if t + 1 < 4:
                est.submit(*_frame(seq, t + 1))
            piped.append(left(est, est.result()[0]))
    for t, (a, b) in enumerate(zip(walked, piped)):
        assert _same(a['pose'], b['pose']) and _same(a['rel'], b['rel']) and a['ok'] == b['ok'] and same_low(a['low'], b['low']), t
        assert sorted(a['quality']) == sorted(KEYS) and all(_same(a['quality'][key], b['quality'][key]) for key in KEYS), t
    # both options did something: a first frame without a solve, later ones with one, and passes that started from a kept flow
    assert float(walked[0]['quality']['pd'][0]) == 0.0 and bool(torch.isnan(walked[0]['quality']['cov']).all()) and walked[0]['low'] is None
    assert any(float(r['quality']['pd'][0]) == 1.0 for r in walked[1:]) and any(r['low'] is not None for r in walked[1:3])
    assert any(r['low'] is not None for run in single for r in run[:3])
