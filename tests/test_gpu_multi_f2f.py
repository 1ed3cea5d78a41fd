"""GPU: MultiPoseEstimator (K frame-to-frame sequences in lockstep) and trajectory.track_sequences on it against PoseEstimator runs of
each sequence alone, at 128x160 with K = 3 sequences of 4 frames (own frames, intrinsics, baselines and initial poses): poses, success
flags, returned flow and weights, the frame kept for the next call, the kept 1/8 flow and the quality rows are torch.equal bit for bit,
with every row in every call and with a changing subset of rows (rows out of order, a sequence's first frame beside tracked rows,
sequences of different lengths), cold, with ``warm_start`` and with ``report_quality``; a frame the gate rejects; one host
synchronisation, one RAFT pass, one solve and one gate launch per call; ``reset(rows=[k])``."""
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
H, W = 128, 160
NSEQ, NFRAMES = 3, 4
BIG = (352, 384)                    # the smallest size the fused weight heads take (a 44x44 map at 1/8): one test runs with them
F2F = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=8, conf_weighing=False)
OPTS = {'cold': {}, 'warm': dict(warm_start=True), 'quality': dict(report_quality=True)}
QKEYS = ('cov', 'pd', 'n2d', 'n3d', 'rms2d_px', 'rms3d', 'f', 'grad_max', 'n_iter', 'func_evals', 'stop_reason')


def _same(a, b):
    """Bit for bit, NaNs included."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    kind = {torch.float64: torch.int64, torch.float32: torch.int32, torch.bool: torch.uint8}.get(a.dtype, a.dtype)
    return torch.equal(a.detach().contiguous().view(kind), b.detach().contiguous().view(kind))


@pytest.fixture(scope='module')
def model(rpe):
    """128x160 is below what the fused weight heads take, so the model runs without them (``use_weights`` off: unit weights).  Four GRU
    iterations: the seeded weights' flow drifts with every iteration, and at this size twelve take every pair past the gate, while after
    four every pair of every seeded sequence passes it -- so the poses chain, warm starts are kept and only the scripted frame is rejected."""
    from rpe_amd import pose_net, synth
    return synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(H, W, iters=4, lbgfs_iters=8, use_weights=False))).eval().to(DEV)


def _data(nseq, nframes, h, w, seed):
    from rpe_amd import synth
    from rpe_amd.se3 import SE3
    seqs, Ks, bfs = [], [], []
    for k in range(nseq):
        s = synth.stereo_frames(seed + k, nframes, h, w)
        seqs.append([(s['image2l'][i:i + 1].to(DEV), s['image2r'][i:i + 1].to(DEV), s['mask2'][i:i + 1].to(DEV)) for i in range(nframes)])
        Ks.append(s['K'][0] * torch.tensor([[1.0 + 0.02 * k], [1.0 - 0.01 * k], [1.0]]))
        bfs.append(float(s['baseline'][0]) * 250.0 * (1.0 + 0.1 * k))
    inits = SE3.exp(torch.tensor([[0.0] * 6, [1.0, -2.0, 0.5, 0.01, 0.0, -0.02], [0.0, 3.0, 0.0, 0.0, 0.03, 0.0]][:nseq]).to(DEV)).data.cpu()
    return seqs, Ks, bfs, inits, (h, w)


@pytest.fixture(scope='module')
def data(rpe):
    """Three sequences of four frames on the device, each with its own intrinsics, baseline and initial pose."""
    return _data(NSEQ, NFRAMES, H, W, 70)


def _left(P, ok, flow, weights, quality, mask, low):
    """What a call leaves for one sequence, as clones: row 0 of a single tracker's results or one row of the batched tracker's."""
    return dict(P=P.clone(), ok=bool(ok), flow=None if flow is None else flow.clone(), w=None if weights is None else [w.clone() for w in weights],
                q=None if quality is None else {k: v.clone() for k, v in quality.items()}, mask=mask.clone(),
                low=None if low is None else low.clone())


def _single_run(cfg, data, model, k, first=0, count=None):
    """Frames first .. first+count-1 of sequence k through a PoseEstimator of its own."""
    from rpe_amd import pose_estimator
    from rpe_amd.se3 import SE3
    seqs, Ks, bfs, inits, (h, w) = data
    est = pose_estimator.PoseEstimator(cfg, Ks[k], bfs[k], model, (w, h), init_pose=SE3(inits[k:k + 1])).to(DEV)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for l, r, m in seqs[k][first:][:count]:
            m = m.clone()
            P, _, flow, wts = est(l, r, m)
            out.append(_left(P.data, est.success, flow, wts, est.last_quality, m, est._flow_low))
    return out


_SINGLE = {}


@pytest.fixture
def single(data, model):
    """opts name -> the three single-tracker runs under those options: computed once per option set, shared, left unchanged."""
    def get(name):
        if name not in _SINGLE:
            _SINGLE[name] = [_single_run(dict(F2F, **OPTS[name]), data, model, k) for k in range(NSEQ)]
            print(f'{name}: single trackers accept', [[o['ok'] for o in run] for run in _SINGLE[name]])
        return _SINGLE[name]
    return get


def _multi(cfg, data, model):
    from rpe_amd import pose_estimator
    _, Ks, bfs, inits, (h, w) = data
    return pose_estimator.MultiPoseEstimator(cfg, torch.stack(Ks), torch.tensor(bfs), model, (w, h), init_poses=inits).to(DEV)


def _step(multi, data, rows, nxt, got):
    """One lockstep call on the next frame of each sequence in ``rows``; what it leaves per sequence goes to got[k]."""
    seqs, (h, w) = data[0], data[4]
    fr = [seqs[k][nxt[k]] for k in rows]
    l, r = (torch.cat([f[i] for f in fr]) for i in range(2))
    m = torch.cat([f[2] for f in fr]).clone()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        P, ok, flow, wts = multi(l, r, m, rows=rows)
    R = len(rows)
    assert P.data.shape == (R, 7) and ok.shape == (R,) and ok.dtype == torch.bool and not ok.is_cuda
    assert flow.shape == (R, 2, h, w) and wts[0].shape == wts[1].shape == (R, 1, h, w)
    q = multi.last_quality
    assert (q is None) == (not multi.report_quality) and (q is None or all(v.shape[0] == R for v in q.values()))
    for j, k in enumerate(rows):
        assert multi.success[k] == bool(ok[j]) and torch.equal(multi.last_pose[k].data, P.data[j:j + 1])
        low = multi._flow_lows[k]
        got[k].append(_left(P.data[j:j + 1], ok[j], flow[j:j + 1], [x[j:j + 1] for x in wts], None if q is None else {key: v[j:j + 1] for key, v in q.items()},
                            m[j:j + 1], None if low is None else low[0][low[1]:low[1] + 1]))
        nxt[k] += 1
    return ok


def _assert_same_runs(want, got, who):
    assert len(got) == len(want), who
    for i, (a, b) in enumerate(zip(want, got)):
        at = (*who, i) if isinstance(who, tuple) else (who, i)
        assert _same(a['P'], b['P']), (at, a['P'], b['P'])
        assert a['ok'] == b['ok'] and _same(a['mask'], b['mask']), at
        if a['flow'] is None:                                              # the first frame: zeros from the batched tracker
            assert not b['flow'].any() and not b['w'][0].any() and not b['w'][1].any(), at
        else:
            assert _same(a['flow'], b['flow']) and _same(a['w'][0], b['w'][0]) and _same(a['w'][1], b['w'][1]), at
        assert (a['low'] is None) == (b['low'] is None) and (a['low'] is None or _same(a['low'], b['low'])), at
        assert (a['q'] is None) == (b['q'] is None), at
        if a['q'] is not None:
            assert sorted(a['q']) == sorted(b['q']) == sorted(QKEYS)
            for key in QKEYS:
                assert _same(a['q'][key], b['q'][key]), (at, key)


@pytest.mark.parametrize('name', list(OPTS))
def test_every_row_in_every_call(single, data, model, name):
    want = single(name)
    multi = _multi(dict(F2F, **OPTS[name]), data, model)
    nxt, got = [0] * NSEQ, [[] for _ in range(NSEQ)]
    for _ in range(NFRAMES):
        _step(multi, data, list(range(NSEQ)), nxt, got)
    for k in range(NSEQ):
        _assert_same_runs(want[k], got[k], (name, k))
    tracked = [o for run in want for o in run[1:]]
    assert any(o['ok'] for o in tracked) and all(o['flow'].abs().max() > 0 for o in tracked)            # the runs did track
    if name == 'warm':
        assert any(o['low'] is not None for o in tracked[:-1])
        cold = single('cold')                                              # ... and the warm start changed a later pass
        assert any(not _same(a['flow'], b['flow']) for ra, rb in zip(want, cold) for a, b in zip(ra[2:], rb[2:]))
    if name == 'quality':
        assert all(float(run[0]['q']['pd'][0]) == 0.0 and bool(torch.isnan(run[0]['q']['cov']).all()) for run in want)
        assert any(float(o['q']['pd'][0]) == 1.0 for o in tracked)


# call by call: the rows that get their next frame.  Rows out of order, sequence 2's first frame beside tracked rows (call 2), single rows.
SCHEDULE = ([0, 1], [2, 0, 1], [1], [0, 2, 1], [2, 0], [2])


@pytest.mark.parametrize('name', list(OPTS))
def test_changing_rows_per_call(single, data, model, name):
    want = single(name)
    multi = _multi(dict(F2F, **OPTS[name]), data, model)
    nxt, got = [0] * NSEQ, [[] for _ in range(NSEQ)]
    for rows in SCHEDULE:
        _step(multi, data, rows, nxt, got)
    assert nxt == [NFRAMES] * NSEQ
    for k in range(NSEQ):
        _assert_same_runs(want[k], got[k], (name, k))


@pytest.mark.parametrize('name', list(OPTS))
def test_track_sequences_with_different_lengths(single, data, model, name):
    from rpe_amd import trajectory
    want = single(name)
    seqs, inits = data[0], data[3]
    lengths = (4, 2, 3)
    multi = _multi(dict(F2F, **OPTS[name]), data, model)
    quality = name == 'quality'
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        trajs = trajectory.track_sequences(multi, [[(l, r, m.clone(), 100 * k + i) for i, (l, r, m) in enumerate(seqs[k][:n])]
                                                   for k, n in enumerate(lengths)], start_stamps=[-1, -2, -3], quality=quality)
    for k, n in enumerate(lengths):
        assert [it['timestamp'] for it in trajs[k]] == [-1 - k] + [100 * k + i for i in range(n)]
        assert _same(trajs[k][0]['camera-pose'], inits[k])
        for i in range(n):
            assert _same(trajs[k][i + 1]['camera-pose'], want[k][i]['P'][0].cpu()), (k, i)
            if quality:
                for key in QKEYS:
                    assert _same(trajs[k][i + 1]['quality'][key], want[k][i]['q'][key][0].cpu()), (k, i, key)
        assert ('quality' in trajs[k][0]) == quality


def test_with_the_weight_heads_at_their_smallest_size(rpe):
    """352x384, two sequences of three frames, the fused weight heads on: a first frame alone, the other sequence's first frame beside a
    tracked row, rows out of order, a single tracked row."""
    from rpe_amd import pose_net, synth
    h, w = BIG
    model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(h, w, iters=12, lbgfs_iters=8))).eval().to(DEV)
    data = _data(2, 3, h, w, 80)
    cfg = dict(F2F, conf_weighing=True, warm_start=True, report_quality=True)
    want = [_single_run(cfg, data, model, k) for k in range(2)]
    multi = _multi(cfg, data, model)
    nxt, got = [0, 0], [[], []]
    for rows in ([0], [1, 0], [0, 1], [1]):
        _step(multi, data, rows, nxt, got)
    for k in range(2):
        _assert_same_runs(want[k], got[k], ('heads', k))
    assert any(float(o['w'][0].min()) < float(o['w'][0].max()) for run in want for o in run[1:])          # (the heads' maps, not unit weights)


class _RejectFrame(torch.nn.Module):
    """The model, except that the relative pose of the row whose new left image is ``marked`` is replaced by ``rel`` (a pose the gate
    rejects), as test_gpu_multi_tracker's scripted model prescribes its rejected frame; everything else of the pass is the model's."""

    def __init__(self, model, marked, rel):
        super().__init__()
        self.model, self.marked, self.rel, self.hits = model, marked, rel, 0

    def flow2depth(self, *a, **kw):
        return self.model.flow2depth(*a, **kw)

    def infer(self, image1l, image2l, *a, **kw):
        from rpe_amd.se3 import SE3
        r = self.model.infer(image1l, image2l, *a, **kw)
        data = r[0].data.reshape(-1, 7).clone()
        for i in range(image2l.shape[0]):
            if torch.equal(image2l[i], self.marked):
                data[i] = self.rel
                self.hits += 1
        return (SE3(data), *r[1:])


@pytest.mark.parametrize('name', ['cold', 'warm'])
def test_a_rejected_frame(single, data, model, name):
    """Sequence 1's frame 2 gets the golden gate case's first rejected relative pose.  In that call only that row fails and keeps its
    pose, the other sequences stay bit-equal to their single runs throughout, and sequence 1 -- the rejected frame and the next one,
    which is tracked against the rejected frame (cold under warm_start) -- equals a single tracker given the same rejection."""
    from rpe_amd import pose_estimator
    from rpe_amd.se3 import SE3
    seqs, Ks, bfs, inits, _ = data
    g = dict(np.load(os.path.join(GOLDEN, 'tracker_f2m.npz')))
    bad = [i for i in range(len(g['gate_success'])) if not g['gate_success'][i]][0]
    rel = torch.from_numpy(g['gate_rel'][bad]).float().to(DEV)
    cfg = dict(F2F, **OPTS[name])
    want = single(name)
    assert all(o['ok'] for run in want for o in run[:3]), 'the sequences must pass the gate on their own up to the scripted frame'
    proxy = _RejectFrame(model, seqs[1][2][0][0], rel)
    est = pose_estimator.PoseEstimator(cfg, Ks[1], bfs[1], model, (W, H), init_pose=SE3(inits[1:2])).to(DEV)
    est.model = proxy
    alone = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for l, r, m in seqs[1]:
            m = m.clone()
            P, _, flow, w = est(l, r, m)
            alone.append(_left(P.data, est.success, flow, w, est.last_quality, m, est._flow_low))
    assert proxy.hits == 1 and [o['ok'] for o in alone[:3]] == [True, True, False] and _same(alone[2]['P'], alone[1]['P'])
    multi = _multi(cfg, data, model)
    multi.model = proxy
    nxt, got, flags = [0] * NSEQ, [[] for _ in range(NSEQ)], []
    for _ in range(NFRAMES):
        flags.append(_step(multi, data, list(range(NSEQ)), nxt, got).tolist())
    assert proxy.hits == 2
    assert flags[2] == [True, False, True] and multi.success[1] == alone[3]['ok']
    assert _same(got[1][2]['P'], got[1][1]['P'])                           # the pose is unchanged
    _assert_same_runs(alone, got[1], (name, 'rejected'))
    for k in (0, 2):
        _assert_same_runs(want[k], got[k], (name, k))
    assert not _same(alone[3]['P'], want[1][3]['P'])                       # (the rejection did change what follows)
    if name == 'warm':
        assert got[1][2]['low'] is None and got[1][1]['low'] is not None


def test_reset_restarts_one_sequence(single, data, model):
    """After two lockstep frames sequence 1 is reset: its next frames are a new run from its frame 2 at its initial pose, the others go on."""
    cfg = dict(F2F, **OPTS['warm'])
    want = single('warm')
    multi = _multi(cfg, data, model)
    nxt, got = [0] * NSEQ, [[] for _ in range(NSEQ)]
    for t in range(NFRAMES):
        if t == 2:
            assert multi.reset(rows=[1]) is multi
            assert multi._prev[1] is None and multi._flow_lows[1] is None and multi.success[1] and multi._prev[0] is not None
            assert _same(multi.last_pose[1].data.cpu(), data[3][1:2])
        _step(multi, data, list(range(NSEQ)), nxt, got)
    for k in (0, 2):
        _assert_same_runs(want[k], got[k], ('reset', k))
    again = _single_run(cfg, data, model, 1, first=2, count=2)
    _assert_same_runs(want[1][:2] + again, got[1], ('reset', 1))


class _HostReads:
    """Counts what makes the host wait for the device: reads of a device tensor's value from Python (cpu, item, tolist, numpy, a move to
    the host, bool / int / float / index of a tensor) and explicit synchronize calls."""
    READS = ('cpu', 'item', 'tolist', 'numpy', '__bool__', '__int__', '__float__', '__index__')

    def __init__(self, monkeypatch):
        self.n = 0

        def read(real):
            def f(t, *a, **kw):
                self.n += bool(t.is_cuda)
                return real(t, *a, **kw)
            return f

        def to(real):
            def f(t, *a, **kw):
                out = real(t, *a, **kw)
                self.n += bool(t.is_cuda and not out.is_cuda)
                return out
            return f

        def sync(real):
            def f(*a, **kw):
                self.n += 1
                return real(*a, **kw)
            return f
        for name in self.READS:
            monkeypatch.setattr(torch.Tensor, name, read(getattr(torch.Tensor, name)))
        monkeypatch.setattr(torch.Tensor, 'to', to(torch.Tensor.to))
        monkeypatch.setattr(torch.cuda, 'synchronize', sync(torch.cuda.synchronize))
        for cls in (torch.cuda.Stream, torch.cuda.Event):
            monkeypatch.setattr(cls, 'synchronize', sync(cls.synchronize))


@pytest.mark.parametrize('name', ['cold', 'warm', 'quality'])
def test_one_synchronisation_one_pass_one_solve_one_gate_per_call(data, model, monkeypatch, name):
    """Per ``forward``: one host synchronisation (the success flags), at most one ``flow2depth`` (over the first-frame rows only), one
    ``infer`` = one RAFT pass over the 2 R' pairs of the R' tracked rows, one solve with ``rows_alone=True``, one
    ``ops.pose_gate_chain_rows`` over all R rows -- in a call of first frames only, a call of tracked rows only and a mixed one."""
    from rpe_amd import ops
    multi = _multi(dict(F2F, **OPTS[name]), data, model)
    seqs = data[0]

    def call(t, rows):
        fr = [seqs[k][t] for k in rows]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return multi(torch.cat([f[0] for f in fr]), torch.cat([f[1] for f in fr]), torch.cat([f[2] for f in fr]).clone(), rows=rows)

    def schedule(check):
        multi.reset()
        check(lambda: call(0, [0, 1]), first=2, tracked=0)
        check(lambda: call(1, [0, 1]), first=0, tracked=2)
        check(lambda: call(2, [1, 2, 0]), first=1, tracked=2)
        check(lambda: call(3, [0, 1, 2]), first=0, tracked=3)
    schedule(lambda f, **kw: f())                                          # (first use of every shape outside the counted region)
    torch.cuda.synchronize()
    log = []
    real = dict(solve=model._solve, flow=model.flow.forward, f2d=model.flow2depth, infer=model.infer, gate=ops.pose_gate_chain_rows)
    monkeypatch.setattr(model, '_solve', lambda inputs, rows_alone=False: (log.append(('solve', inputs[0].shape[0], rows_alone)), real['solve'](inputs, rows_alone))[1])
    monkeypatch.setattr(model.flow, 'forward', lambda *a, **kw: (log.append(('raft', kw['fmaps'][0].shape[0])), real['flow'](*a, **kw))[1])
    monkeypatch.setattr(model, 'flow2depth', lambda l, *a, **kw: (log.append(('flow2depth', l.shape[0])), real['f2d'](l, *a, **kw))[1])
    monkeypatch.setattr(model, 'infer', lambda l, *a, **kw: (log.append(('infer', l.shape[0])), real['infer'](l, *a, **kw))[1])
    monkeypatch.setattr(ops, 'pose_gate_chain_rows', lambda rel, *a, **kw: (log.append(('gate', rel.shape[0])), real['gate'](rel, *a, **kw))[1])
    reads = _HostReads(monkeypatch)

    def check(f, first, tracked):
        del log[:]
        n0 = reads.n
        f()
        assert reads.n - n0 == 1, (first, tracked, reads.n - n0)
        want = [('flow2depth', first), ('raft', first)] if first else []
        want += [('infer', tracked), ('raft', 2 * tracked), ('solve', tracked, True)] if tracked else []
        assert log == want + [('gate', first + tracked)], (first, tracked, log)
    schedule(check)
