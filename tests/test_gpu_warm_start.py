"""GPU: warm start of RAFT from the previous frame's flow.

* ops.forward_interpolate (rpe_flow_forward_interpolate) bit-exact against the numpy restatement (tests/flow_interp_ref.py) at several
  map sizes and kinds of flow, and row k of a batch of 64 equal to row k alone, bit for bit.
* RAFT.forward(flow_init=...) against a test-local restatement of the oracle loop started at coords1 = coords0 + flow_init, with
  test_gpu_pipeline's tolerances for cold flow; the launch-by-launch, launch-list and recorded routes bitwise equal; zero flow_init
  bitwise equal to a cold call on every route; library calls of cold and warm passes.
* The trackers with ``warm_start: True`` on a 6-frame synthetic sequence: what must stay cold stays bitwise cold, frame t's temporal flow
  is the hand-driven warm RAFT pass, submit / result equals forward, a rejected frame and reset() make the next pass cold, and each
  sequence of MultiSurfelPoseEstimator equals its own warm SurfelPoseEstimator."""
import warnings

import numpy as np
import pytest
import torch

from flow_interp_ref import forward_interpolate as ref_interpolate, make_flows
from oracle import pose_net as opn
from oracle import raft as oraft

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
H, W = 352, 384
F2F = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=8, conf_weighing=True)
F2M = dict(frame2frame=False, depth_clipping=[1, 250], lbgfs_iters=8, conf_weighing=True, dist_thr=0.05, average_pts=True)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t.view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ forward_interpolate
@pytest.mark.parametrize('h,w,kinds', [(64, 80, ('subpixel', 'outward', 'invalid', 'zero', 'shift')),
                                       (80, 64, ('subpixel', 'outward', 'shift')),
                                       (128, 160, ('subpixel', 'outward')),
                                       (45, 61, ('subpixel', 'outward', 'invalid', 'zero', 'shift'))])
def test_forward_interpolate_is_bit_exact(rpe, h, w, kinds):
    from rpe_amd import ops
    for i, kind in enumerate(kinds):
        f = make_flows(kind, h, w, seed=10 + i)
        got = ops.forward_interpolate(torch.from_numpy(f).to(DEV)).cpu().numpy()
        want = ref_interpolate(f)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (h, w, kind, int((got != want).sum()))
        if kind == 'invalid':
            assert not got.any()


def test_forward_interpolate_rows_do_not_depend_on_the_batch(rpe):
    from rpe_amd import ops
    kinds = ('subpixel', 'outward', 'invalid', 'zero', 'shift')
    f = torch.from_numpy(np.concatenate([make_flows(kinds[i % 5], 64, 80, seed=100 + i) for i in range(64)])).to(DEV)
    out = torch.full_like(f, 7.0)
    assert ops.forward_interpolate(f, out=out) is out
    for k in range(64):
        assert _same(ops.forward_interpolate(f[k:k + 1]), out[k:k + 1]), k
    assert _same(ops.forward_interpolate(f), out)                         # and run to run
    with pytest.raises(rpe.RpeError):
        ops.forward_interpolate(f, out=f)


# ------------------------------------------------------------------------------------------------ RAFT flow_init
@pytest.fixture(scope='module')
def models(rpe):
    from rpe_amd import pose_net, synth
    cfg = synth.model_config(H, W, iters=12, lbgfs_iters=8)
    model = synth.init_synthetic_weights(pose_net.PoseNet(cfg)).eval().to(DEV)
    om = opn.PoseNet(cfg)
    om.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    om.eval()
    return model, om, synth


@torch.no_grad()
def _oracle_warm(of, image1, image2, flow_init, iters=12):
    """oracle/raft.py's RAFT.forward with upstream's warm start: coords1 = coords0 + flow_init."""
    image1, image2 = 2 * (image1 / 255.0) - 1.0, 2 * (image2 / 255.0) - 1.0
    fmap1, fmap2 = of.fnet([image1.contiguous(), image2.contiguous()])
    corr_fn = oraft.CorrBlock(fmap1.float(), fmap2.float(), num_levels=of.corr_levels, radius=of.corr_radius)
    net, inp = torch.split(of.cnet(image1), [of.hidden_dim, of.context_dim], dim=1)
    net, inp = torch.tanh(net), torch.relu(inp)
    N, _, h, w = image1.shape
    coords0 = oraft.coords_grid(N, h // 8, w // 8)
    coords1 = coords0 + flow_init
    for _ in range(iters):
        corr = corr_fn(coords1)
        net, up_mask, delta_flow = of.update_block(net, inp, corr, coords1 - coords0)
        coords1 = coords1 + delta_flow
    return oraft.upsample_flow(coords1 - coords0, up_mask), net, coords1 - coords0


def _pair(synth, seed, n, h=H, w=W):
    fr = synth.stereo_frames(seed, n, h, w)
    return fr['image1l'], fr['image2l']


def _routes(monkeypatch, raft):
    """(name, settings) of the fused route's three ways to run a small pass."""
    return (('launch by launch', dict(FRAME_OPLISTS=False, LOOP_OPLIST=False)), ('launch list', dict(FRAME_OPLISTS=False, LOOP_OPLIST=True)),
            ('recorded', dict(FRAME_OPLISTS=True, LOOP_OPLIST=True)))


def test_raft_flow_init_matches_oracle_and_routes_agree(models, monkeypatch):
    model, om, synth = models
    from rpe_amd import raft
    i1, i2 = _pair(synth, 41, 2)
    g1, g2 = i1.to(DEV), i2.to(DEV)
    cold, _, _, low = model.flow(g1, g2, ret_lowres=True)
    # a plausible warm start: the cold answer, scaled and displaced (the loop has to move from it)
    finit = (0.6 * low + 0.25).contiguous()
    warm = {}
    for name, st in _routes(monkeypatch, raft):
        for k, v in st.items():
            monkeypatch.setattr(raft, k, v)
        for _ in range(2):                                                   # (the second pass replays what the first built)
            warm[name] = model.flow(g1, g2, flow_init=finit, ret_lowres=True)
    ref = warm['recorded']
    for name, r in warm.items():
        assert len(r) == 4 and len(r[0]) == 1
        assert _same(r[0][-1], ref[0][-1]) and _same(r[1], ref[1]) and _same(r[2], ref[2]) and _same(r[3], ref[3]), name
    every = model.flow(g1, g2, flow_init=finit, all_flows=True, ret_lowres=True)
    assert len(every[0]) == 12 and _same(every[0][-1], ref[0][-1]) and _same(every[3], ref[3]) and _same(every[1], ref[1])
    assert not _same(ref[0][-1], cold[0])                                   # the start really matters
    oflow, onet, olow = _oracle_warm(om.flow, i1, i2, finit.cpu())
    d = float((ref[0][-1].cpu() - oflow).abs().max())
    print(f'warm flow vs oracle: {d:.2e} px')
    assert d < 1e-3 and float((ref[1].cpu() - onet).abs().max()) < 5e-3 and float((ref[3].cpu() - olow).abs().max()) < 5e-3
    assert ref[3].data_ptr() != warm['launch list'][3].data_ptr()           # fresh tensors


def test_zero_flow_init_is_the_cold_pass_on_every_route(models, monkeypatch):
    model, om, synth = models
    from rpe_amd import raft
    i1, i2 = (t.to(DEV) for t in _pair(synth, 42, 2))
    zero = torch.zeros(2, 2, H // 8, W // 8, device=DEV)
    for name, st in _routes(monkeypatch, raft):
        for k, v in st.items():
            monkeypatch.setattr(raft, k, v)
        for up in (True, False):
            c = model.flow(i1, i2, upsample=up)
            z = model.flow(i1, i2, upsample=up, flow_init=zero)
            assert len(c) == len(z) == 3
            assert _same(c[0][-1], z[0][-1]) and _same(c[1], z[1]) and _same(c[2], z[2]), (name, up)
    ca = model.flow(i1, i2, all_flows=True)
    za = model.flow(i1, i2, all_flows=True, flow_init=zero)
    assert all(_same(a, b) for a, b in zip(ca[0], za[0]))


@pytest.mark.parametrize('h,w', [(360, 360), (352, 360)])
def test_generic_route_flow_init(models, monkeypatch, h, w):
    """Odd / non-quad maps: the generic route seeds coords1 = coords0 + flow_init too; zero is the cold pass bit for bit, a real start
    matches the oracle restatement."""
    model, om, synth = models
    i1, i2 = _pair(synth, 43, 1, h, w)
    g1, g2 = i1.to(DEV), i2.to(DEV)
    assert model.flow.update_block.packed_convs(w // 8) is None or (h // 8) % 2 == 1
    cold = model.flow(g1, g2, ret_lowres=True)
    zero = model.flow(g1, g2, flow_init=torch.zeros_like(cold[3]), ret_lowres=True)
    assert all(_same(a, b) for a, b in ((cold[0][-1], zero[0][-1]), (cold[1], zero[1]), (cold[3], zero[3])))
    finit = (0.6 * cold[3] + 0.25).contiguous()
    warm = model.flow(g1, g2, flow_init=finit, ret_lowres=True)
    every = model.flow(g1, g2, flow_init=finit, all_flows=True)
    assert _same(every[0][-1], warm[0][-1])
    oflow, onet, _ = _oracle_warm(om.flow, i1, i2, finit.cpu())
    d = float((warm[0][-1].cpu() - oflow).abs().max())
    print(f'{h}x{w} warm flow vs oracle: {d:.2e} px')
    assert d < 1e-3 and float((warm[1].cpu() - onet).abs().max()) < 5e-3


def test_library_calls_of_cold_and_warm_passes(models, monkeypatch):
    model, om, synth = models
    from rpe_amd import _lib, raft
    i1, i2 = (t.to(DEV) for t in _pair(synth, 44, 2))
    f = model.flow.encode_features((i1, i2))
    cn = model.flow.encode_context(i1)
    fm = (f[:2], f[2:])
    finit = torch.full((2, 2, H // 8, W // 8), 0.5, device=DEV)

    def count(**kw):
        for _ in range(2):                   # (records what the counted pass replays; a recording that met a first-use weight packing is redone)
            model.flow(None, None, fmaps=fm, cnet=cn, **kw)
        with _lib.CountingLib() as c:
            model.flow(None, None, fmaps=fm, cnet=cn, **kw)
        return c
    cold, warm = count(), count(flow_init=finit)
    assert cold.calls == 3 and warm.calls == 3 and cold.names == warm.names == ['rpe_run_ops'] * 3     # recorded: front, loop, tail
    assert warm.list_ops == cold.list_ops - 3                                 # four plane copies -> one seeding launch
    monkeypatch.setattr(raft, 'FRAME_OPLISTS', False)
    cold, warm = count(), count(flow_init=finit)
    assert 'rpe_flow_seed' not in cold.names and warm.names.count('rpe_flow_seed') == 1
    assert warm.calls == cold.calls - 3 and cold.names.count('rpe_copy_planes') == warm.names.count('rpe_copy_planes') + 4


# ------------------------------------------------------------------------------------------------ trackers
def _frames(synth, seed, n=6):
    s = synth.stereo_frames(seed, n, H, W)
    return [(s['image2l'][i:i + 1].to(DEV), s['image2r'][i:i + 1].to(DEV), s['mask2'][i:i + 1].to(DEV)) for i in range(n)], s['K'][0]


def _gate(monkeypatch, reject=()):
    """Every frame passes the gate (the seeded weights would reject some at random) except the scripted calls in ``reject``."""
    from rpe_amd import ops
    real, real_rows = ops.pose_gate_chain, ops.pose_gate_chain_rows
    calls = [0]

    def gate(rel, init, scale, thr=0.1):
        r, p, ok = real(rel, init, scale, thr)
        i = calls[0]
        calls[0] += 1
        return r, p, torch.full_like(ok, 0 if i in reject else 1)

    def gate_rows(rel, init, scale, thr=0.1):
        r, p, ok = real_rows(rel, init, scale, thr)
        return r, p, torch.ones_like(ok)
    monkeypatch.setattr(ops, 'pose_gate_chain', gate)
    monkeypatch.setattr(ops, 'pose_gate_chain_rows', gate_rows)


def _spy(monkeypatch, model):
    """Records the flow_init of every PoseNet.infer call (None = a cold pass)."""
    seen, real = [], model.infer

    def infer(*a, **kw):
        fi = kw.get('flow_init')
        seen.append(None if fi is None else fi.clone())
        return real(*a, **kw)
    monkeypatch.setattr(model, 'infer', infer)
    return seen


def _run(est, frames, pipelined=False):
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if pipelined:
            est.submit(*frames[0][:2], frames[0][2].clone())
        for t, (l, r, m) in enumerate(frames):
            if pipelined:
                if t + 1 < len(frames):
                    est.submit(*frames[t + 1][:2], frames[t + 1][2].clone())
                P, _, flow, _ = est.result()
            else:
                P, _, flow, _ = est(l, r, m.clone())
            out.append(dict(P=P.data.clone(), flow=None if flow is None else flow.clone(), depth=est.frame.depth.clone(),
                            sflow=est.frame.flow.clone(), low=None if est._flow_low is None else est._flow_low.clone(), ok=est.success))
    return out


def test_f2f_tracker_warm_start(models, monkeypatch):
    model, om, synth = models
    from rpe_amd import ops, pose_estimator
    frames, K = _frames(synth, 51)
    _gate(monkeypatch)
    cold = _run(pose_estimator.PoseEstimator(F2F, K, 7.2 * 250.0, model, (W, H)).to(DEV), frames)
    seen = _spy(monkeypatch, model)
    est = pose_estimator.PoseEstimator(dict(F2F, warm_start=True), K, 7.2 * 250.0, model, (W, H)).to(DEV)
    warm = _run(est, frames)
    assert len(seen) == 5 and seen[0] is None and all(s is not None for s in seen[1:])       # frame 1's pair is cold, the rest warm
    assert _same(warm[0]['P'], cold[0]['P']) and _same(warm[1]['P'], cold[1]['P']) and _same(warm[1]['flow'], cold[1]['flow'])
    for t in range(6):
        assert _same(warm[t]['depth'], cold[t]['depth']) and _same(warm[t]['sflow'], cold[t]['sflow']), t
    assert not _same(warm[5]['flow'], cold[5]['flow'])
    flow_net = model.flow
    for t in range(2, 6):
        (pl, _, _), (l, r, _) = frames[t - 1], frames[t]
        fi = ops.forward_interpolate(warm[t - 1]['low'])
        assert _same(seen[t - 1], fi), t
        f = flow_net.encode_features((pl, l, r))
        cn = flow_net.encode_context((pl, l))
        preds, _, _, low = flow_net(None, None, fmaps=(f[:2], f[1:]), cnet=cn, flow_init=torch.cat((fi, torch.zeros_like(fi))), ret_lowres=True)
        assert _same(preds[-1][:1], warm[t]['flow']) and _same(low[:1], warm[t]['low']), t
    # pipelined: bit for bit the same as forward
    est.reset()
    piped = _run(est, frames, pipelined=True)
    for a, b in zip(warm, piped):
        assert all(_same(a[k], b[k]) for k in ('P', 'depth', 'sflow')) and (a['flow'] is None or _same(a['flow'], b['flow']))


def test_rejected_frame_and_reset_make_the_next_pass_cold(models, monkeypatch):
    model, om, synth = models
    from rpe_amd import pose_estimator
    frames, K = _frames(synth, 52)
    _gate(monkeypatch, reject=(3,))                                           # the gate rejects frame 3 (call 3: frame 0 is call 0)
    seen = _spy(monkeypatch, model)
    est = pose_estimator.PoseEstimator(dict(F2F, warm_start=True), K, 7.2 * 250.0, model, (W, H)).to(DEV)
    out = _run(est, frames)
    assert [o['ok'] for o in out] == [True, True, True, False, True, True]
    assert [s is None for s in seen] == [True, False, False, True, False]    # pairs (0,1) .. (4,5): after the rejected frame 3, cold
    est.reset()
    assert est._flow_low is None
    _run(est, frames[:3])
    assert [s is None for s in seen[5:]] == [True, False]
    # the cold pass after the rejection is the cold tracker's pass on the same inputs
    f = model.flow.encode_features((frames[3][0], frames[4][0], frames[4][1]))
    cn = model.flow.encode_context((frames[3][0], frames[4][0]))
    preds, _, _ = model.flow(None, None, fmaps=(f[:2], f[1:]), cnet=cn)
    assert _same(preds[-1][:1], out[4]['flow'])


def _f2m_sequences(synth):
    seqs, Ks, bfs = [], [], []
    for k, n in enumerate((6, 5, 4)):
        fr, K = _frames(synth, 60 + k, n)
        seqs.append(fr)
        Ks.append(K * torch.tensor([[1.0 + 0.02 * k], [1.0 - 0.01 * k], [1.0]]))
        bfs.append(7.2 * 250.0 * (1.0 + 0.1 * k))
    return seqs, Ks, bfs, (0, 0, 2)


def test_f2m_trackers_warm_start(models, monkeypatch):
    """SurfelPoseEstimator: first pose, depth and stereo flow as the cold tracker's; its temporal pairs (render -> frame) warm from the
    second frame on, seeded with forward_interpolate of the previous pass's flow.  MultiSurfelPoseEstimator: each sequence bit for bit
    its own warm SurfelPoseEstimator, with rows subsets and a reset of one sequence."""
    model, om, synth = models
    from rpe_amd import ops, pose_estimator
    _gate(monkeypatch)
    seqs, Ks, bfs, starts = _f2m_sequences(synth)
    cold = _run(pose_estimator.SurfelPoseEstimator(F2M, Ks[0], bfs[0], model, (W, H)).to(DEV), seqs[0])
    seen = _spy(monkeypatch, model)
    single = []
    for k, seq in enumerate(seqs):
        est = pose_estimator.SurfelPoseEstimator(dict(F2M, warm_start=True), Ks[k], bfs[k], model, (W, H)).to(DEV)
        n0 = len(seen)
        single.append(_run(est, seq))
        assert seen[n0] is None and all(s is not None for s in seen[n0 + 1:])
        for t in range(1, len(seq)):
            assert _same(seen[n0 + t], ops.forward_interpolate(single[k][t - 1]['low'])), (k, t)
    w0 = single[0]
    assert _same(w0[0]['P'], cold[0]['P']) and _same(w0[0]['flow'], cold[0]['flow'])
    for t in range(6):
        assert _same(w0[t]['depth'], cold[t]['depth']) and _same(w0[t]['sflow'], cold[t]['sflow']), t
    assert not _same(w0[5]['flow'], cold[5]['flow'])
    # one frame-to-model tracker per sequence, in lockstep; sequence 1 is reset after its second frame (its next pass is cold again)
    multi = pose_estimator.MultiSurfelPoseEstimator(dict(F2M, warm_start=True), torch.stack(Ks), torch.tensor(bfs), model, (W, H)).to(DEV)
    got = [[] for _ in seqs]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for t in range(max(st + len(sq) for st, sq in zip(starts, seqs))):
            rows = [k for k in range(len(seqs)) if starts[k] <= t < starts[k] + len(seqs[k])]
            fr = [seqs[k][t - starts[k]] for k in rows]
            P, ok, _, flow, _ = multi(*(torch.cat([f[i] for f in fr]) for i in range(2)), torch.cat([f[2] for f in fr]).clone(), rows=rows)
            for j, k in enumerate(rows):
                got[k].append(dict(P=P.data[j:j + 1].clone(), flow=flow[j:j + 1].clone()))
            if t == 1:
                multi.reset([1])
    for k in (0, 2):
        assert len(got[k]) == len(single[k])
        for t, (a, b) in enumerate(zip(single[k], got[k])):
            assert _same(a['P'], b['P']) and _same(a['flow'], b['flow']), (k, t)
    # sequence 1: frames 0, 1 as its own tracker; after the reset, frames 2.. are a new sequence starting at frame 2
    est = pose_estimator.SurfelPoseEstimator(dict(F2M, warm_start=True), Ks[1], bfs[1], model, (W, H)).to(DEV)
    again = _run(est, seqs[1][2:])
    for t, (a, b) in enumerate(zip(single[1][:2] + again, got[1])):
        assert _same(a['P'], b['P']) and _same(a['flow'], b['flow']), (1, t)
