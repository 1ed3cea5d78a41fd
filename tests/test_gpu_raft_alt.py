"""GPU: RAFT with ``alternate_corr`` (the correlation windows recomputed from the feature maps at every iteration, ops.AltCorr) against
the CPU oracle and against the pyramid route.

Image 128 x 192, 3 GRU iterations, synthetic weights, batch 2.  (A 64 x 96 image has an 8 x 12 map whose fourth correlation level would be
1 x 1: the oracle's bilinear_sampler divides by size - 1 there and both routes refuse it; 128 x 192 is the smallest image of that aspect
with four levels.)  The flag-on deviation of the final flow from the oracle is held to 2x the flag-off deviation: the same factor as for
one lookup (tests/test_gpu_corr_alt.py: a different but equally long summation order), compounded over 3 iterations.

Measured on an MI355X: see NOTES.md, "On-the-fly correlation"."""
import warnings

import pytest
import torch

from oracle import pose_net as opn
from oracle import se3 as ose3
from oracle import tracker as otracker

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
H, W, ITERS = 128, 192, 3
ROUTES = (('launch by launch', dict(FRAME_OPLISTS=False, LOOP_OPLIST=False)), ('launch list', dict(FRAME_OPLISTS=False, LOOP_OPLIST=True)),
          ('recorded', dict(FRAME_OPLISTS=True, LOOP_OPLIST=True)))


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope='module')
def nets(rpe):
    """RAFT with the key absent, False and True on the same weights, the CPU oracle RAFT, and one pair of image batches."""
    from rpe_amd import raft, synth
    cfg = synth.model_config(H, W, iters=ITERS)
    absent = {k: v for k, v in cfg.items() if k != 'alternate_corr'}
    off = synth.init_synthetic_weights(raft.RAFT(dict(cfg, alternate_corr=False))).eval().to(DEV)
    sd = off.state_dict()
    on, no_key = raft.RAFT(dict(cfg, alternate_corr=True)).eval().to(DEV), raft.RAFT(absent).eval().to(DEV)
    on.load_state_dict(sd), no_key.load_state_dict(sd)
    from oracle import raft as oraft
    om = oraft.RAFT(cfg)
    om.load_state_dict({k: v.cpu() for k, v in sd.items()})
    om.eval()
    fr = synth.stereo_frames(21, 2, H, W)
    return dict(off=off, on=on, no_key=no_key, oracle=om, i1=fr['image1l'], i2=fr['image2l'], synth=synth)


def test_forward_against_the_oracle(nets):
    i1, i2 = nets['i1'], nets['i2']
    with torch.no_grad():
        want = nets['oracle'](i1.clone(), i2.clone(), iters=ITERS)[0][-1]
    dev = {}
    for name in ('off', 'on'):
        got = nets[name](i1.to(DEV), i2.to(DEV))[0][-1].cpu()
        assert got.shape == want.shape == (2, 2, H, W)
        dev[name] = float((got - want).abs().max())
    print(f'RAFT {H}x{W}, {ITERS} iterations, final flow vs oracle: alternate_corr off {dev["off"]:.3e} px, on {dev["on"]:.3e} px '
          f'(flow scale {float(want.abs().max()):.2f} px)')
    assert isinstance(nets['on']._pyr, __import__('rpe_amd').ops.AltCorr) and not isinstance(nets['off']._pyr, __import__('rpe_amd').ops.AltCorr)
    assert dev['on'] <= 2 * dev['off'], dev


def test_routes_agree_bitwise_with_the_flag_on(nets, monkeypatch):
    """Called as the tracker calls it (encoder outputs given, batch <= 4) the pass is recorded and replayed; that, the launch list and
    launch by launch give the same bits -- cold, and warm from a flow_init."""
    from rpe_amd import raft
    net = nets['on']
    g1, g2 = nets['i1'].to(DEV), nets['i2'].to(DEV)
    f = net.encode_features((g1, g2))
    fm, cn = (f[:2].contiguous(), f[2:].contiguous()), net.encode_context(g1)
    finit = torch.full((2, 2, H // 8, W // 8), 0.75, device=DEV)
    finit[:, 1] = -1.25
    for kw in ({}, {'flow_init': finit}):
        res = {}
        for name, st in ROUTES:
            for k, v in st.items():
                monkeypatch.setattr(raft, k, v)
            for _ in range(3):                                   # (the later passes replay what the first ones recorded)
                res[name] = net(None, None, fmaps=fm, cnet=cn, ret_lowres=True, **kw)
        ref = res['launch by launch']
        for name, r in res.items():
            assert _same(r[0][-1], ref[0][-1]) and _same(r[1], ref[1]) and _same(r[3], ref[3]), (name, sorted(kw))
    cold = net(None, None, fmaps=fm, cnet=cn)
    assert not _same(cold[0][-1], res['recorded'][0][-1])        # the warm start really matters


def test_recorded_pass_is_three_library_calls_with_the_flag_on(nets):
    from rpe_amd import _lib
    net = nets['on']
    g1, g2 = nets['i1'].to(DEV), nets['i2'].to(DEV)
    f = net.encode_features((g1, g2))
    fm, cn = (f[:2].contiguous(), f[2:].contiguous()), net.encode_context(g1)
    for _ in range(3):
        net(None, None, fmaps=fm, cnet=cn)
    with _lib.CountingLib() as c:
        net(None, None, fmaps=fm, cnet=cn)
    assert c.names == ['rpe_run_ops'] * 3, c.names               # recorded front (with the prepare), loop, tail


def test_key_absent_equals_false(nets, monkeypatch):
    from rpe_amd import _lib, raft
    g1, g2 = nets['i1'].to(DEV), nets['i2'].to(DEV)
    for name, st in ROUTES:
        for k, v in st.items():
            monkeypatch.setattr(raft, k, v)
        out, counts = {}, {}
        for which in ('no_key', 'off'):
            net = nets[which]
            f = net.encode_features((g1, g2))
            fm, cn = (f[:2].contiguous(), f[2:].contiguous()), net.encode_context(g1)
            for _ in range(3):
                net(None, None, fmaps=fm, cnet=cn)
            with _lib.CountingLib() as c:
                out[which] = net(None, None, fmaps=fm, cnet=cn)
            counts[which] = (c.calls, c.list_ops, tuple(c.names))
        assert _same(out['no_key'][0][-1], out['off'][0][-1]) and _same(out['no_key'][1], out['off'][1]), name
        assert counts['no_key'] == counts['off'], name
        assert not any('corr_alt' in n for n in counts['off'][2])


def _relative(poses):
    """inv(P[t-1]) P[t] of a list of (1, 7) absolute poses."""
    return torch.cat([ose3.se3_mul(ose3.se3_inv(a), b) for a, b in zip(poses[:-1], poses[1:])])


def test_tracker_runs_with_the_flag_on(rpe, monkeypatch):
    """PoseEstimator over 4 synthetic frames.  The flag-off tracker's recorded and call-by-call routes are bit-identical (difference 0), so
    the rule that applies is the oracle-deviation one: the flag-on relative poses deviate from the CPU oracle tracker's by at most 2x what
    the flag-off ones do."""
    from rpe_amd import pose_estimator, pose_net, raft, synth
    h, w, n = 256, 320, 4
    cfg = synth.model_config(h, w, iters=ITERS, lbgfs_iters=3, use_weights=False)
    slam = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=3, conf_weighing=False)
    model = synth.init_synthetic_weights(pose_net.PoseNet(cfg)).eval().to(DEV)
    model_on = pose_net.PoseNet(dict(cfg, alternate_corr=True)).eval().to(DEV)
    model_on.load_state_dict(model.state_dict())
    om = opn.PoseNet(cfg)
    om.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    om.eval()
    fr = synth.stereo_frames(33, n, h, w)
    K = fr['K'][0]

    def track(m):
        est = pose_estimator.PoseEstimator(slam, K, 7.2 * 250.0, m, (w, h)).to(DEV)
        poses, ok = [], []
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for t in range(n):
                P = est(fr['image2l'][t:t + 1].to(DEV), fr['image2r'][t:t + 1].to(DEV), fr['mask2'][t:t + 1].clone().to(DEV))[0]
                poses.append(P.data.cpu().reshape(1, 7).float())
                ok.append(bool(est.success))
        return poses, ok
    off, ok_off = track(model)
    monkeypatch.setattr(raft, 'FRAME_OPLISTS', False)
    monkeypatch.setattr(raft, 'LOOP_OPLIST', False)
    off_calls, _ = track(model)
    monkeypatch.undo()
    route_diff = max(float((a - b).abs().max()) for a, b in zip(off, off_calls))
    on, ok_on = track(model_on)
    assert isinstance(model_on.flow._pyr, rpe.ops.AltCorr)
    assert all(bool(torch.isfinite(p).all()) for p in on) and all(ok_on) and ok_on == ok_off       # finite, within the gate
    traj_diff = max(float((a - b).abs().max()) for a, b in zip(on, off))
    oest = otracker.PoseEstimator(om, K, 7.2 * 250.0)
    want = [oest.forward(fr['image2l'][t:t + 1], fr['image2r'][t:t + 1], fr['mask2'][t:t + 1].clone()).reshape(1, 7).float() for t in range(n)]
    d_off = float((_relative(off) - _relative(want)).abs().max())
    d_on = float((_relative(on) - _relative(want)).abs().max())
    print(f'tracker {w}x{h}, {n} frames: recorded vs call-by-call (flag off) {route_diff:.3e}; flag on vs off {traj_diff:.3e}; relative poses vs oracle: '
          f'off {d_off:.3e}, on {d_on:.3e}; rule applied: {"route difference" if route_diff > 0 else "2x oracle deviation"}')
    if route_diff > 0:
        assert traj_diff <= route_diff
    else:
        assert d_on <= 2 * d_off, (d_on, d_off)
