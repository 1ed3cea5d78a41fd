"""GPU: the training step closed on the package's own kernels -- train.train_step / validate / fit with optim.ClippedAdamW on PoseNet.

352 x 352 and 3 GRU iterations: the smallest grid the weight heads take (44 x 44 at 1/8; below it TinyUNet refuses, and without the heads
neither they nor ``loss_weight``'s partner parameters train) and the fewest iterations at which the synthetic weights leave the pose layer
a regular system (tests/test_gpu_raft_whole.py); n = 1, seeded synthetic weights, a small ``lbgfs_iters``, the heads on the hand-written
training kernels (``train_heads_hip``), the reference's learning rate, weight decay, epsilon and clip (configuration/train.yaml)."""
import os
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H, W = 352, 352
TRAIN = dict(learning_rate=1.0e-5, weight_decay=5.0e-5, epsilon=1.0e-8, grad_clip=1.0, freeze_flow_steps=2, epochs=4)


def _config(lbgfs_iters=20, **train):
    from rpe_amd import synth
    return dict(model=dict(synth.model_config(H, W, iters=3, lbgfs_iters=lbgfs_iters), train_heads_hip=True), train=dict(TRAIN, **train),
                image_shape=[H, W], depth_scale=250)


def _model(config):
    from rpe_amd import pose_net, synth
    return synth.init_synthetic_weights(pose_net.PoseNet(config['model'])).to(DEV)


def _batches(seed, count):
    from rpe_amd import synth
    return list(synth.training_pairs(seed, count, H, W))


def _eval_forward(model, batch):
    from rpe_amd import train
    model.eval()
    with torch.no_grad():
        pose, _ = train._forward(model, batch)
    return pose.clone()


def _track(est, batch):
    """Two stereo frames (the batch's target, then its reference) through a tracker -> the second call's (absolute pose, temporal flow)."""
    ref, trg, ref_r, trg_r, ref_m, trg_m = (x.to(DEV) for x in batch[:6])
    est.reset()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)      # (the gate may reject an untrained model's pose: the flow is compared as well)
        est(trg, trg_r, trg_m.clone())
        out = est(ref, ref_r, ref_m.clone())
    return out[0].data.clone(), out[2].clone()


SLAM = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=20, conf_weighing=True)


def test_the_caches_follow_the_optimizer(rpe):
    """Everything made from weights is cached under (version, pointer); the kernels write through pointers.  After a step the recorded
    passes and packed weights must be those of the NEW weights: the forward equals, to the bit, a fresh model's built from the state_dict
    (it fails, with the pre-step output, when ``step`` does not bump the versions)."""
    from rpe_amd import optim, pose_estimator, pose_net, synth, train
    config = _config()
    model = _model(config)
    batch = _batches(21, 1)[0]
    K, bf = batch[7][0], 250.0 * float(batch[8][0])            # (the tracker normalises by 1 / depth_clipping[1] itself)
    est = pose_estimator.PoseEstimator(SLAM, K, bf, model, (W, H)).to(DEV)
    _eval_forward(model, batch)
    before = _eval_forward(model, batch)                    # (twice: the passes are recorded)
    tracked_before = _track(est, batch)
    model.train().freeze_flow().freeze_flow(False, parts='raft')
    opt = optim.ClippedAdamW(model.parameters(), lr=1e-3, weight_decay=TRAIN['weight_decay'], eps=TRAIN['epsilon'], max_norm=TRAIN['grad_clip'])
    versions = {k: p._version for k, p in model.named_parameters()}
    train.train_step(model, opt, batch)
    assert int(opt.steps) == 1 and int(opt.skipped) == 0
    assert all(p._version > versions[k] for k, p in model.named_parameters())
    after = _eval_forward(model, batch)
    fresh = pose_net.PoseNet(config['model'])
    fresh.load_state_dict(model.state_dict())
    fresh = fresh.to(DEV)
    want = _eval_forward(fresh, batch)
    assert torch.equal(after, want), float((after - want).abs().max())
    assert not torch.equal(after, before)
    tracked_after = _track(est, batch)
    fresh_est = pose_estimator.PoseEstimator(SLAM, K, bf, fresh, (W, H)).to(DEV)
    tracked_fresh = _track(fresh_est, batch)
    assert torch.equal(tracked_after[0], tracked_fresh[0]) and torch.equal(tracked_after[1], tracked_fresh[1])
    assert not torch.equal(tracked_after[1], tracked_before[1])


def test_train_step_equals_the_reference_sequence(rpe):
    """Two train_steps with ClippedAdamW against forward / loss / backward / clip_grad_norm_ / torch.optim.AdamW.step on a copy; truth
    is a float64 replay of the two updates on the CPU from the copy's own gradients, the yardstick the same replay in float32; the bar
    is tests/test_gpu_optim.py's, over all parameters together.
    The comparison holds only while the two models keep the same weights: once they differ by a rounding, the second step's gradients of
    an untrained network differ by far more (measured: up to 1.98 max |g| on one tensor), and the replay, fed the copy's gradients,
    cannot know.  csrc/optim.hip therefore takes torch's GPU roundings (tests/test_gpu_optim.py::test_same_bits_as_torch_on_the_gpu), the
    clip does not engage (norms 0.12 and 0.03 against 1.0), and all 197 parameters agree to the bit after both steps (one MI355X run:
    multiple 1.00; with the kernel rounding in the CPU's order instead it was 2.88)."""
    from rpe_amd import optim, train
    config = _config()
    model = _model(config)
    model.train().freeze_flow().freeze_flow(False, parts='raft')
    twin = _model(config)                                   # (seeded: the same weights)
    twin.train().freeze_flow().freeze_flow(False, parts='raft')
    assert all(torch.equal(a, b) for a, b in zip(model.parameters(), twin.parameters()))
    batches = _batches(22, 2)
    t = config['train']
    start = [p.detach().cpu().clone() for p in model.parameters()]
    opt = optim.ClippedAdamW(model.parameters(), lr=t['learning_rate'], weight_decay=t['weight_decay'], eps=t['epsilon'], max_norm=t['grad_clip'])
    ref = torch.optim.AdamW(twin.parameters(), lr=t['learning_rate'], weight_decay=t['weight_decay'], eps=t['epsilon'])
    grads, norms, own = [], [], []
    for batch in batches:
        train.train_step(model, opt, batch)
        own.append([p.grad.detach().cpu().clone() for p in model.parameters()])
        norms.append(opt.last_norm.clone())
        ref.zero_grad()
        pose, gt = train._forward(twin, batch)
        train.supervised_pose_loss(pose, gt).mean().backward()
        grads.append([p.grad.detach().cpu().clone() for p in twin.parameters()])
        torch.nn.utils.clip_grad_norm_(twin.parameters(), t['grad_clip'])
        ref.step()
        same = sum(torch.equal(a, b) for a, b in zip(model.parameters(), twin.parameters()))
        print(f'train_step: after step {len(grads)} {same} of {len(start)} parameters of the two models agree to the bit')
    assert all(g is not None and bool(g.any()) for g in grads[0][:1]) and len(grads[0]) == len(start)

    def replay(dtype):
        params = [torch.nn.Parameter(v.to(dtype).clone()) for v in start]
        o = torch.optim.AdamW(params, lr=t['learning_rate'], weight_decay=t['weight_decay'], eps=t['epsilon'], foreach=False)
        for step in grads:
            for p, g in zip(params, step):
                p.grad = g.to(dtype).clone()
            torch.nn.utils.clip_grad_norm_(params, t['grad_clip'], foreach=False)
            o.step()
        return [p.detach() for p in params]
    names = [k for k, _ in model.named_parameters()]
    assert all(torch.equal(a, b) for a, b in zip(own[0], grads[0]))          # the same weights, the same batch: the first gradients agree to the bit
    gdiff = max((float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300), k) for k, a, b in zip(names, own[1], grads[1]))
    print(f'train_step: second-step gradients of the two models differ by up to {gdiff[0]:.3e} of max |g| ({gdiff[1]})')
    p64, p32 = replay(torch.float64), replay(torch.float32)
    worst = max((float((g.detach().cpu().double() - x).abs().max()), k) for k, g, x in zip(names, model.parameters(), p64))
    print(f'train_step: worst parameter {worst[1]}, |error| {worst[0]:.3e}')
    err = lambda got, truth: max(float((g.detach().cpu().double() - x.double()).abs().max()) for g, x in zip(got, truth)) / max(float(x.abs().max()) for x in truth)
    e_hip, e_torch, e32 = err(list(model.parameters()), p64), err(list(twin.parameters()), p64), err(p32, p64)
    moved = err(start, p64)
    print(f'train_step, two steps: ClippedAdamW {e_hip:.3e}  torch.optim.AdamW on the GPU {e_torch:.3e}  float32 replay on the CPU {e32:.3e}  '
          f'multiple {e_hip / max(e32, 1e-300):.2f}  (the two steps moved the parameters by {moved:.3e}; norms {[float(n) for n in norms]})')
    assert moved > 100 * e32
    assert e_hip <= 2.0 * e32, (e_hip, e32)


def _snapshot(model):
    return {k: p.detach().clone() for k, p in model.named_parameters()}


def _changed(a, b):
    return {k for k in a if not torch.equal(a[k], b[k])}


def test_fit_on_synthetic_pairs(rpe, tmp_path):
    from rpe_amd import pose_estimator, pose_net, train
    config = _config()
    batches, val = _batches(23, 8), _batches(24, 1)
    model = _model(config)
    flow_names = {'flow.' + k for k, _ in model.flow.named_parameters()}
    assert len(flow_names) == 124
    cancelled = {k for k in flow_names if k.startswith('flow.fnet.') and k.endswith('.bias') and model.get_parameter(k).dim() == 1
                 and model.get_parameter(k[:-4] + 'weight').dim() == 4 and k != 'flow.fnet.conv2.bias'}     # (the output layer has no norm behind it)
    assert len(cancelled) == 15
    shots, logs = [_snapshot(model)], []

    def log(m):
        logs.append(m)
        if 'step' in m:
            shots.append(_snapshot(model))
    out = str(tmp_path / 'run')
    result = train.fit(model, batches, val, config, out, 'net', log=log, val_freq=2)
    assert result['total_steps'] == 5 and not result['stopped_on_nan']           # the reference's `total_steps > epochs`: epochs + 1 steps
    assert int(result['optimizer'].skipped) == 0
    steps = [m for m in logs if 'step' in m]
    assert [m['step'] for m in steps] == [0, 1, 2, 3, 4] and all({'train/loss_rot', 'train/loss_trans', 'train/loss_total'} <= set(m) for m in steps)
    assert sum('val/loss_total' in m for m in logs) == 3                          # validated at steps 0, 2, 4
    for s in range(5):
        moved = _changed(shots[s], shots[s + 1])
        heads = {k for k in shots[0] if k.startswith('weight_head')}
        assert heads <= moved and 'loss_weight' in moved, (s, sorted(heads - moved))
        if s < 2:
            assert not (moved & flow_names), (s, sorted(moved & flow_names)[:4])
        else:
            # all 124 are stepped; fnet's 15 convolution biases are cancelled by its instance norms, their gradients are exact zeros
            # (NOTES.md, "Whole-network training"), and AdamW moves nothing on a zero gradient: 1 - lr * weight_decay = 1 - 5e-10 rounds to 1
            still = flow_names - moved
            assert still == cancelled, (s, sorted(still ^ cancelled)[:4])
    assert all(p.grad is not None and (bool(p.grad.any()) != (k in cancelled)) for k, p in model.named_parameters() if k in flow_names)
    best, last, optim_path = train.checkpoint_paths(out, 'net')
    assert os.path.exists(best) and os.path.exists(last) and os.path.exists(optim_path)
    ckp = torch.load(last, map_location='cpu')
    assert set(ckp) == {'state_dict', 'config'} and set(ckp['state_dict']) == set(model.state_dict())
    assert all(torch.equal(ckp['state_dict'][k], v.cpu()) for k, v in model.state_dict().items())      # written after step 4
    batch = batches[0]
    est = pose_estimator.PoseEstimator(SLAM, batch[7][0], 250.0 * float(batch[8][0]), last, (W, H)).to(DEV)
    assert all(bool(torch.isfinite(x).all()) for x in _track(est, batch))

    # resume: a run cut after step 2's checkpoint, continued from the files, takes step 3 to the bit
    full = _model(config)
    shots_full = []
    train.fit(full, batches, val, _config(epochs=3), str(tmp_path / 'full'), 'net', val_freq=2,
              log=lambda m: shots_full.append(_snapshot(full)) if 'step' in m else None)
    cut = _model(config)
    train.fit(cut, batches, val, _config(epochs=2), str(tmp_path / 'cut'), 'net', val_freq=2)
    _, cut_last, cut_optim = train.checkpoint_paths(str(tmp_path / 'cut'), 'net')
    resumed = pose_net.PoseNet(config['model'])
    resumed.load_state_dict(torch.load(cut_last, map_location='cpu')['state_dict'])
    resumed = resumed.to(DEV)
    assert not _changed(_snapshot(resumed), shots_full[2])
    r = train.fit(resumed, batches[3:], val, _config(epochs=3), str(tmp_path / 'resumed'), 'net', val_freq=2, resume=cut_optim)
    assert r['total_steps'] == 4 and int(r['optimizer'].steps) == 4
    assert not _changed(_snapshot(resumed), shots_full[3])


def test_fit_skips_a_nan_batch_and_stops_on_a_nan_validation(rpe, tmp_path):
    from rpe_amd import train
    config = _config(epochs=1, freeze_flow_steps=0)
    batches, val = _batches(25, 2), _batches(26, 1)
    poisoned = list(batches[1])
    poisoned[1] = poisoned[1].clone()
    poisoned[1][0, 1, 100, 100] = float('nan')              # one pixel of the target image
    model = _model(config)
    shots = []
    r = train.fit(model, [batches[0], tuple(poisoned)], val, config, str(tmp_path / 'nan'), 'net', val_freq=1000,
                  log=lambda m: shots.append(_snapshot(model)) if 'step' in m else None)
    assert r['total_steps'] == 2 and int(r['optimizer'].skipped) == 1 and int(r['optimizer'].steps) == 1
    assert not _changed(shots[0], shots[1])                 # the poisoned step left every weight as it was
    # a NaN validation loss ends the run at its first validation, before anything is written
    bad_val = list(val[0])
    bad_val[6] = torch.full_like(bad_val[6], float('nan'))  # (nanmean, as the reference's: only a loss without one finite component is NaN)
    model = _model(config)
    r = train.fit(model, batches, [tuple(bad_val)], _config(epochs=10), str(tmp_path / 'nanval'), 'net', val_freq=1)
    assert r['stopped_on_nan'] and r['total_steps'] == 0
    assert not os.path.exists(train.checkpoint_paths(str(tmp_path / 'nanval'), 'net')[1])


def test_supervised_pose_loss_against_float64(rpe):
    """|pred - log(gt)| against oracle/se3.py's log in float64: identity, small motions, a rotation near pi/2; a 7-vector and an SE3."""
    import math
    from oracle import se3 as ose3
    from rpe_amd import se3, train
    g = torch.Generator().manual_seed(3)
    xi = torch.cat((torch.zeros(1, 6), 0.05 * torch.randn(4, 6, generator=g),
                    torch.tensor([[0.3, -0.2, 0.1, math.pi / 2 - 1e-3, 0.0, 0.0], [0.1, 0.2, -0.3, 0.9, -0.9, 0.9]])), dim=0).double()
    gt = ose3.se3_exp(xi)
    pred = (xi + 0.01 * torch.randn(xi.shape, generator=g, dtype=torch.float64)).float()
    want = (pred.double() - ose3.se3_log(gt.float().double())).abs()
    for arg in (gt.float().to(DEV), se3.SE3(gt.float().to(DEV))):
        got = train.supervised_pose_loss(pred.to(DEV), arg)
        assert got.shape == (7, 6) and got.dtype == torch.float32
        # f32 rounding of the components: log's (|xi| <= 1.6) and the subtraction's, a few ulps of the larger operand
        # (the log mixes a pose's components: the scale is the row's largest)
        tol = 8 * torch.finfo(torch.float32).eps * torch.maximum(pred.double().abs(), xi.abs()).amax(dim=1, keepdim=True).clamp(min=1e-3)
        assert bool(((got.cpu().double() - want).abs() <= tol).all()), (got.cpu().double() - want).abs().max()
    assert float(train.supervised_pose_loss(torch.zeros(1, 6, device=DEV), se3.SE3.Identity(1, device=DEV)).abs().max()) == 0.0
    with pytest.raises(ValueError, match='shape'):
        train.supervised_pose_loss(torch.zeros(2, 6, device=DEV), se3.SE3.Identity(1, device=DEV))
