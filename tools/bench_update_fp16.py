#!/usr/bin/env python3
"""RAFT's ``update_fp16`` (the update block's convolutions with fp16 operands, rpe_conv_f16) beside the f32 route, in one process:
  * per covered layer at 64 x 80 with 32 pairs and with 2 pairs: rpe_conv_f16 beside the f32 route's kernel for that layer;
  * the update-loop pass (RAFT.forward on given encoder outputs: pyramid build, context terms, 12 iterations, mask head, up-sampling),
    RAFT.forward, the PoseNet.infer step at 16 frame pairs and sequential tracking, each with the flag off and on (640 x 512);
  * D16 = max|flow_on - flow_off| of RAFT's final flow beside what mixed_precision moves it (seeded synthetic weights).
HIP events around repeated launches, as the other tools.
    python tools/bench_update_fp16.py"""
import os, sys, time, warnings
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpe_amd  # noqa: F401
from rpe_amd import ops, pose_estimator, pose_net, raft, synth

dev = torch.device('cuda:0')
torch.manual_seed(0)
H8, W8 = 64, 80


def t(fn, reps=20, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3                  # us


def layer(name, n, ci, co, kh, kw, mode):
    """(f32 route's kernel, its time, rpe_conv_f16's time) for one covered layer at batch n."""
    x = torch.randn(n, ci, H8, W8, device=dev)
    wt, bias = torch.randn(co, ci, kh, kw, device=dev) * 0.05, torch.randn(co, device=dev) * 0.1
    c = co // 2 if mode == ops.CONV_GATE_ZR else co
    out, out2 = torch.empty(n, c, H8, W8, device=dev), torch.empty(n, c, H8, W8, device=dev)
    kw_ = {}
    if mode in (ops.CONV_GATE_ZR, ops.CONV_GATE_H):
        hid = torch.randn(n, c, H8, W8, device=dev)
        kw_ = dict(add=torch.randn(n, co, H8, W8, device=dev), hidden=hid)
        kw_.update(dict(out2=out2, gate_channels=c) if mode == ops.CONV_GATE_ZR else dict(zgate=torch.rand(n, c, H8, W8, device=dev)))
        bias = None                                         # (the loop's gate launches: the bias is part of the context term)
    p16 = ops.PackedConvF16(wt, bias)
    if (kh, kw) == (1, 1):
        c11 = ops.Conv1x1(wt, bias)
        f32, kern = (lambda: c11(x, mode, out)), 'rpe_conv1x1' if n * -(-(H8 * W8) // 128) * -(-co // 128) >= 512 else 'rpe_conv_fused'
    elif (kh, kw) == (3, 3):
        p = ops.PackedWino24(wt, bias)
        f32, kern = (lambda: ops.conv_wino(x, p, mode, out)), 'rpe_conv_wino24'
    else:
        p = ops.PackedWino1d(wt, bias)
        f32, kern = (lambda: ops.conv_wino1d(x, p, mode, out, **kw_)), 'rpe_conv_wino1d'
    t32 = t(f32)
    t16 = t(lambda: ops.conv_fused(x, p16, mode, out, **kw_))
    print('%-7s b%-2d %3d->%3d %dx%d   %-16s %8.1f us   rpe_conv_f16 %8.1f us   f16 / f32 %.3f' % (name, n, ci, co, kh, kw, kern, t32, t16, t16 / t32), flush=True)


LAYERS = (('convc1', 324, 256, 1, 1, ops.CONV_RELU), ('convc2', 256, 192, 3, 3, ops.CONV_RELU), ('convf2', 128, 64, 3, 3, ops.CONV_RELU),
          ('conv', 256, 126, 3, 3, ops.CONV_RELU), ('zr1', 256, 256, 1, 5, ops.CONV_GATE_ZR), ('q1', 256, 128, 1, 5, ops.CONV_GATE_H),
          ('zr2', 256, 256, 5, 1, ops.CONV_GATE_ZR), ('q2', 256, 128, 5, 1, ops.CONV_GATE_H), ('fh1', 128, 256, 3, 3, ops.CONV_RELU),
          ('mask0', 128, 256, 3, 3, ops.CONV_RELU), ('mask2', 256, 576, 1, 1, ops.CONV_LINEAR))

with torch.no_grad():
    for n in (32, 2):
        for spec in LAYERS:
            layer(spec[0], n, *spec[1:])

    H, W = 512, 640
    cfg = synth.model_config(H, W, lbgfs_iters=8)
    models = {False: synth.init_synthetic_weights(pose_net.PoseNet(cfg)).eval().to(dev)}
    for key in ('update_fp16', 'mixed_precision'):
        models[key] = pose_net.PoseNet(dict(cfg, **{key: True})).eval().to(dev)
        models[key].load_state_dict(models[False].state_dict())
    models[True] = models['update_fp16']

    for pairs in (32, 2):
        fr = synth.stereo_frames(5, pairs, H, W)
        i1, i2 = fr['image1l'].to(dev), fr['image2l'].to(dev)
        flows = {}
        for on in (False, True):
            net = models[on].flow
            f = net.encode_features((i1, i2))
            fm, cn = (f[:pairs].contiguous(), f[pairs:].contiguous()), net.encode_context(i1)
            loop = t(lambda: net(None, None, fmaps=fm, cnet=cn), reps=5, warm=4)
            full = t(lambda: net(i1, i2), reps=5, warm=2)
            flows[on] = net(i1, i2)[0][-1]
            print(f'RAFT {W}x{H}, {pairs} pairs, update_fp16={on}: update-loop pass (encoders given) {loop / 1e3:8.2f} ms   RAFT.forward {full / 1e3:8.2f} ms', flush=True)
        if pairs == 2:
            mp = models['mixed_precision'].flow(i1, i2)[0][-1]
            print(f'final flow against the f32 model ({W}x{H}, {pairs} pairs, 12 iterations, seeded weights): D16 = max|flow_on - flow_off| = '
                  f'{float((flows[True] - flows[False]).abs().max()):.3e} px (mean |.| {float((flows[True] - flows[False]).abs().mean()):.3e}); mixed_precision moves it '
                  f'{float((mp - flows[False]).abs().max()):.3e} px (mean {float((mp - flows[False]).abs().mean()):.3e})', flush=True)

    fr = synth.stereo_frames(6, 16, H, W)
    ga = {k: v.to(dev) for k, v in synth.infer_args(fr).items()}
    for on in (False, True):
        print(f'PoseNet.infer, 16 frame pairs, update_fp16={on}: {t(lambda: models[on].infer(**ga), reps=5, warm=3) / 1e3:8.2f} ms', flush=True)

    F = 24
    fr = synth.stereo_frames(77, F, H, W)
    frames = [(fr['image2l'][i:i + 1].to(dev), fr['image2r'][i:i + 1].to(dev), fr['mask2'][i:i + 1].to(dev)) for i in range(F)]
    slam = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=8, conf_weighing=True, reuse_features=True)

    def run(model):
        est = pose_estimator.PoseEstimator(slam, fr['K'][0], 7.2 * 250.0, model, (W, H)).to(dev)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for l, r, m in frames:
                est(l, r, m.clone())
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for on in (False, True):
        run(models[on])
        dt = min(run(models[on]) for _ in range(3))
        print(f'sequential tracking, update_fp16={on}: {F / dt:.1f} frames/s ({1e3 * dt / F:.2f} ms/frame; best of 3 runs of {F} frames), {W}x{H}, 12 GRU iters, L-BFGS 8', flush=True)
