#!/usr/bin/env python3
"""Sequential tracking throughput (the reference's real use: one stereo frame at a time, batch 1):
PoseEstimator over a synthetic sequence, with and without streaming encoder-feature reuse.
``--quality``: instead, ``report_quality`` off and on (reuse_features on), alternating in this process: median frames/s of REPS runs each,
their spread, and the difference per frame.
``--alternate-corr``: instead, RAFT's ``alternate_corr`` off and on (reuse_features on), each model warmed up, then one timed run each."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpe_amd
from rpe_amd import pose_estimator, pose_net, synth

dev = torch.device('cuda:0')
H, W, F = 512, 640, 24
cfg = synth.model_config(H, W, lbgfs_iters=20)          # configuration/infer_f2f.yaml:11 lbgfs_iters: 20
model = synth.init_synthetic_weights(pose_net.PoseNet(cfg)).eval().to(dev)
fr = synth.stereo_frames(77, F, H, W)
frames = [(fr['image2l'][i:i + 1].to(dev), fr['image2r'][i:i + 1].to(dev), fr['mask2'][i:i + 1].to(dev)) for i in range(F)]


def run(slam):
    est = pose_estimator.PoseEstimator(slam, fr['K'][0], 7.2 * 250.0, model, (W, H)).to(dev)
    import warnings
    torch.cuda.synchronize(); t = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for l, r, m in frames:
            est(l, r, m.clone())
    torch.cuda.synchronize()
    return time.perf_counter() - t


if '--alternate-corr' in sys.argv:
    base = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=20, conf_weighing=True, reuse_features=True)
    model_on = pose_net.PoseNet(dict(cfg, alternate_corr=True)).eval().to(dev)
    model_on.load_state_dict(model.state_dict())
    models = {False: model, True: model_on}
    for on in (False, True):
        model = models[on]
        run(base)                                                             # warm-up
        dt = min(run(base) for _ in range(3))
        print(f'alternate_corr={on}: {F / dt:.1f} frames/s ({1e3 * dt / F:.2f} ms/frame; best of 3 runs of {F} frames), 640x512, 12 GRU iters, L-BFGS 20')
    sys.exit(0)

if '--quality' in sys.argv:
    import statistics
    REPS = 7
    base = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=20, conf_weighing=True, reuse_features=True)
    run(base), run(dict(base, report_quality=True))                       # warm-up of both
    ms = {False: [], True: []}
    for rep in range(REPS):
        for on in (False, True):
            ms[on].append(1e3 * run(dict(base, report_quality=on)) / F)
    for on in (False, True):
        v = sorted(ms[on])
        print(f'report_quality={on}: median {1e3 / statistics.median(v):.1f} frames/s ({statistics.median(v):.3f} ms/frame; min {v[0]:.3f}, max {v[-1]:.3f} over '
              f'{REPS} runs of {F} frames), 640x512, 12 GRU iters, L-BFGS 20')
    d = statistics.median(ms[True]) - statistics.median(ms[False])
    print(f'report_quality on - off: {1e3 * d:+.1f} us/frame ({100 * d / statistics.median(ms[False]):+.2f} %)')
    sys.exit(0)

for reuse in (False, True):
    slam = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=20, conf_weighing=True, reuse_features=reuse)
    for rep in range(2):
        est = pose_estimator.PoseEstimator(slam, fr['K'][0], 7.2 * 250.0, model, (W, H)).to(dev)
        torch.cuda.synchronize(); t = time.perf_counter()
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for l, r, m in frames:
                est(l, r, m.clone())
        torch.cuda.synchronize(); dt = time.perf_counter() - t
    print(f'reuse_features={reuse}: {F / dt:.1f} frames/s ({1e3 * dt / F:.2f} ms/frame), 640x512, 12 GRU iters, L-BFGS 20')
