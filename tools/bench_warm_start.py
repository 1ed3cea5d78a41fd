#!/usr/bin/env python3
"""Warm start of the temporal RAFT pass (slam config ``warm_start: True``): what it costs and what it can buy, on one GPU.

  * ops.forward_interpolate (rpe_flow_forward_interpolate): median us over HIP events at (rows, 1/8 map) = (1, 64x80), (16, 64x80),
    (64, 64x80), (1, 128x160);
  * the frame-to-frame tracker at 640x512 (12 GRU iterations, L-BFGS 20), warm vs cold: GPU ms per frame (HIP events around
    PoseEstimator.forward), host enqueue ms per frame (until the last launch is handed to the runtime), library calls per frame (and the
    ops the launch lists carry) -- the warm start's overhead at equal iterations;
  * frames/s of the warm tracker at 6 GRU iterations vs the cold one at 12 -- SPEED ONLY.  The weights are seeded random-init (the trained
    checkpoint is not available), so whether 6 warm iterations are as accurate as 12 cold ones cannot be measured here.
Prints one JSON line."""
import json
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpe_amd  # noqa: E402,F401
from rpe_amd import _lib, ops, pose_estimator, pose_net, synth  # noqa: E402

DEV = torch.device('cuda:0')
H, W, F = 512, 640, 16


def interp_us(n, h, w, reps=30):
    g = torch.Generator().manual_seed(n * 7 + h)
    flow = (torch.rand(n, 2, h, w, generator=g) * 6.0 - 3.0).to(DEV)
    out = torch.empty_like(flow)
    for _ in range(3):
        ops.forward_interpolate(flow, out=out)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.forward_interpolate(flow, out=out)
        e1.record()
        torch.cuda.synchronize()
        ts.append(1e3 * e0.elapsed_time(e1))
    return statistics.median(ts)


def walk(model, frames, K, warm, iters):
    """One tracker over the frames (twice: the second walk is timed).  Per steady-state frame (2..F-1): GPU ms, host enqueue ms; frames/s
    of the timed walk; the library calls of one steady-state frame; how many temporal passes ran warm."""
    model.flow.iters = iters
    slam = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=20, conf_weighing=True, warm_start=warm)
    for rep in range(2):
        est = pose_estimator.PoseEstimator(slam, K, 7.2 * 250.0, model, (W, H)).to(DEV)
        rec, n_warm = [], 0
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i, (l, r, m) in enumerate(frames):
            n_warm += int(warm and est._flow_low is not None)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            est(l, r, m.clone())
            e1.record()
            if i >= 2:
                rec.append((est.t_enqueued - t0, e0, e1))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
    with _lib.CountingLib() as c:
        l, r, m = frames[2]
        est(l, r, m.clone())
    torch.cuda.synchronize()
    return dict(gpu_ms_per_frame=statistics.median([a.elapsed_time(b) for _, a, b in rec]),
                host_enqueue_ms_per_frame=1e3 * statistics.median([h for h, _, _ in rec]), fps=F / dt,
                library_calls_per_frame=c.calls, list_ops_per_frame=c.list_ops, warm_passes=n_warm, frames=F, iters=iters)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    res = {'forward_interpolate_us': {}}
    for n, h, w in ((1, 64, 80), (16, 64, 80), (64, 64, 80), (1, 128, 160)):
        res['forward_interpolate_us'][f'{n}x{h}x{w}'] = round(interp_us(n, h, w), 1)
        print(f'forward_interpolate {n} x {h}x{w}: {res["forward_interpolate_us"][f"{n}x{h}x{w}"]:.1f} us', flush=True)
    cfg = synth.model_config(H, W, iters=12, lbgfs_iters=20)
    model = synth.init_synthetic_weights(pose_net.PoseNet(cfg)).eval().to(DEV)
    fr = synth.stereo_frames(77, F, H, W)
    frames = [(fr['image2l'][i:i + 1].to(DEV), fr['image2r'][i:i + 1].to(DEV), fr['mask2'][i:i + 1].to(DEV)) for i in range(F)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for name, warm, iters in (('cold_12', False, 12), ('warm_12', True, 12), ('warm_6', True, 6)):
            res[name] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in walk(model, frames, fr['K'][0], warm, iters).items()}
            print(name, res[name], flush=True)
    res['note'] = ('640x512, batch 1, L-BFGS 20, seeded random-init weights: speed only -- the accuracy of fewer warm iterations is not '
                   'measured (no trained checkpoint)')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
