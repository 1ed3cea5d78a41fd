"""Frame-to-model tracking at 640x512 (SurfelPoseEstimator, seeded synthetic weights and frames, 12 GRU iterations): frames/s, GPU ms
per frame, the map's size over the sequence and the per-frame time of the map's render and fuse (HIP events around each).

  frames/s      wall clock over the timed frames only (``--warmup`` frames first, untimed: allocation, first launches)
  frame_ms      HIP events recorded on the stream before and after each ``est(...)`` call.  The call ends with the gate's host
                synchronisation, so this span is the frame's whole stream time including the gaps in which the GPU waits for the
                host to launch; it is the denominator of ``upkeep_fraction``
  (the kernel time of one frame, launch by launch, comes from a rocprofv3 run of this script and tools/f2m_frame_table.py)
  map_count     the true surfel count after each timed frame (copied on the device per frame, read once at the end)

Usage:  python tools/bench_f2m.py [--frames 60] [--warmup 10] [--lbgfs 20] [--json out.json]      (bench.py is unchanged)
"""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--lbgfs', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import torch
    import rpe_amd  # noqa: F401
    from rpe_amd import pose_estimator, pose_net, synth, surfel_map
    dev = torch.device('cuda:0')
    H, W = 512, 640
    model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(H, W, iters=12, lbgfs_iters=a.lbgfs)))
    s = synth.stereo_frames(3, 4, H, W)
    cfg = dict(frame2frame=False, depth_clipping=[1, 250], lbgfs_iters=a.lbgfs, conf_weighing=True, dist_thr=0.05, average_pts=True)
    est = pose_estimator.SurfelPoseEstimator(cfg, s['K'][0], float(s['baseline'][0]) * 250.0, model, (W, H)).to(dev)
    frames = [(s['image2l'][i:i + 1].to(dev), s['image2r'][i:i + 1].to(dev), s['mask2'][i:i + 1].to(dev)) for i in range(4)]
    ev = {k: [] for k in ('render', 'fuse')}
    cls = surfel_map.SurfelMap
    orig_r, orig_f = cls.render_transformed, cls.fuse

    def timed(name, fn):
        def w(*x, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*x, **k)
            e1.record()
            ev[name].append((e0, e1))
            return r
        return w
    counts, ms, ok = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i in range(a.warmup):
            est(*frames[i % 4])
        cls.render_transformed, cls.fuse = timed('render', orig_r), timed('fuse', orig_f)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.warmup, a.warmup + a.frames):
            f0, f1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            f0.record()
            est(*frames[i % 4])
            f1.record()
            ms.append((f0, f1))
            ok.append(est.success)
            counts.append(est.scene._cnt[est.scene._cur][:1].clone())        # device copy: no host synchronisation
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    cls.render_transformed, cls.fuse = orig_r, orig_f
    med = lambda v: sorted(v)[len(v) // 2] if v else float('nan')
    frame_ms = [x.elapsed_time(y) for x, y in ms]
    r_ms = [x.elapsed_time(y) for x, y in ev['render']]
    f_ms = [x.elapsed_time(y) for x, y in ev['fuse']]
    out = dict(frames=a.frames, warmup=a.warmup, lbgfs_iters=a.lbgfs, frames_per_s=a.frames / wall, wall_ms_per_frame=1e3 * wall / a.frames,
               frame_ms_median=med(frame_ms), render_ms_median=med(r_ms), fuse_ms_median=med(f_ms),
               upkeep_fraction=(med(r_ms) + med(f_ms)) / med(frame_ms), successes=sum(ok), map_count=[int(c) for c in torch.cat(counts).cpu()],
               capacity=est.scene.capacity)
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f)


if __name__ == '__main__':
    main()
