"""Frame-to-model tracking of K sequences at 640x512 (seeded synthetic weights and frames, 12 GRU iterations): MultiSurfelPoseEstimator
advancing K sequences in lockstep, against K SurfelPoseEstimators run one after another in the same process.

Per K (default 1, 2, 4, 8, 16):
  batched_fps        aggregate frames/s of the lockstep run: K * timed steps / wall clock (``--warmup`` steps first, untimed)
  step_ms            HIP events on the stream around each lockstep ``est(...)`` call (it ends with the step's one host
                     synchronisation): GPU ms per lockstep frame, median
  render_ms, fuse_ms HIP events around surfel_map.render_many / fuse_many inside the step, median; upkeep_fraction = their sum / step_ms
  sequential_fps     the same frames through K single trackers, one sequence after the other (each with its own warm-up, untimed)
  speedup            batched_fps / sequential_fps
  map_count          the surfel count of every map after the last timed step

Sequence k reads the four synthetic frames starting at frame k (mod 4), so the rows of a batch differ.

Usage:  python tools/bench_f2m_many.py [--ks 1,2,4,8,16] [--steps 20] [--warmup 5] [--lbgfs 20] [--json out.json]   (bench.py is unchanged)
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
    ap.add_argument('--ks', default='1,2,4,8,16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--lbgfs', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import torch
    import rpe_amd  # noqa: F401
    from rpe_amd import pose_estimator, pose_net, synth, surfel_map
    dev = torch.device('cuda:0')
    H, W = 512, 640
    model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(H, W, iters=12, lbgfs_iters=a.lbgfs))).eval().to(dev)
    s = synth.stereo_frames(3, 4, H, W)
    cfg = dict(frame2frame=False, depth_clipping=[1, 250], lbgfs_iters=a.lbgfs, conf_weighing=True, dist_thr=0.05, average_pts=True)
    K0, bf = s['K'][0], float(s['baseline'][0]) * 250.0
    L, R, M = (s[k].to(dev) for k in ('image2l', 'image2r', 'mask2'))
    med = lambda v: sorted(v)[len(v) // 2] if v else float('nan')          # noqa: E731
    ev = {'render': [], 'fuse': []}
    orig = {'render': surfel_map.render_many, 'fuse': surfel_map.fuse_many}

    def timed(name):
        def w(*x, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = orig[name](*x, **k)
            e1.record()
            ev[name].append((e0, e1))
            return r
        return w

    def step_frames(n, i):
        idx = [(k + i) % 4 for k in range(n)]
        return L[idx], R[idx], M[idx].clone()

    results = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for n in (int(k) for k in a.ks.split(',')):
            est = pose_estimator.MultiSurfelPoseEstimator(cfg, K0.expand(n, 3, 3), torch.tensor([bf] * n), model, (W, H)).to(dev)
            for i in range(a.warmup):
                est(*step_frames(n, i))
            ev['render'].clear()
            ev['fuse'].clear()
            surfel_map.render_many, surfel_map.fuse_many = timed('render'), timed('fuse')
            spans, ok = [], 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.warmup, a.warmup + a.steps):
                f0, f1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                f0.record()
                _, succ, _, _, _ = est(*step_frames(n, i))
                f1.record()
                spans.append((f0, f1))
                ok += int(succ.sum())
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            surfel_map.render_many, surfel_map.fuse_many = orig['render'], orig['fuse']
            step_ms = med([x.elapsed_time(y) for x, y in spans])
            r_ms = med([x.elapsed_time(y) for x, y in ev['render']])
            f_ms = med([x.elapsed_time(y) for x, y in ev['fuse']])
            counts = [m.n for m in est.scenes]
            del est
            torch.cuda.empty_cache()
            # the same frames through K single trackers, one after another
            seq_wall = 0.0
            for k in range(n):
                one = pose_estimator.SurfelPoseEstimator(cfg, K0, bf, model, (W, H)).to(dev)
                for i in range(a.warmup):
                    one(L[(k + i) % 4:(k + i) % 4 + 1], R[(k + i) % 4:(k + i) % 4 + 1], M[(k + i) % 4:(k + i) % 4 + 1].clone())
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.warmup, a.warmup + a.steps):
                    j = (k + i) % 4
                    one(L[j:j + 1], R[j:j + 1], M[j:j + 1].clone())
                torch.cuda.synchronize()
                seq_wall += time.perf_counter() - t0
                del one
                torch.cuda.empty_cache()
            row = dict(k=n, batched_fps=n * a.steps / wall, step_ms_median=step_ms, render_ms_median=r_ms, fuse_ms_median=f_ms,
                       upkeep_fraction=(r_ms + f_ms) / step_ms, sequential_fps=n * a.steps / seq_wall,
                       speedup=(n * a.steps / wall) / (n * a.steps / seq_wall), successes=ok, map_count=counts)
            print(json.dumps(row), flush=True)
            results.append(row)
    out = dict(h=H, w=W, gru_iters=12, lbgfs_iters=a.lbgfs, steps=a.steps, warmup=a.warmup, rows=results)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f)


if __name__ == '__main__':
    main()
