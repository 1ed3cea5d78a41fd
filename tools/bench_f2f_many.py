"""Frame-to-frame tracking of K sequences at 640x512 (seeded synthetic weights and frames, 12 GRU iterations): MultiPoseEstimator
advancing K sequences in lockstep, against K PoseEstimators run one after another, in the same process, with ``warm_start`` off and on.

Per ``warm_start`` setting and K (default 1, 2, 4, 8, 16) both sides are built and warmed up (``--warmup`` untimed frames per sequence),
then timed in ``--rounds`` alternating rounds (batched, sequential, batched, ...) of ``--steps`` frames per sequence each; the trackers
keep their state from round to round.  Reported per row:
  batched_fps        aggregate frames/s of the lockstep run, K * steps / wall clock of a round: median over the rounds, and [min, max]
  sequential_fps     the same frames through the K single trackers, one sequence after the other: median and [min, max]
  speedup            median batched_fps / median sequential_fps
  step_ms            HIP events on the stream around each lockstep ``est(...)`` call (it ends with the step's one host synchronisation):
                     GPU ms per lockstep frame, median over all rounds
  accepted           rows the gate accepted / rows, over the timed lockstep frames

Sequence k reads the four synthetic frames starting at frame k (mod 4), so the rows of a batch differ.

Usage:  python tools/bench_f2f_many.py [--ks 1,2,4,8,16] [--steps 20] [--warmup 5] [--rounds 3] [--lbgfs 20] [--json out.json]   (bench.py is unchanged)
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
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--lbgfs', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import torch
    import rpe_amd  # noqa: F401
    from rpe_amd import pose_estimator, pose_net, synth
    dev = torch.device('cuda:0')
    H, W = 512, 640
    model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(H, W, iters=12, lbgfs_iters=a.lbgfs))).eval().to(dev)
    s = synth.stereo_frames(3, 4, H, W)
    K0, bf = s['K'][0], float(s['baseline'][0]) * 250.0
    L, R, M = (s[k].to(dev) for k in ('image2l', 'image2r', 'mask2'))
    med = lambda v: sorted(v)[len(v) // 2]                                 # noqa: E731

    results = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for warm in (False, True):
            cfg = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=a.lbgfs, conf_weighing=True, warm_start=warm)
            for n in (int(k) for k in a.ks.split(',')):
                multi = pose_estimator.MultiPoseEstimator(cfg, K0.expand(n, 3, 3), torch.tensor([bf] * n), model, (W, H)).to(dev)
                ones = [pose_estimator.PoseEstimator(cfg, K0, bf, model, (W, H)).to(dev) for _ in range(n)]
                spans, accepted = [], [0, 0]

                def batched(i0, count, timed):
                    for i in range(i0, i0 + count):
                        idx = [(k + i) % 4 for k in range(n)]
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        ok = multi(L[idx], R[idx], M[idx].clone())[1]
                        e1.record()
                        if timed:
                            spans.append((e0, e1))
                            accepted[0] += int(ok.sum())
                            accepted[1] += n

                def sequential(i0, count):
                    for k, one in enumerate(ones):
                        for i in range(i0, i0 + count):
                            j = (k + i) % 4
                            one(L[j:j + 1], R[j:j + 1], M[j:j + 1].clone())

                def wall(f):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0
                batched(0, a.warmup, False)
                sequential(0, a.warmup)
                fps = {'batched': [], 'sequential': []}
                for rnd in range(a.rounds):
                    i0 = a.warmup + rnd * a.steps
                    fps['batched'].append(n * a.steps / wall(lambda: batched(i0, a.steps, True)))
                    fps['sequential'].append(n * a.steps / wall(lambda: sequential(i0, a.steps)))
                row = dict(warm_start=warm, k=n, batched_fps=med(fps['batched']), batched_fps_range=[min(fps['batched']), max(fps['batched'])],
                           sequential_fps=med(fps['sequential']), sequential_fps_range=[min(fps['sequential']), max(fps['sequential'])],
                           speedup=med(fps['batched']) / med(fps['sequential']), step_ms_median=med([x.elapsed_time(y) for x, y in spans]),
                           accepted=accepted)
                print(json.dumps(row), flush=True)
                results.append(row)
                del multi, ones
                torch.cuda.empty_cache()
    out = dict(h=H, w=W, gru_iters=12, lbgfs_iters=a.lbgfs, steps=a.steps, warmup=a.warmup, rounds=a.rounds, rows=results)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f)


if __name__ == '__main__':
    main()
