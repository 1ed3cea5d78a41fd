"""The input side measured: pinned host uint8 frames -> H2D -> ingest -> tracker, at 1280x1024 per eye -> 640x512, conventional
rectification (NOTES.md "Input side from host frames").

  --mode kernel --variant fused|chain --n 1|16    a loop of copies + ingests for a `rocprofv3 --kernel-trace --memory-copy-trace --stats`
                                                   run (kernel and copy times come from the trace); prints the host enqueue time per call
  --mode e2e                                       frames/s of the tracker from pinned host frames: (a) blocking copy + the six-call chain +
                                                   forward, (b) track_host_frames(pipelined=False), (c) pipelined=True, (d) track_sequence on
                                                   resident, prepared device tensors; same process, interleaved repeats, median and range
One JSON line per run.  Needs the GPU; nothing here falls back."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpe_amd  # noqa: E402,F401
from rpe_amd import pose_estimator, pose_net, preprocess as pp, synth, trajectory  # noqa: E402

H, W, SIZE = 1024, 1280, (640, 512)


def calibration(size):
    """A mild stereo calibration for (w, h) images (distortion of an endoscope's order, 4 mm baseline)."""
    w, h = size
    f = 0.85 * w
    K1 = np.array([[f, 0, w / 2 - 3.0], [0, f * 0.998, h / 2 + 2.0], [0, 0, 1]])
    K2 = np.array([[f * 1.004, 0, w / 2 + 4.0], [0, f * 1.001, h / 2 - 1.5], [0, 0, 1]])
    return dict(lkmat=K1, rkmat=K2, ld=np.array([-0.22, 0.09, 0.0012, -0.0007, -0.015]), rd=np.array([-0.20, 0.08, -0.0010, 0.0006, -0.012]),
                R=pp.rodrigues(np.array([0.004, -0.008, 0.003])), T=np.array([-4.2, 0.04, -0.06]), img_size=size)


def host_frames(n, seed=0, pin=True):
    """n stacked BGR uint8 frames (2H, W, 3) in pinned memory: synth's band-limited stereo pairs at 640x512, doubled."""
    fr = synth.stereo_frames(seed, n, SIZE[1], SIZE[0])
    q = lambda t: t.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).repeat_interleave(2, 1).repeat_interleave(2, 2).flip(-1)
    frames = torch.cat((q(fr['image2l']), q(fr['image2r'])), 1).contiguous()
    frames[:, 100:160, 200:280] = 255                                # a specular highlight
    return (frames.pin_memory() if pin else frames), fr['K'][0]


def chain(dev_frame, rect):
    """What a user of the six library calls does today with one stacked BGR frame on the device."""
    left, right = dev_frame[:H].flip(-1).contiguous(), dev_frame[H:].flip(-1).contiguous()
    m = pp.mask_specularities(left)
    l, r, m = pp.ResizeStereo(SIZE)(left, right, m[None])
    l, r = rect(l, r)
    return l[None], r[None], (m != 0)[None]


def chain_calls_only(left, right, rect):
    """The six library calls alone (split and colour order done beforehand): the chain's GPU time without torch's flip kernels."""
    m = pp.mask_specularities(left)
    l, r, m = pp.ResizeStereo(SIZE)(left, right, m[None])
    return rect(l, r) + (m,)


def mode_kernel(args):
    rect = pp.StereoRectifier(calibration(SIZE))
    frames, _ = host_frames(args.n)
    dev = torch.empty_like(frames, device='cuda')
    rgb = [(f[:H].flip(-1).contiguous(), f[H:].flip(-1).contiguous()) for f in frames.cuda()]
    enq = []
    for it in range(args.warmup + args.iters):
        torch.cuda.synchronize()
        dev.copy_(frames, non_blocking=True)                         # the copy's own time and rate: memory-copy trace
        t0 = time.perf_counter()
        if args.variant == 'fused':
            out = pp.ingest_stereo(dev, SIZE, rect, bgr=True)
        else:
            out = [chain_calls_only(l, r, rect) for l, r in rgb]
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if it >= args.warmup:
            enq.append((t1 - t0) * 1e3)
    del out
    print(json.dumps(dict(mode='kernel', variant=args.variant, n=args.n, iters=args.iters, frame_bytes=int(frames[0].numel()),
                          host_enqueue_ms_per_call=statistics.median(enq), host_enqueue_ms_per_frame=statistics.median(enq) / args.n)))


def mode_e2e(args):
    dev = torch.device('cuda:0')
    rect = pp.StereoRectifier(calibration(SIZE))
    frames, K = host_frames(args.frames)
    model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(SIZE[1], SIZE[0], iters=12, lbgfs_iters=20))).eval().to(dev)
    slam = dict(frame2frame=True, depth_clipping=[1, 250], lbgfs_iters=20, conf_weighing=True, reuse_features=True)
    make = lambda: pose_estimator.PoseEstimator(slam, K, 7.2 * 250.0, model, SIZE).to(dev)
    src = [(frames[i], i + 1) for i in range(args.frames)]
    resident = [chain(frames[i].to(dev), rect) for i in range(args.frames)]

    def run_a(est):
        traj = []
        for f, stamp in src:
            l, r, m = chain(f.to(dev), rect)                         # blocking copy from pinned memory, then the six calls
            traj.append(est(l, r, m)[0].vec().reshape(7).cpu())
        return traj

    def run_d(est):
        return [t['camera-pose'] for t in trajectory.track_sequence(est, [(l, r, m.clone(), i) for i, (l, r, m) in enumerate(resident)])[1:]]
    runs = {'a_chain_blocking_copy_forward': run_a,
            'b_host_frames_forward': lambda est: [t['camera-pose'] for t in trajectory.track_host_frames(
                est, src, pp.HostFrameIngest(SIZE, rect, depth=2, bgr=True), pipelined=False)[1:]],
            'c_host_frames_pipelined': lambda est: [t['camera-pose'] for t in trajectory.track_host_frames(
                est, src, pp.HostFrameIngest(SIZE, rect, depth=2, bgr=True), pipelined=True)[1:]],
            'd_resident_track_sequence': run_d}
    fps = {k: [] for k in runs}
    poses = {}
    for rep in range(args.warmup + args.repeats):
        for name, fn in runs.items():                                # interleaved: every repeat runs all four
            est = make()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            traj = fn(est)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            poses[name] = torch.stack(traj)
            if rep >= args.warmup:
                fps[name].append(args.frames / dt)
    same = all(torch.equal(poses['a_chain_blocking_copy_forward'], p) for p in poses.values())
    res = {k: dict(median_fps=statistics.median(v), min_fps=min(v), max_fps=max(v), ms_per_frame=1e3 / statistics.median(v)) for k, v in fps.items()}
    print(json.dumps(dict(mode='e2e', frames=args.frames, repeats=args.repeats, same_poses_all_routes=same, **res)))
    assert same, 'the four routes must give one trajectory'


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['kernel', 'e2e'], required=True)
    ap.add_argument('--variant', choices=['fused', 'chain'], default='fused')
    ap.add_argument('--n', type=int, default=1)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ingest.py measures on the GPU'
    (mode_kernel if a.mode == 'kernel' else mode_e2e)(a)
