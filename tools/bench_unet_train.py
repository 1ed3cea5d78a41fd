"""One TinyUNet(264) head, forward + backward, on the two training routes in one process: the hand-written kernels
(unet.TinyUNet.train_hip, csrc/unet_train.hip) against forward_train on PyTorch-ROCm ops.  80x64 grid (640x512 images), n = 1, 4, 16,
norms in train mode.  Per shape: both routes warmed up, then timed in alternating rounds with device events around ``--steps`` steps
each; the median round and the spread are printed, one JSON line per shape.  Needs the GPU.

    python tools/bench_unet_train.py [--steps 20] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpe_amd  # noqa: E402,F401
from rpe_amd import unet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_unet_train needs the GPU: a CPU run says nothing about either route')
    torch.manual_seed(0)
    h8, w8, out = 64, 80, (512, 640)
    for n in (1, 4, 16):
        net = unet.TinyUNet(264, out).cuda().train()
        x = torch.randn(n, 264, h8, w8, device='cuda')
        g = torch.randn(n, 1, *out, device='cuda')

        def step(hip):
            net.train_hip = hip
            net.zero_grad(set_to_none=True)
            net(x).backward(g)

        def timed(hip):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(hip)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.steps
        for hip in (True, False):
            for _ in range(a.warmup):
                step(hip)
        torch.cuda.synchronize()
        t = {True: [], False: []}
        for _ in range(a.rounds):
            for hip in (True, False):
                t[hip].append(timed(hip))
        print(json.dumps({'n': n, 'grid': [h8, w8], 'steps': a.steps, 'rounds': a.rounds,
                          'hip_ms': round(statistics.median(t[True]), 4), 'hip_ms_min_max': [round(min(t[True]), 4), round(max(t[True]), 4)],
                          'torch_ms': round(statistics.median(t[False]), 4), 'torch_ms_min_max': [round(min(t[False]), 4), round(max(t[False]), 4)],
                          'hip_over_torch': round(statistics.median(t[True]) / statistics.median(t[False]), 3)}), flush=True)


if __name__ == '__main__':
    main()
