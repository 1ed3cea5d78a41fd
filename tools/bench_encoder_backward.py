"""Backward of RAFT's encoders at the bench geometry, 640x512: raft_grad.encoder_backward for fnet on 3 images and for cnet on 2 (with
its tanh | ReLU output) beside the same encoders' forward, all in one process.  Median of --reps after --warmup, HIP events around each
call.  Every step runs under its own time limit (--limit seconds): a step that exceeds it ends the process with its traceback, and nothing
more is started on the GPU.  No threshold hangs on these numbers.  Prints one JSON line."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, reps, limit):
    faulthandler.dump_traceback_later(limit, exit=True)               # this step's own time limit
    try:
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts)
    finally:
        faulthandler.cancel_dump_traceback_later()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--limit', type=float, default=120.0)
    a = ap.parse_args()
    import rpe_amd  # noqa: F401
    from rpe_amd import raft, raft_grad, synth
    dev = 'cuda'
    model = synth.init_synthetic_weights(raft.RAFT(synth.model_config(a.height, a.width))).eval().to(dev)
    g = torch.Generator().manual_seed(0)
    out = dict(height=a.height, width=a.width)
    for name, enc, n, split in (('fnet', model.fnet, 3, False), ('cnet', model.cnet, 2, True)):
        images = (255.0 * torch.rand(n, 3, a.height, a.width, generator=g)).to(dev)
        with torch.no_grad():
            y = enc(images, raw255=True, split_act=split)
        d_out = torch.randn(y.shape, generator=g).to(dev)
        T = lambda fn: timed(fn, a.warmup, a.reps, a.limit)
        with torch.no_grad():
            out[f'{name}_{n}_forward_ms'] = T(lambda: enc(images, raw255=True, split_act=split))
        out[f'{name}_{n}_backward_ms'] = T(lambda: raft_grad.encoder_backward(enc, images, d_out, raw255=True, split_act=split))
        out[f'{name}_{n}_backward_over_forward'] = out[f'{name}_{n}_backward_ms'] / out[f'{name}_{n}_forward_ms']
        torch.cuda.synchronize()
        out[f'{name}_{n}_peak_gb'] = torch.cuda.max_memory_allocated() / 2 ** 30
    print(json.dumps(out))


if __name__ == '__main__':
    main()
