"""Backward of RAFT's update block at the bench geometry: 640x512 (64x80 maps), with --pairs flow pairs in one pass (2 and 16 are the
figures NOTES.md quotes).  Median of --reps after --warmup, HIP events around each call, everything in one process:
  * every new kernel (csrc/update_backward.hip): the weight-gradient GEMM at 1x5 / 5x1 / 7x7 and the four gate kernels,
  * one raft_grad.update_step_backward,
  * a whole pass with ``grad_update`` (12 iterations) and its backward through time, beside the plain forward of the same pass.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=2)
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    import rpe_amd  # noqa: F401
    from rpe_amd import ops, raft, raft_grad, synth
    dev = 'cuda'
    b, hh, ww = a.pairs, a.height // 8, a.width // 8
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    T = lambda fn: timed(fn, a.warmup, a.reps)
    out = dict(pairs=b, h8=hh, w8=ww, iters=a.iters)
    A, dzr, dq, flow, df1 = r(b, 384, hh, ww), r(b, 256, hh, ww), r(b, 128, hh, ww), r(b, 2, hh, ww), r(b, 128, hh, ww)
    out['wgrad_1x5_384_256_ms'] = T(lambda: ops.conv_bwd_weight(A, dzr, (1, 5)))
    out['wgrad_5x1_384_128_ms'] = T(lambda: ops.conv_bwd_weight(A, dq, (5, 1)))
    out['wgrad_7x7_2_128_ms'] = T(lambda: ops.conv_bwd_weight(flow, df1, (7, 7)))
    h, z, rr, q, t1, t2 = (torch.sigmoid(r(b, 128, hh, ww)) for _ in range(6))
    out['gates_zr_recompute_ms'] = T(lambda: ops.gru_gates_zr_recompute(dzr, h, z, rr, t1))
    out['gates_h_recompute_ms'] = T(lambda: ops.gru_gates_h_recompute(dq, z, h, q, t1))
    out['gates_zq_backward_ms'] = T(lambda: ops.gru_gates_zq_backward(dq, h, z, q, dzr[:, :128], t1, t2))
    out['gates_r_backward_ms'] = T(lambda: ops.gru_gates_r_backward(dq, h, rr, t2, dzr[:, 128:], t1))
    model = synth.init_synthetic_weights(raft.RAFT(synth.model_config(a.height, a.width, iters=a.iters))).eval().to(dev)
    upd = model.update_params()
    hx, inp, corr, d_net = r(b, 256, hh, ww), torch.relu(r(b, 128, hh, ww)), r(b, 324, hh, ww), r(b, 128, hh, ww)
    out['update_step_backward_ms'] = T(lambda: raft_grad.update_step_backward(hx, inp, corr, d_net, upd))
    im1, im2 = (255.0 * torch.rand(b, 3, a.height, a.width, generator=g)).to(dev), (255.0 * torch.rand(b, 3, a.height, a.width, generator=g)).to(dev)
    G = r(b, 2, a.height, a.width)
    for p in model.head_params()[0] + model.head_params()[1] + upd:
        p.requires_grad_(True)
    out['forward_ms'] = T(lambda: model(im1, im2))
    out['forward_grad_update_ms'] = T(lambda: model(im1, im2, grad_update=True))

    def both():
        flows = model(im1, im2, grad_update=True)[0]
        (flows[-1] * G).sum().backward()
    out['forward_backward_ms'] = T(both)
    out['backward_ms'] = out['forward_backward_ms'] - out['forward_grad_update_ms']
    out['backward_over_forward'] = out['backward_ms'] / out['forward_ms']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
