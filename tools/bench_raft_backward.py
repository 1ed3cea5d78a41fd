"""Backward of RAFT's output heads at the bench geometry: 640x512 (64x80 maps), 48 rows (n = 16 x three passes).
Median of 30 after 5 warm-ups, HIP events around each call, everything in one process:
  * every kernel of the tail backward (csrc/raft_backward.hip) and the whole of raft_grad.raft_tail_backward,
  * the weight-gradient GEMM's share of the f32 matrix peak (256 CUs x 4 SIMDs x 64 FLOP / clock at the clock given with --mhz),
  * the same tail's backward through PyTorch-ROCm autograd (conv2d, unfold, softmax).
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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
    ap.add_argument('--rows', type=int, default=48)
    ap.add_argument('--h8', type=int, default=64)
    ap.add_argument('--w8', type=int, default=80)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--mhz', type=float, default=2400.0, help='matrix clock assumed for the peak')
    a = ap.parse_args()
    import rpe_amd  # noqa: F401
    from rpe_amd import ops, raft_grad
    dev = 'cuda'
    b, hh, ww = a.rows, a.h8, a.w8
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    net, low, gup = torch.tanh(r(b, 128, hh, ww)), 3.0 * r(b, 2, hh, ww), r(b, 2, 8 * hh, 8 * ww)
    fh = (r(256, 128, 3, 3) / 34.0, 0.1 * r(256), r(2, 256, 3, 3) / 48.0, 0.1 * r(2))
    mk = (r(256, 128, 3, 3) / 34.0, 0.1 * r(256), r(576, 256, 1, 1) / 4.0, 0.1 * r(576))
    t_f, t_m, m, d_m, g512 = torch.relu(r(b, 256, hh, ww)), torch.relu(r(b, 256, hh, ww)), r(b, 576, hh, ww), r(b, 576, hh, ww), r(b, 512, hh, ww)
    T = lambda fn: timed(fn, a.warmup, a.reps)
    out = dict(rows=b, h8=hh, w8=ww)
    out['upsample_backward_ms'] = T(lambda: ops.upsample_convex_backward(gup, low, m))
    out['wgrad_3x3_128_512_ms'] = T(lambda: ops.conv_bwd_weight(net, g512, (3, 3)))
    out['wgrad_1x1_256_576_ms'] = T(lambda: ops.conv_bwd_weight(t_m, d_m, (1, 1), scale=0.25))
    out['wgrad_3x3_256_2_ms'] = T(lambda: ops.conv_bwd_weight(t_f, low, (3, 3)))
    out['to2_bwd_data_ms'] = T(lambda: ops.conv3x3_to2_bwd_data(low, fh[2], act=t_f, out=g512[:, :256]))
    out['relu_backward_ms'] = T(lambda: ops.relu_backward(g512[:, 256:], t_m))
    out['tail_backward_ms'] = T(lambda: raft_grad.raft_tail_backward(net, low, gup, fh, mk))
    peak = 256 * 4 * 64 * a.mhz * 1e6
    flops = 2.0 * b * hh * ww * 512 * 128 * 9
    out['wgrad_3x3_tflops'] = flops / (out['wgrad_3x3_128_512_ms'] * 1e-3) / 1e12
    out['wgrad_3x3_share_of_f32_matrix_peak'] = flops / (out['wgrad_3x3_128_512_ms'] * 1e-3) / peak

    params = [p.clone().requires_grad_(True) for p in fh + mk]
    netg = net.clone().requires_grad_(True)

    def torch_tail():
        t1 = torch.relu(F.conv2d(netg, params[0], params[1], padding=1))
        delta = F.conv2d(t1, params[2], params[3], padding=1)
        t2 = torch.relu(F.conv2d(netg, params[4], params[5], padding=1))
        mm = 0.25 * F.conv2d(t2, params[6], params[7])
        fl = low + delta
        p = torch.softmax(mm.view(b, 1, 9, 8, 8, hh, ww), dim=2)
        up = F.unfold(8.0 * fl, (3, 3), padding=1).view(b, 2, 9, 1, 1, hh, ww)
        return (p * up).sum(dim=2).permute(0, 1, 4, 2, 5, 3).reshape(b, 2, 8 * hh, 8 * ww)

    def torch_step():
        up = torch_tail()
        torch.autograd.grad((up * gup).sum(), [netg] + params)
    out['torch_forward_ms'] = T(lambda: torch_tail())
    out['torch_forward_backward_ms'] = T(torch_step)
    out['torch_backward_ms'] = out['torch_forward_backward_ms'] - out['torch_forward_ms']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
