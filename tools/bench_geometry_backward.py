"""Times the geometry stage's backward (csrc/geometry_backward.hip) at 640x512, n = 16, on the GPU: the forward kernel pair
(ops.depth_backproject_warp), the hand-written backward (ops.depth_backproject_warp_backward, all four gradients from all four incoming
gradients) and the same backward through PyTorch-ROCm autograd over a torch restatement of the stage built here (float32, on the GPU).
Device events around each call, a warm-up, the median of --reps runs.  The backward's achieved bytes/s is its ALGORITHMIC traffic -- every
input it must read once (time_flow, stereo_flow2, the incoming gradients) and every output it must write once; the lists in its workspace
are not counted -- over its median time.  Prints one JSON line.  There is no CPU path: without a GPU it fails."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_stage(sf2, tf, b, K, d1, i1, i2, sf1):
    """core/pose/pose_net.py:73-79,104-113 with the torch calls the reference makes."""
    n, _, h, w = sf2.shape

    def remap(x):
        row, col = torch.meshgrid(torch.arange(h, device=x.device), torch.arange(w, device=x.device), indexing='ij')
        g = torch.stack((2 * (tf[:, 0] + col) / (w - 1) - 1, 2 * (tf[:, 1] + row) / (h - 1) - 1), dim=-1)
        return F.grid_sample(x, g, align_corners=True)

    def proj(depth):
        xs, ys = torch.arange(w, device=depth.device) + 0.5, torch.arange(h, device=depth.device) + 0.5
        coords = torch.stack((xs[None, :].expand(h, w).reshape(-1), ys[:, None].expand(h, w).reshape(-1), torch.ones(h * w, device=depth.device)))
        return (depth.view(n, 1, -1) * (torch.linalg.inv(K) @ coords[None])).view(n, 3, h, w)
    depth = b[:, None, None] / -sf2[:, 0]
    depth2 = torch.where((depth > 0) & (depth <= 1.0), depth, torch.ones_like(depth)).unsqueeze(1)
    pcl1, pcl2w = proj(d1), remap(proj(depth2))
    inp1 = F.interpolate(torch.cat((sf1, i1, pcl1), dim=1), scale_factor=0.125, mode='bilinear')
    inp2 = F.interpolate(torch.cat((remap(sf2), remap(i2), pcl2w), dim=1), scale_factor=0.125, mode='bilinear')
    return pcl1, pcl2w, inp1, inp2


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=16)
    ap.add_argument('--h', type=int, default=512)
    ap.add_argument('--w', type=int, default=640)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_geometry_backward: needs the GPU (a CPU timing says nothing about it)')
    from rpe_amd import ops
    n, h, w, dev = a.n, a.h, a.w, 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.rand(*s, device=dev, generator=g)                   # noqa: E731
    b = torch.full((n,), 7.2 / 250, device=dev)
    K = torch.tensor([[0.9 * w, 0.0, 0.5 * w], [0.0, 0.9 * w, 0.5 * h], [0.0, 0.0, 1.0]], device=dev).expand(n, 3, 3).contiguous()
    sf2 = torch.stack((-b[:, None, None] / (0.05 + 0.9 * r(n, h, w)), r(n, h, w) - 0.5), dim=1)         # smooth-ish valid depths ...
    sf2[:, 0][r(n, h, w) < 0.1] *= -1                                                                   # ... a tenth clamped
    tf = 6.0 * (r(n, 2, h, w) - 0.5)                                                                    # a few pixels of motion
    sf1, d1 = sf2.flip(0).contiguous(), 0.1 + 0.9 * r(n, 1, h, w)
    i1, i2 = 255 * r(n, 3, h, w), 255 * r(n, 3, h, w)
    m2 = torch.ones(n, 1, h, w, dtype=torch.bool, device=dev)
    ups = [torch.randn(n, 3, h, w, device=dev, generator=g), torch.randn(n, 3, h, w, device=dev, generator=g),
           torch.randn(n, 8, h // 8, w // 8, device=dev, generator=g), torch.randn(n, 8, h // 8, w // 8, device=dev, generator=g)]

    fwd = timed(lambda: ops.depth_backproject_warp(sf2, tf, b, K, d1, i1, i2, sf1, m2), a.warmup, a.reps)
    bwd = timed(lambda: ops.depth_backproject_warp_backward(sf2, tf, b, K, d1, i2, sf1, m2, *ups), a.warmup, a.reps)

    leaves = [t.clone().requires_grad_(True) for t in (sf2, tf, d1, sf1)]
    outs = torch_stage(leaves[0], leaves[1], b, K, leaves[2], i1, i2, leaves[3])
    ref = timed(lambda: torch.autograd.grad(outs, leaves, ups, retain_graph=True), a.warmup, a.reps)

    got = ops.depth_backproject_warp_backward(sf2, tf, b, K, d1, i2, sf1, m2, *ups)
    want = dict(zip(('stereo_flow2', 'time_flow', 'depth1', 'stereo_flow1'), torch.autograd.grad(outs, leaves, ups, retain_graph=True)))
    # cross-check against torch's float32 GPU backward: the share of elements further apart than 1e-4 of the gradient's scale, and the
    # largest difference.  (On random flows a few positions lie within an ulp of a pixel; where the two sides floor such a position
    # differently the position gradient, which jumps there, differs by its own size.  The parity tests judge against float64.)
    agree = {k: dict(share_beyond_1e4=float(((got[k] - want[k]).abs() > 1e-4 * want[k].abs().max()).float().mean()),
                     max=float((got[k] - want[k]).abs().max() / want[k].abs().max())) for k in got}
    floats_per_pixel = (2 + 2 + 3 + 3) + 16 / 64 + (2 + 2 + 2 + 1)        # tf, sf2, grad_pcl1, grad_pcl2w | grad_inp1 + grad_inp2 | four outputs
    nbytes = 4 * floats_per_pixel * n * h * w
    print(json.dumps(dict(tool='bench_geometry_backward', n=n, h=h, w=w, reps=a.reps, forward_ms=round(fwd[0], 4), backward_ms=round(bwd[0], 4),
                          backward_min_ms=round(bwd[1], 4), torch_autograd_backward_ms=round(ref[0], 4), backward_algorithmic_bytes=int(nbytes),
                          backward_GBps=round(nbytes / (bwd[0] * 1e-3) / 1e9, 1), rel_diff_vs_torch_f32=agree)))


if __name__ == '__main__':
    main()
