#!/usr/bin/env python3
"""The on-the-fly correlation route (ops.AltCorr, RAFT's alternate_corr) against the pyramid route, both in one process and alternated:
prepare vs build and lookup vs lookup per launch (HIP events, median of 20 launches after a warm-up, smooth sub-pixel flow), and the peak
of torch.cuda.max_memory_allocated over one RAFT.forward with the flag off and on.  ``--sizes 640x512,1280x1024 --pairs 2,32`` (defaults);
``--no-forward`` skips the memory part.  ``--fp16``: the same table with the fp16 route (ops.AltCorr(fp16=True), RAFT's alt_corr_fp16)
beside the f32 alt route and the pyramid route, all three alternated in the same process, and the forward peak of alternate_corr with
alt_corr_fp16 off and on (the pyramid model's peak is the table without the flag)."""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpe_amd
from rpe_amd import ops, raft, synth

ap = argparse.ArgumentParser()
ap.add_argument('--sizes', default='640x512,1280x1024')
ap.add_argument('--pairs', default='2,32')
ap.add_argument('--no-forward', action='store_true')
ap.add_argument('--fp16', action='store_true')
args = ap.parse_args()
dev = torch.device('cuda:0')
N = 20


def timed(fns, n=N, warm=3):
    """Median microseconds of each callable, the callables alternated launch by launch."""
    for _ in range(warm):
        for fn in fns:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for _ in fns]
    for i in range(n):
        for k, fn in enumerate(fns):
            a, b = ev[k][i]
            a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) for a, b in e) * 1e3 for e in ev]


for size in args.sizes.split(','):
    W, H = (int(v) for v in size.split('x'))
    h8, w8 = H // 8, W // 8
    for b in (int(v) for v in args.pairs.split(',')):
        g = torch.Generator(device='cpu').manual_seed(1)
        f1, f2 = torch.randn(b, 256, h8, w8, generator=g).to(dev), torch.randn(b, 256, h8, w8, generator=g).to(dev)
        ys, xs = torch.meshgrid(torch.arange(h8), torch.arange(w8), indexing='ij')
        co = (torch.stack((xs, ys)).float()[None].repeat(b, 1, 1, 1) + 0.37 + torch.randn(b, 2, h8, w8, generator=g) * 0.05).to(dev)
        pyr, alt = ops.CorrPyramid(b, h8, w8, device=dev), ops.AltCorr(b, 256, h8, w8, device=dev)
        t_build, t_prep = timed([lambda: pyr.build(f1, f2), lambda: alt.build(f1, f2)], n=N if b * h8 * w8 < 200000 else 5, warm=1)
        out_p, out_a = torch.empty(b, 324, h8, w8, device=dev), torch.empty(b, 324, h8, w8, device=dev)
        lk_p, lk_a = pyr.lookup(co, out=out_p, prepare=True), alt.lookup(co, out=out_a, prepare=True)
        t_lp, t_la = timed([lk_p, lk_a])
        err = float((out_p - out_a).abs().max())
        flop = 2.0 * b * 256 * sum(64 * min(20 * 19, (h8 >> l) * (w8 >> l)) for l in range(4)) * (-(-h8 // 8)) * (-(-w8 // 8))     # upper bound: full boxes
        useful = 2.0 * b * h8 * w8 * 4 * 100 * 256
        print(f'{W}x{H}, {b} pairs: build {t_build:.0f} us, prepare {t_prep:.0f} us; lookup pyramid {t_lp:.1f} us, alt {t_la:.1f} us (x{t_la / t_lp:.1f}; '
              f'{t_la / b:.1f} us per pair); alt = {useful / t_la * 1e-6:.1f} TFLOP/s of window products ({flop / t_la * 1e-6:.1f} incl. full boxes at most); '
              f'buffers: pyramid {pyr.buf.numel() / 2**20:.0f} MiB, alt {alt.nbytes / 2**20:.0f} MiB; max|pyramid - alt| = {err:.2e}', flush=True)
        if args.fp16:
            alt16 = ops.AltCorr(b, 256, h8, w8, device=dev, fp16=True)
            t_prep32, t_prep16 = timed([lambda: alt.build(f1, f2), lambda: alt16.build(f1, f2)], n=N if b * h8 * w8 < 200000 else 5, warm=1)
            out_h = torch.empty(b, 324, h8, w8, device=dev)
            lk_h = alt16.lookup(co, out=out_h, prepare=True)
            t_lp, t_la, t_lh = timed([lk_p, lk_a, lk_h])
            print(f'{W}x{H}, {b} pairs, fp16 features: prepare {t_prep32:.0f} us, prepare16 {t_prep16:.0f} us; lookup per pair: pyramid {t_lp / b:.1f} us, '
                  f'alt f32 {t_la / b:.1f} us, alt fp16 {t_lh / b:.1f} us (alt f32 / alt fp16 = x{t_la / t_lh:.2f}; alt fp16 / pyramid = x{t_lh / t_lp:.1f}); '
                  f'alt fp16 = {useful / t_lh * 1e-6:.1f} TFLOP/s of window products; scratch: alt f32 {alt.nbytes} bytes, alt fp16 {alt16.nbytes} bytes; '
                  f'max|alt f32 - alt fp16| = {float((out_a - out_h).abs().max()):.2e}', flush=True)
            del alt16, out_h, lk_h
        del pyr, alt, out_p, out_a, lk_p, lk_a
        torch.cuda.empty_cache()
    if args.no_forward:
        continue
    for b in (int(v) for v in args.pairs.split(',')):
        peaks = {}
        for flag in (False, True):
            cfg = synth.model_config(H, W, alternate_corr=True, alt_corr_fp16=flag) if args.fp16 else synth.model_config(H, W, alternate_corr=flag)
            net = synth.init_synthetic_weights(raft.RAFT(cfg)).eval().to(dev)
            fr = synth.stereo_frames(3, 1, H, W)
            i1, i2 = fr['image1l'].to(dev).repeat(b, 1, 1, 1), fr['image2l'].to(dev).repeat(b, 1, 1, 1)
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            net(i1, i2)
            torch.cuda.synchronize()
            peaks[flag] = (torch.cuda.max_memory_allocated() - base) / 2**20
            del net, i1, i2
            torch.cuda.empty_cache()
        what = 'alternate_corr with alt_corr_fp16' if args.fp16 else 'alternate_corr'
        print(f'{W}x{H}, {b} pairs: RAFT.forward peak memory above the model and images: {what} off {peaks[False]:.0f} MiB, on {peaks[True]:.0f} MiB', flush=True)
