#!/usr/bin/env python3
"""RAFT's ``pad_maps`` (the update loop on zero-padded maps at 1/8 map sizes the tuned kernels refuse) against the generic route, in one
process: per frame pair, flag off and on alternated pass by pass, median of ``--passes`` (default 20) passes after a warm-up, HIP events.
Reported separately: the encoders (both routes run them on the generic kernels at such sizes) and the update loop with the heads
(RAFT.forward on given encoder outputs).  ``--sizes 360x352,1920x1080`` (width x height, defaults), ``--pairs 1``, ``--iters 12``.
Off is the parent route: the same model with raft.PAD_MAPS = False.
``--encoders``: the encoder column instead -- RAFT.encode_both and the whole RAFT.forward under three settings alternated pass by pass (both
switches off = the parent's launches, ``pad_maps`` only, ``pad_maps`` + ``pad_encoders``), with the rpe_conv_direct calls of a pass under each;
e.g. ``--encoders --sizes 360x352,720x576,1920x1080`` and ``--encoders --sizes 360x352 --pairs 16``."""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpe_amd  # noqa: F401
from rpe_amd import _lib, raft, synth

ap = argparse.ArgumentParser()
ap.add_argument('--sizes', default='360x352,1920x1080')
ap.add_argument('--pairs', type=int, default=1)
ap.add_argument('--iters', type=int, default=12)
ap.add_argument('--passes', type=int, default=20)
ap.add_argument('--encoders', action='store_true')
args = ap.parse_args()
dev = torch.device('cuda:0')


def median_ms(fns, n, warm=4):
    """Median milliseconds of each callable, the callables alternated pass by pass."""
    for _ in range(warm):
        for fn in fns:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for _ in fns]
    for i in range(n):
        for k, fn in enumerate(fns):
            a, b = ev[k][i]
            a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) for a, b in e) for e in ev]


def with_flag(flag, fn, encoders=False):
    def run():
        raft.PAD_MAPS, raft.PAD_ENCODERS = flag, encoders
        try:
            return fn()
        finally:
            raft.PAD_MAPS = raft.PAD_ENCODERS = False
    return run


def encoder_table():
    settings = ((False, False), (True, False), (True, True))          # (pad_maps, pad_encoders): parent | loop only | both
    print('| image | 1/8 map -> padded | encode_both off ms | maps ms | maps + encoders ms | off / both | pass off ms | maps ms | maps + encoders ms | maps / both | '
          'conv_direct calls off / maps / both |')
    print('|---|---|---|---|---|---|---|---|---|---|---|')
    for size in args.sizes.split(','):
        W, H = (int(v) for v in size.split('x'))
        net = synth.init_synthetic_weights(raft.RAFT(synth.model_config(H, W, iters=args.iters))).eval().to(dev)
        fr = synth.stereo_frames(5, args.pairs, H, W)
        i1, i2 = fr['image1l'].to(dev), fr['image2l'].to(dev)
        enc = lambda: net.encode_both((i1, i2), i1)
        whole = lambda: net(i1, i2)
        t_enc = median_ms([with_flag(m, enc, e) for m, e in settings], args.passes)
        t_all = median_ms([with_flag(m, whole, e) for m, e in settings], args.passes)
        calls = []
        for m, e in settings:
            with _lib.CountingLib() as c:
                with_flag(m, whole, e)()
            calls.append(sum(n == 'rpe_conv_direct' for n in c.names))
        d = float((with_flag(True, whole, True)()[0][-1] - with_flag(False, whole)()[0][-1]).abs().max())
        print(f'| {W}x{H} x{args.pairs} | {H // 8}x{W // 8} -> {"x".join(map(str, raft.padded_size(H // 8, W // 8)))} | {t_enc[0]:.2f} | {t_enc[1]:.2f} | {t_enc[2]:.2f} | '
              f'{t_enc[0] / t_enc[2]:.2f} | {t_all[0]:.2f} | {t_all[1]:.2f} | {t_all[2]:.2f} | {t_all[1] / t_all[2]:.2f} | {calls[0]} / {calls[1]} / {calls[2]} |   '
              f'(flow both vs off: {d:.1e} px)', flush=True)
        del net
        torch.cuda.empty_cache()


if args.encoders:
    encoder_table()
    sys.exit(0)


print(f'| image | 1/8 map -> padded | encoders ms | loop off ms | loop on ms | loop off/on | pass off ms | pass on ms | pass off/on | loop share off | conv_direct calls off / on |')
print('|---|---|---|---|---|---|---|---|---|---|---|')
for size in args.sizes.split(','):
    W, H = (int(v) for v in size.split('x'))
    net = synth.init_synthetic_weights(raft.RAFT(synth.model_config(H, W, iters=args.iters))).eval().to(dev)
    fr = synth.stereo_frames(5, args.pairs, H, W)
    i1, i2 = fr['image1l'].to(dev), fr['image2l'].to(dev)
    f = net.encode_features((i1, i2))
    fm, cn = (f[:args.pairs], f[args.pairs:]), net.encode_context(i1)
    enc = lambda: (net.encode_features((i1, i2)), net.encode_context(i1))
    loop = lambda: net(None, None, fmaps=fm, cnet=cn)
    whole = lambda: net(i1, i2)
    t_enc, = median_ms([enc], args.passes)
    l_off, l_on = median_ms([with_flag(False, loop), with_flag(True, loop)], args.passes)
    p_off, p_on = median_ms([with_flag(False, whole), with_flag(True, whole)], args.passes)
    calls = []
    for flag in (False, True):
        with _lib.CountingLib() as c:
            with_flag(flag, whole)()
        calls.append(sum(n == 'rpe_conv_direct' for n in c.names))
    d = float((with_flag(True, whole)()[0][-1] - with_flag(False, whole)()[0][-1]).abs().max())
    print(f'| {W}x{H} x{args.pairs} | {H // 8}x{W // 8} -> {"x".join(map(str, raft.padded_size(H // 8, W // 8)))} | {t_enc:.2f} | {l_off:.2f} | {l_on:.2f} | {l_off / l_on:.2f} | '
          f'{p_off:.2f} | {p_on:.2f} | {p_off / p_on:.2f} | {l_off / p_off:.0%} | {calls[0]} / {calls[1]} |   (flow on vs off: {d:.1e} px)', flush=True)
    del net
    torch.cuda.empty_cache()
