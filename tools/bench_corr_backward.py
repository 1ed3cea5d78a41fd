"""Backward of the correlation at the bench geometry: 640x512 (64x80 maps), with --pairs flow pairs in one pass (2 and 16 are the figures
NOTES.md quotes).  Median of --reps after --warmup, HIP events around each call, everything in one process:
  * one ops.corr_lookup_backward (the lookup's adjoint of one iteration into the gradient volume G),
  * one ops.corr_build_backward (the pool, the two GEMMs with their second passes, the pool adjoints),
  * one raft_grad.update_step_backward with and without ``ret_d_corr``,
  * a whole pass and its backward through time with ``grad_update`` (the parent's "backward (tail + 12 steps)") and with ``grad_corr``.
G is S h8 w8 4 bytes per pair (139 MB at 640x512).  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_update_backward import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=2)
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    a = ap.parse_args()
    import rpe_amd  # noqa: F401
    from rpe_amd import ops, raft, raft_grad, synth
    dev = 'cuda'
    b, hh, ww = a.pairs, a.height // 8, a.width // 8
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    T = lambda fn: timed(fn, a.warmup, a.reps)
    out = dict(pairs=b, h8=hh, w8=ww, iters=a.iters)
    vol = ops.corr_grad_volume(b, hh, ww)
    out['grad_volume_mb'] = vol.numel() * 4 / 1e6
    coords = torch.stack((torch.rand(b, hh, ww, generator=g) * ww, torch.rand(b, hh, ww, generator=g) * hh), 1).to(dev)
    d_corr, f1, f2 = r(b, 324, hh, ww), r(b, 256, hh, ww), r(b, 256, hh, ww)
    out['corr_lookup_backward_ms'] = T(lambda: ops.corr_lookup_backward(coords, d_corr, vol))
    out['corr_build_backward_ms'] = T(lambda: ops.corr_build_backward(vol, f1, f2))
    del vol
    model = synth.init_synthetic_weights(raft.RAFT(synth.model_config(a.height, a.width, iters=a.iters))).eval().to(dev)
    upd = model.update_params()
    hx, inp, corr, d_net = r(b, 256, hh, ww), torch.relu(r(b, 128, hh, ww)), r(b, 324, hh, ww), r(b, 128, hh, ww)
    out['update_step_backward_ms'] = T(lambda: raft_grad.update_step_backward(hx, inp, corr, d_net, upd))
    out['update_step_backward_d_corr_ms'] = T(lambda: raft_grad.update_step_backward(hx, inp, corr, d_net, upd, ret_d_corr=True))
    im1, im2 = (255.0 * torch.rand(b, 3, a.height, a.width, generator=g)).to(dev), (255.0 * torch.rand(b, 3, a.height, a.width, generator=g)).to(dev)
    G = r(b, 2, a.height, a.width)
    for p in model.head_params()[0] + model.head_params()[1] + upd:
        p.requires_grad_(True)
    out['forward_ms'] = T(lambda: model(im1, im2))
    for key in ('grad_update', 'grad_corr'):
        out[f'forward_{key}_ms'] = T(lambda: model(im1, im2, **{key: True}))

        def both():
            flows = model(im1, im2, **{key: True})[0]
            (flows[-1] * G).sum().backward()
        out[f'forward_backward_{key}_ms'] = T(both)
        out[f'backward_{key}_ms'] = out[f'forward_backward_{key}_ms'] - out[f'forward_{key}_ms']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
