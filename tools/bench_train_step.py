"""One training step of PoseNet -- forward + loss.backward() -- at the bench geometry, 640x512, n = 1, with the flow network frozen, with
its update block trainable (freeze_flow(False, parts='update')) and with all of it trainable (parts='raft': the node goes through both
encoders), all in one process.  Median of --reps after --warmup, HIP events around each step, peak memory per mode.  Every mode runs under
its own time limit (--limit seconds): a mode that exceeds it ends the process with its traceback, and nothing more is started on the GPU.
Modes the tree does not have are skipped by name (``--modes``), so the same file times an older tree's unchanged modes.
``--optimizer none|torch|hip`` (default none: forward + backward on weights that never move): the parameter update runs INSIDE the timed
step -- ``torch`` = clip_grad_norm_ + torch.optim.AdamW.step, ``hip`` = optim.ClippedAdamW.step (two launches of csrc/optim.hip) -- with the
reference's learning rate, weight decay, epsilon and clip, so the step includes the repacking and re-recording that moved weights cause in
the next forward.  With an optimizer every mode also reports ``opt_ms``: HIP events around the optimizer calls alone.  No threshold
hangs on these numbers; nothing here is tuned.  Prints one JSON line."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, reps, limit):
    faulthandler.dump_traceback_later(limit, exit=True)               # this mode's own time limit
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
        return statistics.median(ts), min(ts), max(ts)
    finally:
        faulthandler.cancel_dump_traceback_later()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--limit', type=float, default=180.0)
    ap.add_argument('--modes', default='frozen,update,raft')
    ap.add_argument('--optimizer', choices=('none', 'torch', 'hip'), default='none')
    a = ap.parse_args()
    import rpe_amd  # noqa: F401
    from rpe_amd import pose_net, synth
    dev = 'cuda'
    model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(a.height, a.width))).to(dev)
    model.train()
    s = {k: v.to(dev) for k, v in synth.stereo_frames(3, 1, a.height, a.width).items()}
    image1r = (0.98 * s['image2r']).contiguous()
    target = torch.tensor([[0.004, -0.003, 0.002, 0.01, -0.008, 0.006]], device=dev)

    hyper = dict(lr=1.0e-5, weight_decay=5.0e-5, eps=1.0e-8)            # configuration/train.yaml of the reference; grad_clip 1.0
    opt, opt_events = None, []
    if a.optimizer == 'torch':
        opt = torch.optim.AdamW(model.parameters(), **hyper)
    elif a.optimizer == 'hip':
        from rpe_amd import optim
        opt = optim.ClippedAdamW(model.parameters(), max_norm=1.0, **hyper)

    def step():
        model.zero_grad(set_to_none=True)
        out = model(s['image1l'], s['image2l'], s['K'], s['baseline'], image1r, s['image2r'], mask1=s['mask1'], mask2=s['mask2'])
        (out[0] - target).abs().sum().backward()
        if opt is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if a.optimizer == 'torch':
                torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.grad is not None], 1.0)
            opt.step()
            e1.record()
            opt_events.append((e0, e1))
    out = dict(height=a.height, width=a.width, iters=model.flow.iters, optimizer=a.optimizer)
    for mode in a.modes.split(','):
        model.freeze_flow(True)
        if mode != 'frozen':
            model.freeze_flow(False, parts=mode)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        opt_events.clear()
        med, lo, hi = timed(step, a.warmup, a.reps, a.limit)
        torch.cuda.synchronize()
        out[mode] = dict(ms=round(med, 2), min_ms=round(lo, 2), max_ms=round(hi, 2), peak_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                         trained=sum(p.requires_grad for p in model.flow.parameters()))
        if opt is not None:
            ts = [e0.elapsed_time(e1) for e0, e1 in opt_events[a.warmup:]]
            out[mode].update(opt_ms=round(statistics.median(ts), 3), opt_min_ms=round(min(ts), 3), opt_max_ms=round(max(ts), 3),
                             stepped=sum(p.grad is not None for p in model.parameters()))
        model.zero_grad(set_to_none=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
