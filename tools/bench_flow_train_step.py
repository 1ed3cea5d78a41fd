"""One step of training RAFT on ground-truth flow (train.flow_train_step: a grad_encoders + grad_all_flows pass, the sequence loss, backward,
ClippedAdamW) at the bench geometry, 640x512, n = 1, 12 iterations, beside the pose-loss step of PoseNet with all of RAFT trainable
(freeze_flow(False, parts='raft'), forward + loss.backward() + ClippedAdamW) in the same process, the order of the two alternating from
repetition to repetition.  Median of --reps with min and max after --warmup, HIP events around each step; peak memory of each step
measured in a repetition of its own.  Also timed alone: the two launches of the loss's forward and the one of its backward on the pass's
own predictions, and the N - 1 extra tails (raft_tail_backward on the last state, N - 1 times: every tail has the same shapes).  The loss
of the first --losses sequence-loss steps is printed as an observation.  Every phase runs under its own time limit (--limit seconds): a
phase that exceeds it ends the process with its traceback, and nothing more is started on the GPU.  No threshold hangs on these
numbers; the tails are untuned.  Prints one JSON line."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts, digits=2):
    return dict(ms=round(statistics.median(ts), digits), min_ms=round(min(ts), digits), max_ms=round(max(ts), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--losses', type=int, default=6)
    ap.add_argument('--limit', type=float, default=240.0)
    a = ap.parse_args()
    import rpe_amd  # noqa: F401
    from rpe_amd import optim, pose_net, raft, raft_grad, synth, train
    dev = 'cuda'
    hyper = dict(lr=1.0e-5, weight_decay=5.0e-5, eps=1.0e-8, max_norm=1.0)      # configuration/train.yaml of the reference
    # the pose-loss step, tools/bench_train_step.py's
    pose_model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(a.height, a.width, iters=a.iters))).to(dev)
    pose_model.train()
    pose_model.freeze_flow(True).freeze_flow(False, parts='raft')
    pose_opt = optim.ClippedAdamW(pose_model.parameters(), **hyper)
    s = {k: v.to(dev) for k, v in synth.stereo_frames(3, 1, a.height, a.width).items()}
    image1r = (0.98 * s['image2r']).contiguous()
    target = torch.tensor([[0.004, -0.003, 0.002, 0.01, -0.008, 0.006]], device=dev)

    def pose_step():
        pose_model.zero_grad(set_to_none=True)
        out = pose_model(s['image1l'], s['image2l'], s['K'], s['baseline'], image1r, s['image2r'], mask1=s['mask1'], mask2=s['mask2'])
        (out[0] - target).abs().sum().backward()
        pose_opt.step()
    # the sequence-loss step
    flow_model = synth.init_synthetic_weights(raft.RAFT(synth.model_config(a.height, a.width, iters=a.iters))).eval().to(dev)
    flow_opt = optim.ClippedAdamW(flow_model.parameters(), **hyper)
    batch = tuple(x.to(dev) for x in next(iter(synth.flow_pairs(3, 1, a.height, a.width))))
    losses = []

    def seq_step():
        m = train.flow_train_step(flow_model, flow_opt, batch)
        if len(losses) < a.losses:
            losses.append(m['loss'])
    out = dict(height=a.height, width=a.width, iters=a.iters, reps=a.reps)
    faulthandler.dump_traceback_later(a.limit, exit=True)
    for _ in range(a.warmup):
        pose_step()
        seq_step()
    times = {'pose': [], 'sequence': []}
    for i in range(a.reps):
        for name in (('pose', 'sequence') if i % 2 == 0 else ('sequence', 'pose')):
            times[name].append(event_ms(pose_step if name == 'pose' else seq_step))
    for name, fn in (('pose', pose_step), ('sequence', seq_step)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        out[name] = dict(stats(times[name]), peak_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    out['sequence']['first_losses'] = [round(float(x), 5) for x in losses]
    out['sequence']['skipped'] = int(flow_opt.skipped)
    faulthandler.cancel_dump_traceback_later()
    # the loss alone, on the pass's own predictions, and the extra tails alone
    faulthandler.dump_traceback_later(a.limit, exit=True)
    r = flow_model(batch[0], batch[1], all_flows=True, grad_heads=True, grad_all_flows=True)
    preds = [f.detach().requires_grad_(True) for f in r[0]]
    fw, bw = [], []
    for i in range(a.warmup + a.reps):
        box = []
        t = event_ms(lambda: box.append(train.sequence_loss(preds, batch[2], batch[3])[0]))
        tb = event_ms(lambda: box[0].backward())
        if i >= a.warmup:
            fw.append(t)
            bw.append(tb)
    out['loss_forward'], out['loss_backward'] = stats(fw, 3), stats(bw, 3)
    rec = r[0][-1].grad_fn.passes[0]
    fh, mk = flow_model.head_params()
    g = torch.randn_like(preds[-1])

    def tails():
        for _ in range(a.iters - 1):
            raft_grad.raft_tail_backward(rec.hidden.detach(), rec.flow_low, g, fh, mk)
    ts = [event_ms(tails) for _ in range(a.warmup + a.reps)][a.warmup:]
    out['extra_tails'] = dict(stats(ts), count=a.iters - 1)
    faulthandler.cancel_dump_traceback_later()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
