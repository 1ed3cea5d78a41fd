"""The reference's training script (scripts/train_posenet.py:23-160) as a module: its loss, its validation pass, one training step and the
loop around them -- on this package's PoseNet, with the parameter update on ``optim.ClippedAdamW`` in place of
``GradScaler.unscale_ / clip_grad_norm_ / scaler.step(AdamW)``.  Host code; where the reference decides something (the order of a step,
when the flow network is released, when it validates and saves, when it stops) this file decides the same.  What it leaves out: wandb and
the TrainLogger (``log`` is any callable that takes the metrics dicts), DataParallel and the dataset readers (``fit`` takes any iterable
of the reference's 9-tuples; ``synth.training_pairs`` makes such tuples with exact ground truth).

A batch is ``(ref_img, trg_img, ref_img_r, trg_img_r, ref_mask, trg_mask, gt_pose, intrinsics, baseline)`` as the reference's datasets
yield it, and reaches the model as the reference hands it over: ``model(trg_img, ref_img, K, baseline, image1r=trg_img_r,
image2r=ref_img_r, mask1=trg_mask, mask2=ref_mask, ret_confmap=True)``."""
import math
import os

import torch

from . import ops
from .optim import ClippedAdamW
from .se3 import SE3

SUM_FREQ = 100
VAL_FREQ = 1000


def supervised_pose_loss(pose_pred, gt):
    """|pose_pred - log(gt)| per component (train_posenet.py:23-26): pose_pred (n,6) tangent, ``gt`` an se3.SE3 or its (n,7) vectors."""
    gt = gt if isinstance(gt, SE3) else SE3(gt)
    if tuple(pose_pred.shape) != (*gt.shape, 6):
        raise ValueError(f'supervised_pose_loss: a prediction of shape {tuple(pose_pred.shape)} for poses of shape {tuple(gt.shape)}')
    return (pose_pred - gt.log()).abs()


def _forward(model, batch):
    """The reference's model call on one batch (train_posenet.py:103-111, 33-41) -> (log-pose (n,6), the SE3 ground truth)."""
    device = next(model.parameters()).device
    ref_img, trg_img, ref_img_r, trg_img_r, ref_mask, trg_mask, gt_pose, intrinsics, baseline = [x.to(device) for x in batch]
    out = model(trg_img, ref_img, intrinsics.float(), baseline.float(), image1r=trg_img_r, image2r=ref_img_r, mask1=trg_mask.to(torch.bool),
                mask2=ref_mask.to(torch.bool), ret_confmap=True)
    return out[0], SE3(gt_pose.float())


def train_step(model, optimizer, batch):
    """One step as the reference takes it: zero_grad, the training forward, the mean of the loss, backward, the clipped update
    (``optimizer.step()``: a ClippedAdamW skips it on the device when a gradient is not finite, as ``scaler.step`` does on the host).
    Returns the per-component loss (n,6), detached, on the device: nothing here reads a value back."""
    optimizer.zero_grad()
    pose, gt = _forward(model, batch)
    loss_pose = supervised_pose_loss(pose, gt)
    torch.mean(loss_pose).backward()
    optimizer.step()
    return loss_pose.detach()


def sequence_loss(flow_preds, flow_gt, valid, gamma=0.8, max_flow=400.0):
    """Upstream RAFT's ``sequence_loss`` (train.py of RAFT: the exponentially weighted L1 distance of every iteration's prediction to the
    ground-truth flow) -> (loss, metrics with 'epe', '1px', '3px', '5px'): ops.flow_sequence_loss under the name its users look for; its
    docstring states the definition and the one departure (a masked pixel contributes exactly zero, NaN or not)."""
    return ops.flow_sequence_loss(flow_preds, flow_gt, valid, gamma=gamma, max_flow=max_flow)


def flow_train_step(raft, optimizer, batch, gamma=0.8, max_flow=400.0, iters=None):
    """One step of training RAFT as RAFT itself is trained, on ground-truth flow: ``batch`` = (image1, image2, flow_gt, valid) -- images
    (b,3,H,W) 0..255, flow_gt (b,2,H,W) f32, valid (b,H,W) or (b,1,H,W) bool -- as synth.flow_pairs yields it.  zero_grad, one
    ``grad_encoders`` + ``grad_all_flows`` pass (every prediction an output of the one node, every parameter reached), the sequence loss,
    backward, ``optimizer.step()`` (a ClippedAdamW skips it on the device when a gradient is not finite).  The batch norms must be frozen
    (RAFT.freeze_bn / eval mode), as upstream freezes them outside its first stage.  Returns the metrics dict with the loss under 'loss',
    detached, on the device: nothing here reads a value back."""
    device = next(raft.parameters()).device
    image1, image2, flow_gt, valid = [x.to(device) for x in batch]
    optimizer.zero_grad()
    flows = raft(image1, image2, iters=iters, all_flows=True, grad_encoders=True, grad_all_flows=True)[0]
    loss, metrics = sequence_loss(flows, flow_gt, valid, gamma=gamma, max_flow=max_flow)
    loss.backward()
    optimizer.step()
    return dict(metrics, loss=loss.detach())


def _metrics(loss_pose, key, mean):
    loss_cpu = loss_pose.detach().cpu()
    return {f'{key}/loss_rot': mean(loss_cpu[:, 3:].sum(dim=-1)).item(), f'{key}/loss_trans': mean(loss_cpu[:, :3].sum(dim=-1)).item(),
            f'{key}/loss_total': mean(loss_cpu.sum(dim=-1)).item()}


def validate(model, loader, log=None, key='val'):
    """The reference's ``val`` (train_posenet.py:29-53): eval mode, no gradients, every batch's three metrics with nanmean -- rotation,
    translation, total -- handed to ``log``; the model goes back to train mode.  Returns (the LAST batch's nanmean loss as a float, as the
    reference does, the metrics averaged over the batches)."""
    model.eval()
    loss, sums, count = float('nan'), {}, 0
    with torch.no_grad():
        for batch in loader:
            pose, gt = _forward(model, batch)
            loss_pose = supervised_pose_loss(pose, gt)
            loss = torch.nanmean(loss_pose).item()
            m = _metrics(loss_pose, key, torch.nanmean)
            if log is not None:
                log(m)
            for k, v in m.items():
                sums[k] = sums.get(k, 0.0) + v
            count += 1
    model.train()
    return loss, {k: v / max(1, count) for k, v in sums.items()}


def checkpoint_paths(outpath, name):
    """(best model, last model, optimizer state beside the last model)."""
    return os.path.join(outpath, f'{name}.pth'), os.path.join(outpath, f'{name}_last.pth'), os.path.join(outpath, f'{name}_last.optim.pth')


def fit(model, train_loader, val_loader, config, outpath, name, log=None, val_freq=VAL_FREQ, resume=None):
    """The reference's training loop (train_posenet.py:72-156).  ``config`` is its YAML as a dict; ``config['train']`` gives
    learning_rate, weight_decay, epsilon, grad_clip, freeze_flow_steps and epochs.

    ``model.train()`` and ``freeze_flow()``; a ClippedAdamW over ALL parameters (the reference hands ``model.parameters()`` to AdamW: a
    frozen parameter has no gradient and is not stepped; once released it joins, because ``step()`` goes by ``.grad``).  At batch index
    ``freeze_flow_steps`` of a pass over the loader the flow network is released -- ``freeze_flow(False, parts='raft')``, this package's
    spelling of the reference's ``freeze_flow(False)``.  Whenever ``total_steps % val_freq == 0`` the model is validated after the update:
    a NaN validation loss ends the run, a new best loss writes ``<name>.pth``, and ``<name>_last.pth`` is written every time, both as
    ``{"state_dict", "config"}`` (what PoseEstimator loads); ``<name>_last.optim.pth`` holds the optimizer's state_dict, the step count and
    the best loss, so that a run can go on from there.  The run ends as the reference's does, when ``total_steps > epochs`` after its
    increment (epochs + 1 steps), the loader being iterated again whenever it runs out.

    ``resume``: the path of such an optimizer file.  The caller has loaded the model (``<name>_last.pth``); the optimizer state, the step
    count and the best loss come from the file, the loader is expected to yield the batches that follow, and the first pass's batch index
    starts at the step count, so a run interrupted after the release resumes released.
    ``log``: a callable; it receives every step's {'train/loss_rot', 'train/loss_trans', 'train/loss_total', 'step'} (which reads the loss
    back, as the reference does per step) and the validation dicts.  Returns {'total_steps', 'best_loss', 'optimizer', 'stopped_on_nan'}."""
    tcfg = config['train']
    model.train()
    model.freeze_flow()
    optimizer = ClippedAdamW(model.parameters(), lr=tcfg['learning_rate'], weight_decay=tcfg['weight_decay'], eps=tcfg['epsilon'],
                             max_norm=tcfg['grad_clip'])
    total_steps, best_loss, first = 0, 1000000.0, 0
    if resume is not None:
        saved = torch.load(resume, map_location='cpu')
        optimizer.load_state_dict(saved['optimizer'])
        total_steps, best_loss = int(saved['total_steps']), float(saved['best_loss'])
        first = total_steps
        if first > tcfg['freeze_flow_steps']:
            model.freeze_flow(False, parts='raft')
    os.makedirs(outpath, exist_ok=True)
    best_path, last_path, optim_path = checkpoint_paths(outpath, name)
    should_keep_training, stopped_on_nan = True, False
    while should_keep_training:
        yielded = False
        for i_batch, batch in enumerate(train_loader, start=first):
            yielded = True
            if i_batch == tcfg['freeze_flow_steps']:
                model.freeze_flow(False, parts='raft')
            loss_pose = train_step(model, optimizer, batch)
            if log is not None:
                log(dict(_metrics(loss_pose, 'train', torch.mean), step=total_steps))
            if total_steps % val_freq == 0:
                val_loss, _ = validate(model, val_loader, log)
                if math.isnan(val_loss):
                    should_keep_training, stopped_on_nan = False, True
                    break
                state = {'state_dict': model.state_dict(), 'config': config}
                if val_loss < best_loss:
                    best_loss = val_loss
                    torch.save(state, best_path)
                torch.save(state, last_path)
                torch.save({'optimizer': optimizer.state_dict(), 'total_steps': total_steps + 1, 'best_loss': best_loss}, optim_path)
            total_steps += 1
            if total_steps > tcfg['epochs']:
                should_keep_training = False
                break
        first = 0
        if not yielded:
            raise ValueError('fit: the training loader yielded no batch')
    return dict(total_steps=total_steps, best_loss=best_loss, optimizer=optimizer, stopped_on_nan=stopped_on_nan)
