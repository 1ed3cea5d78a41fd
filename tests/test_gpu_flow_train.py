"""GPU: one step of training RAFT on ground-truth flow (train.flow_train_step): 128 x 128, 3 iterations, two pairs from synth.flow_pairs.
The step against the same step spelled out by hand on a copy of the model (pass, loss, backward, ClippedAdamW) to the bit; a NaN in the
ground truth under a valid pixel skips the step on the device and under an invalid pixel changes nothing; the stepped model's eval
forward is that of a fresh model built from its state_dict (no stale packed weights)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ITERS = 3
HYPER = dict(lr=1e-4, weight_decay=1e-5, eps=1e-8, max_norm=1.0)


def _fresh():
    from rpe_amd import optim, raft, synth
    model = synth.init_synthetic_weights(raft.RAFT(synth.model_config(128, 128, iters=ITERS))).eval().to(DEV)
    for p in model.parameters():
        p.requires_grad_(True)
    return model, optim.ClippedAdamW(model.parameters(), **HYPER)


def _batch():
    from rpe_amd import synth
    return next(iter(synth.flow_pairs(11, 1, 128, 128, batch=2)))


def _weights(model):
    return [p.detach().clone() for p in model.parameters()]


def test_step_equals_the_step_spelled_out(rpe):
    from rpe_amd import ops, optim, raft, synth, train
    batch = _batch()
    model, opt = _fresh()
    twin = copy.deepcopy(model)
    opt2 = optim.ClippedAdamW(twin.parameters(), **HYPER)
    before = _weights(model)
    metrics = train.flow_train_step(model, opt, batch)
    assert set(metrics) >= {'loss', 'epe', '1px', '3px', '5px'} and all(v.is_cuda and not v.requires_grad for v in metrics.values())
    # by hand on the twin
    im1, im2, gt, valid = (x.to(DEV) for x in batch)
    opt2.zero_grad()
    flows = twin(im1, im2, all_flows=True, grad_encoders=True, grad_all_flows=True)[0]
    assert len(flows) == ITERS
    loss, m2 = ops.flow_sequence_loss(flows, gt, valid, gamma=0.8, max_flow=400.0)
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in twin.parameters())
    opt2.step()
    assert int(opt.steps) == 1 == int(opt2.steps) and int(opt.skipped) == 0
    assert torch.equal(metrics['loss'], loss.detach()) and torch.equal(metrics['epe'], m2['epe'])
    changed = 0
    for (name, p), q, b in zip(model.named_parameters(), twin.parameters(), before):
        assert torch.equal(p, q), name
        changed += int(not torch.equal(p.detach(), b))
    assert changed >= 100                                               # (the fnet conv biases have zero gradients: cancelled by the instance norm)
    print(f'flow_train_step: loss {float(loss.detach()):.6f} epe {float(m2["epe"]):.4f} grad norm {float(opt.last_norm):.4f}')
    # the stepped model against a fresh one built from its state_dict
    with torch.no_grad():
        got = model(im1, im2)[0][-1]
        fresh = raft.RAFT(synth.model_config(128, 128, iters=ITERS)).eval()
        fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
        want = fresh.to(DEV)(im1, im2)[0][-1]
    assert torch.equal(got, want)


def test_nan_in_the_ground_truth(rpe):
    from rpe_amd import train
    im1, im2, gt, valid = _batch()
    y, x = (valid[0].nonzero()[0]).tolist()                             # a valid pixel
    yi, xi = ((~valid[0]).nonzero()[0]).tolist()                        # an invalid one
    bad_valid, bad_invalid = gt.clone(), gt.clone()
    bad_valid[0, 0, y, x] = float('nan')
    bad_invalid[0, :, yi, xi] = float('nan')
    clean_model, clean_opt = _fresh()
    clean = train.flow_train_step(clean_model, clean_opt, (im1, im2, gt, valid))
    # under an invalid pixel: nothing changes, to the bit
    model, opt = _fresh()
    got = train.flow_train_step(model, opt, (im1, im2, bad_invalid, valid))
    assert int(opt.skipped) == 0 and int(opt.steps) == 1 and torch.equal(got['loss'], clean['loss'])
    for (name, p), q in zip(model.named_parameters(), clean_model.parameters()):
        assert torch.equal(p, q), name
    # under a valid pixel: the step is skipped on the device and no weight is touched
    model, opt = _fresh()
    before = _weights(model)
    got = train.flow_train_step(model, opt, (im1, im2, bad_valid, valid))
    assert int(opt.skipped) == 1 and int(opt.steps) == 0 and bool(torch.isnan(got['loss']))
    for (name, p), b in zip(model.named_parameters(), before):
        assert torch.equal(p.detach(), b), name
