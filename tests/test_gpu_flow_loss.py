"""GPU: RAFT's sequence loss and its gradient (csrc/flow_loss.hip through ops.flow_sequence_loss) against float64 on the CPU, on the
kernel's own float32 inputs (sign(pred - gt) of the same float32 inputs is the same in float32 and float64, so the L1 gradient has an
exact truth here).  Shapes: one workgroup with one prediction; an odd map over two rows with three; 6144 pixels -- six workgroups -- with
twelve.  gamma 0.8, max_flow 40.  The inputs hold pixels with pred_k == gt exactly, invalid pixels with NaN and inf in pred and in gt, and
gt magnitudes on both sides of max_flow, none within 1e-3 of it (checked where they are generated).
Bars: loss, per-iteration terms and metrics to a relative 1e-12 (tests/test_gpu_optim.py's bar for its f64 norm: the sums are f64, the
truth's too); the gradient exact 0 where masked or equal, elsewhere within 1 ulp of float32(w_k g / M) with the sign of pred_k - gt."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GAMMA, MAX_FLOW = 0.8, 40.0
CASES = [(1, 8, 8, 1), (2, 17, 23, 3), (1, 64, 96, 12)]
_MADE = {}


def _case(shape):
    """The inputs and their float64 truth, made once per shape and left unchanged."""
    if shape in _MADE:
        return _MADE[shape]
    b, h, w, n = shape
    g = torch.Generator().manual_seed(1000 * h + w + n)
    gt = 30.0 * torch.randn(b, 2, h, w, generator=g)
    mag = gt.double().pow(2).sum(1).sqrt()
    near = (mag - MAX_FLOW).abs() < 1e-2
    gt = torch.where(near[:, None], gt * 1.01, gt)
    valid = torch.rand(b, h, w, generator=g) < 0.7
    preds = [gt + 2.0 * torch.randn(b, 2, h, w, generator=g) * (0.5 + k / n) for k in range(n)]
    for k in range(n):                                                                       # elements with pred_k == gt exactly
        same = torch.rand(b, 2, h, w, generator=g) < 0.1
        preds[k] = torch.where(same, gt, preds[k])
    # a fixed corner: two valid pixels on either side of max_flow, one of them equal in every prediction; four invalid ones with NaN / inf
    valid[0, 0, :6] = torch.tensor([True, True, False, False, False, False])
    gt[0, :, 0, 0], gt[0, :, 0, 1] = torch.tensor([3.0, -4.0]), torch.tensor([39.0, 39.0])
    for p in preds:
        p[0, :, 0, 0] = gt[0, :, 0, 0]
        p[0, :, 0, 1] = torch.tensor([1.0, 1.0])
        p[0, :, 0, 2], p[0, :, 0, 3] = float('nan'), torch.tensor([float('inf'), -float('inf')])
    gt[0, :, 0, 4], gt[0, :, 0, 5] = float('nan'), torch.tensor([float('inf'), 1.0])
    gt[0, 0, 0, 2] = 1.0
    preds[-1][0, :, 0, 5] = float('nan')
    # the conditions on the inputs, checked here on the CPU
    mag = gt.double().pow(2).sum(1).sqrt()
    fin = torch.isfinite(mag)
    assert not bool(((mag - MAX_FLOW).abs() < 1e-3)[fin].any())
    assert bool((valid & fin & (mag < MAX_FLOW)).any()) and bool((valid & fin & (mag > MAX_FLOW)).any())
    assert bool(torch.isfinite(gt[valid[:, None].expand_as(gt)]).all())                      # NaN / inf in gt lie under invalid pixels only
    assert all(bool(torch.isfinite(p[valid[:, None].expand_as(p)]).all()) for p in preds)
    assert any(bool(torch.isnan(p[~valid[:, None].expand_as(p)]).any()) for p in preds) and bool(torch.isnan(gt).any()) and bool(torch.isinf(gt).any())
    # float64 truth, written with torch.where
    mask = valid & (mag < MAX_FLOW)
    M = float(gt.numel())
    m2 = mask[:, None].expand_as(gt)
    zero = torch.zeros((), dtype=torch.float64)
    weights = [GAMMA ** (n - 1 - k) for k in range(n)]
    terms = [float(torch.where(m2, (p.double() - gt.double()).abs(), zero).sum()) / M for p in preds]
    assert all(bool((m2 & (p == gt)).any()) and bool((m2 & (p != gt)).any()) for p in preds)
    epe = torch.where(mask, (preds[-1].double() - gt.double()).pow(2).sum(1).sqrt(), zero)
    count = int(mask.sum())
    truth = dict(mask=mask, M=M, weights=weights, terms=terms, loss=sum(wk * t for wk, t in zip(weights, terms)), count=count,
                 epe=float(epe.sum()) / count, **{f'{r}px': float((mask & (epe < r)).sum()) / count for r in (1, 3, 5)},
                 signs=[torch.where(m2, torch.sign(p.double() - gt.double()), zero) for p in preds])
    _MADE[shape] = (preds, gt, valid, truth)
    return _MADE[shape]


def _run(preds, gt, valid, scale=None):
    from rpe_amd import ops
    leaves = [p.to(DEV).requires_grad_(True) for p in preds]
    loss, metrics = ops.flow_sequence_loss(leaves, gt.to(DEV), valid.to(DEV), gamma=GAMMA, max_flow=MAX_FLOW)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.grad_fn is not None and not any(v.requires_grad for v in metrics.values())
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), metrics, [p.grad for p in leaves]


def _rel(got, want):
    return abs(float(got) - want) / max(abs(want), 1e-300)


@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_loss_metrics_and_gradient_against_float64(rpe, shape):
    preds, gt, valid, T = _case(shape)
    n = shape[3]
    for scale in (None, 0.37):
        loss, metrics, grads = _run(preds, gt, valid, scale)
        again = _run(preds, gt, valid, scale)
        got_terms = metrics['terms'].cpu()
        errs = dict(loss=_rel(metrics['loss_f64'], T['loss']), epe=_rel(metrics['epe'], T['epe']),
                    terms=max(_rel(got_terms[k], T['terms'][k]) for k in range(n)), **{f'{r}px': _rel(metrics[f'{r}px'], T[f'{r}px']) for r in (1, 3, 5)})
        print(f'flow loss {shape} g = {scale or 1}: loss {float(metrics["loss_f64"]):.12g}  relative errors ' + '  '.join(f'{k} {v:.2e}' for k, v in errs.items()))
        assert all(v <= 1e-12 for v in errs.values()), errs
        assert int(metrics['count']) == T['count'] and got_terms.shape == (n,)
        assert float(loss) == float(np.float32(float(metrics['loss_f64'])))                     # the f32 loss is the f64 one rounded once
        g32 = float(np.float32(1.0 if scale is None else scale))
        for k in range(n):
            got = grads[k].cpu()
            sign = T['signs'][k]
            c = np.float32(T['weights'][k] * g32 / T['M'])
            assert bool((got[sign == 0] == 0).all()), k                                          # masked or equal: exact zero (and no NaN)
            live = sign != 0
            assert bool((torch.sign(got[live]).double() == sign[live]).all()), k
            off = (got[live].abs().double() - float(c)).abs().max()
            assert float(off) <= float(np.spacing(c)), (k, float(off), float(c))
        # two runs, the same bits
        assert torch.equal(loss, again[0]) and all(torch.equal(a, b) for a, b in zip(grads, again[2]))
        assert all(torch.equal(metrics[key].view(torch.int64) if metrics[key].dtype == torch.float64 else metrics[key],
                               again[1][key].view(torch.int64) if metrics[key].dtype == torch.float64 else again[1][key]) for key in metrics)


def test_a_mask_with_no_pixel_set(rpe):
    preds, gt, valid, _ = _case(CASES[1])
    for v in (torch.zeros_like(valid), valid & (gt.double().pow(2).sum(1).sqrt() >= MAX_FLOW)):      # nothing valid; nothing below max_flow
        loss, metrics, grads = _run(preds, gt, v)
        assert float(loss) == 0.0 and float(metrics['loss_f64']) == 0.0 and int(metrics['count']) == 0 and not bool(metrics['terms'].any())
        assert all(not bool(g.any()) and bool(torch.isfinite(g).all()) for g in grads)
        assert all(bool(torch.isnan(metrics[k])) for k in ('epe', '1px', '3px', '5px'))


def test_rows_are_independent_of_their_batch(rpe):
    """M doubles with the batch, so row 0's gradient in a batch of two is half its gradient alone: a power of two, equal to the bit."""
    preds, gt, valid, _ = _case(CASES[1])
    _, _, both = _run(preds, gt, valid)
    _, _, alone = _run([p[:1].contiguous() for p in preds], gt[:1].contiguous(), valid[:1].contiguous())
    for k, (a, b2) in enumerate(zip(alone, both)):
        assert bool(a.any()) and torch.equal(a, 2.0 * b2[:1]), k


def test_valid_forms_and_the_upstream_name(rpe):
    from rpe_amd import train
    preds, gt, valid, T = _case(CASES[1])
    dev = [p.to(DEV) for p in preds]
    ref = train.sequence_loss(dev, gt.to(DEV), valid.to(DEV), gamma=GAMMA, max_flow=MAX_FLOW)
    assert _rel(ref[1]['loss_f64'], T['loss']) <= 1e-12
    for v in (valid[:, None], valid.to(torch.uint8), (2 * valid.to(torch.uint8))[:, None]):
        got = train.sequence_loss(dev, gt.to(DEV), v.to(DEV), gamma=GAMMA, max_flow=MAX_FLOW)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1]['terms'], ref[1]['terms'])
