"""GPU: a route switch flipped on a LIVE model (as the tests and bench.py's A/B runs do) takes the whole pass to the other route: the
model computes, bit for bit, what a model built fresh under the flipped switch computes from the same weights.  (Before every cache key
took raft._switches(), the update block's and the mask head's Winograd packings outlived ``WINOGRAD = False``.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 128, 192          # the smallest image whose fourth pyramid level is 2x3 (64x96 ends in 1x1)

# (what is set before the first pass, what is flipped on the live model)
FLIPS = {'winograd-off': ({}, dict(WINOGRAD=False)),
         'wino-2x4-off': ({}, dict(WINO_2X4=False)),
         'conv-bf16x3': ({}, dict(CONV_BF16X3=True)),
         'conv-bf16x3-gru': ({}, dict(CONV_BF16X3=True, X3_GRU=True)),
         'lookup-fused-off': ({}, dict(LOOKUP_FUSED=False)),
         's2-m96-off': (dict(S2_M96_MIN_WGS=0), dict(S2_M96=False))}      # (MIN_WGS = 0: the 96-row tiles run at this size, so the flip shows)


def _model(raft, state=None):
    torch.manual_seed(1234)
    m = raft.RAFT({'iters': 2})
    if state is not None:
        m.load_state_dict(state)
    m = m.cuda().eval()
    m.freeze_bn()
    return m


@pytest.mark.parametrize('flip', sorted(FLIPS))
def test_a_flipped_switch_on_a_live_model_equals_a_fresh_model(rpe, monkeypatch, flip):
    from rpe_amd import raft
    base, flipped = FLIPS[flip]
    for name, value in base.items():
        monkeypatch.setattr(raft, name, value)
    g = torch.Generator().manual_seed(7)
    im1, im2 = (torch.rand(1, 3, H, W, generator=g).mul(255).cuda() for _ in range(2))
    a = _model(raft)
    state = {k: v.clone() for k, v in a.state_dict().items()}
    flows0, hidden0, _ = a(im1, im2, iters=2)
    assert bool(torch.isfinite(flows0[-1]).all())
    for name, value in flipped.items():
        monkeypatch.setattr(raft, name, value)
    flows_a, hidden_a, _ = a(im1, im2, iters=2)
    flows_b, hidden_b, _ = _model(raft, state)(im1, im2, iters=2)
    print(flip, 'max |flow A - B| =', float((flows_a[-1] - flows_b[-1]).abs().max()), ' max |h A - B| =', float((hidden_a - hidden_b).abs().max()),
          ' max |flow before - after| =', float((flows0[-1] - flows_a[-1]).abs().max()))
    assert torch.equal(flows_a[-1], flows_b[-1]) and torch.equal(hidden_a, hidden_b)
