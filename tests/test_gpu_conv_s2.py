"""GPU: the 96-row tile class of the encoders' stride-2 3x3 layers (rpe_conv_fused_m96, csrc/conv_s2.hip) against the 128-row class of
rpe_conv_fused (bit for bit: outputs and statistics records) and against a float64 convolution on the CPU at the tolerances
tests/test_gpu_conv.py uses for rpe_conv_fused.  Shapes: the smallest at which the class can go wrong -- one tile and a ragged one
(16 x 24 -> 96 pixels, 18 x 20 -> 90), more than one tile per row and per column with a partial last tile (34 x 40 -> 340), batch 2 and 3;
64 -> 96 channels run the new class, 96 -> 128 and every other shape must run exactly as rpe_conv_fused does.

The 1x1 stride-2 shortcut has no second route (it stays on rpe_conv_fused), so there is no new-against-old comparison for it here."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_gpu_conv import _rand, _tol

pytestmark = pytest.mark.gpu

NEW, OLD = 'rpe_conv_fused_m96', 'rpe_conv_fused'
SHAPES = [(64, 96, 16, 24, 2), (64, 96, 18, 20, 2), (64, 96, 34, 40, 2), (64, 96, 34, 40, 3),
          (96, 128, 16, 24, 2), (96, 128, 18, 20, 2), (96, 128, 34, 40, 2)]
_CASES = {}


def _case(cin, cout, h, w, b, stress=False):
    """Inputs, the float64 convolution and both routes' results of one shape, computed once and shared (never modified)."""
    key = (cin, cout, h, w, b, stress)
    if key in _CASES:
        return _CASES[key]
    from rpe_amd import ops
    rng = np.random.default_rng(cin + cout + h + w + b + 7 * stress)
    x, wt, bias = _rand(rng, b, cin, h, w), _rand(rng, cout, cin, 3, 3, s=0.05), _rand(rng, cout, s=0.5)
    if stress:                                                # the instance-norm stress of test_gpu_conv.py: |mean| >> std
        wt[1] *= 1e-3                                         # channel 1: a constant + 1e-3 noise plane
        bias = torch.full((cout,), 50.0) * (1 - 2 * (torch.arange(cout) % 2))       # +-50
    scale, shift = _rand(rng, cout).abs() + 0.5, _rand(rng, cout, s=0.3)
    ho, wo = h // 2, w // 2
    conv = F.conv2d(x.double(), wt.double(), None, stride=2, padding=1)
    pc = ops.PackedConv(wt.cuda(), bias.cuda())
    xg = x.cuda()
    c = dict(x=x, wt=wt, conv=conv, bias=bias, scale=scale, shift=shift, hw=ho * wo)
    for entry in (NEW, OLD):
        bn = ops.conv_fused(xg, pc, ops.CONV_RELU, torch.empty(b, cout, ho, wo, device='cuda'), scale=scale.cuda(), bias=shift.cuda(), stride=2,
                            entry=entry)
        stats = ops.conv_stats_buffer(b, cout, h, w, 'cuda', stride=2)
        raw = ops.conv_fused(xg, pc, ops.CONV_LINEAR, torch.empty(b, cout, ho, wo, device='cuda'), stats=stats, stride=2, entry=entry)
        c[entry] = dict(bn=bn, raw=raw, stats=stats, mi=ops.instnorm_finalize(stats, ho * wo, eps=1e-5, channels=cout))
    _CASES[key] = c
    return c


@pytest.mark.parametrize('cin,cout,h,w,b', SHAPES)
def test_m96_is_bit_identical_to_the_128_row_class(rpe, cin, cout, h, w, b):
    """Both epilogue kinds (folded batch norm + ReLU; raw output + moments).  The new class leaves the same record per 32-pixel block, so
    the records and what rpe_instnorm_finalize makes of them are compared to the bit as well."""
    c = _case(cin, cout, h, w, b)
    n, o = c[NEW], c[OLD]
    assert torch.equal(n['bn'], o['bn']) and torch.equal(n['raw'], o['raw'])
    assert torch.equal(n['stats'], o['stats']) and torch.equal(n['mi'], o['mi'])
    assert float(n['stats'][..., 0].sum(-1).min()) == float(n['stats'][..., 0].sum(-1).max()) == c['hw']


@pytest.mark.parametrize('cin,cout,h,w,b', SHAPES)
@pytest.mark.parametrize('entry', [NEW, OLD])
def test_both_routes_match_f64(rpe, entry, cin, cout, h, w, b):
    """The bars of tests/test_gpu_conv.py::test_stride2_convolutions_match_f64; moments: mean to 1e-6 (of max(|mean|, 1)), 1/std to 2e-5
    relative (NOTES 4.5)."""
    c = _case(cin, cout, h, w, b)
    x, wt, conv = c['x'], c['wt'], c['conv']
    ref = (conv * c['scale'].double()[None, :, None, None] + c['shift'].double()[None, :, None, None]).clamp_min(0)
    assert (c[entry]['bn'].cpu().double() - ref).abs().max() < _tol(x, wt) * 2.5
    pre = conv + c['bias'].double()[None, :, None, None]
    assert (c[entry]['raw'].cpu().double() - pre).abs().max() < _tol(x, wt)
    _check_moments(c[entry]['mi'], pre)


def _check_moments(mi, pre):
    mean, var = pre.mean((2, 3)), pre.var((2, 3), unbiased=False)
    inv_ref = 1.0 / torch.sqrt(var + 1e-5)
    mi = mi.cpu().double()
    em = float(((mi[..., 0] - mean).abs() / mean.abs().clamp_min(1.0)).max())
    ei = float(((mi[..., 1] - inv_ref).abs() / inv_ref).max())
    print(f'moments: mean {em:.2e} (bar 1e-6), 1/std {ei:.2e} relative (bar 2e-5)')
    assert em < 1e-6 and ei < 2e-5


@pytest.mark.parametrize('entry', [NEW, OLD])
def test_moments_survive_large_means(rpe, entry):
    """Conv bias +-50 and a constant + 1e-3 noise plane (std ~ 1e-3 around 50): the pivoted moments of the new class keep their digits."""
    c = _case(64, 96, 34, 40, 2, stress=True)
    pre = c['conv'] + c['bias'].double()[None, :, None, None]
    assert (c[entry]['raw'].cpu().double() - pre).abs().max() < _tol(c['x'], c['wt']) + 50 * 2.0 ** -23          # (+ the rounding of v + bias at |v| ~ 50)
    _check_moments(c[entry]['mi'], pre)
    assert torch.equal(c[NEW]['raw'], c[OLD]['raw']) and torch.equal(c[NEW]['stats'], c[OLD]['stats'])


def test_other_shapes_run_as_rpe_conv_fused(rpe):
    """cout other than 96 (64 here), the 1x1 stride-2 shortcut and a descriptor with a residual take rpe_conv_fused's route under the new
    entry point: same bits, within the float64 bar; an odd map is refused by both (the encoders then use the generic kernel)."""
    from rpe_amd import ops
    rng = np.random.default_rng(5)
    b, h, w = 2, 18, 20
    for cin, cout, k in ((64, 64, 3), (64, 96, 1)):
        x, wt, bias = _rand(rng, b, cin, h, w), _rand(rng, cout, cin, k, k, s=0.05), _rand(rng, cout, s=0.5)
        pc = ops.PackedConv(wt.cuda(), bias.cuda())
        got = [ops.conv_fused(x.cuda(), pc, ops.CONV_LINEAR, torch.empty(b, cout, h // 2, w // 2, device='cuda'), stride=2, entry=e) for e in (NEW, OLD)]
        assert torch.equal(got[0], got[1])
        ref = F.conv2d(x.double(), wt.double(), bias.double(), stride=2, padding=k // 2)
        assert (got[0].cpu().double() - ref).abs().max() < _tol(x, wt)
    x, wt, bias = _rand(rng, b, 64, h, w), _rand(rng, 96, 64, 3, 3, s=0.05), _rand(rng, 96, s=0.5)
    res = _rand(rng, b, 96, h // 2, w // 2)
    pc = ops.PackedConv(wt.cuda(), bias.cuda())
    got = [ops.conv_fused(x.cuda(), pc, ops.CONV_RELU, torch.empty(b, 96, h // 2, w // 2, device='cuda'), residual=res.cuda(), stride=2, entry=e)
           for e in (NEW, OLD)]
    assert torch.equal(got[0], got[1])
    ref = (res.double() + F.conv2d(x.double(), wt.double(), bias.double(), stride=2, padding=1).clamp_min(0)).clamp_min(0)
    assert (got[0].cpu().double() - ref).abs().max() < _tol(x, wt) * 2.5
    for e in (NEW, OLD):
        with pytest.raises(rpe.RpeError):
            ops.conv_fused(torch.zeros(1, 64, 17, 20, device='cuda'), pc, ops.CONV_LINEAR, torch.empty(1, 96, 8, 10, device='cuda'), stride=2, entry=e)


def test_odd_map_keeps_the_generic_route(rpe, monkeypatch):
    """A stride-2 block on an odd map (17 x 24) is not fusable: the switch changes nothing there and the result matches float64."""
    from rpe_amd import raft
    torch.manual_seed(11)
    conv, norm = nn.Conv2d(64, 96, 3, stride=2, padding=1).cuda(), nn.InstanceNorm2d(96)
    x = torch.randn(2, 64, 17, 24, device='cuda')
    monkeypatch.setattr(raft, 'S2_M96_MIN_WGS', 0)
    out = {}
    with torch.no_grad():
        for on in (True, False):
            monkeypatch.setattr(raft, 'S2_M96', on)
            out[on] = raft.conv_norm_act(conv, norm, x, relu=True)
    assert torch.equal(out[True], out[False])
    pre = F.conv2d(x.cpu().double(), conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double(), stride=2, padding=1)
    mean, var = pre.mean((2, 3), keepdim=True), pre.var((2, 3), unbiased=False, keepdim=True)
    inv = float((1 / torch.sqrt(var + 1e-5)).max())
    ref = ((pre - mean) / torch.sqrt(var + 1e-5)).clamp_min(0)
    assert (out[True].cpu().double() - ref).abs().max() < (_tol(x.cpu(), conv.weight.detach().cpu()) + 2e-6) * inv * 2


@pytest.mark.parametrize('norm_fn,dim', [('instance', 256), ('batch', 256)])
def test_encoder_pass_is_unchanged_by_the_switch(rpe, monkeypatch, norm_fn, dim):
    """fnet (instance norm) and cnet (frozen batch norm) on 2 images of 64 x 96, the new class forced for every launch size
    (S2_M96_MIN_WGS = 0) against the switch off.  No moment grouping changed, so the outputs must be equal to the bit; the old route's
    own distance to the CPU oracle on the same input is measured and printed beside it (the bound a change of grouping would be given)."""
    from rpe_amd import raft
    from oracle import raft as oraft
    torch.manual_seed(21)
    enc = raft.BasicEncoder(output_dim=dim, norm_fn=norm_fn).cuda().eval()
    oenc = oraft.BasicEncoder(output_dim=dim, norm_fn=norm_fn).eval()
    oenc.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()})
    img = (255 * torch.rand(2, 3, 64, 96))
    calls = []
    real = raft.ops.conv_fused
    monkeypatch.setattr(raft.ops, 'conv_fused', lambda *a, **k: (calls.append(k.get('entry')), real(*a, **k))[1])
    monkeypatch.setattr(raft, 'S2_M96_MIN_WGS', 0)
    out = {}
    with torch.no_grad():
        for on in (True, False):
            monkeypatch.setattr(raft, 'S2_M96', on)
            calls.clear()
            out[on] = enc(img.cuda(), raw255=True)
            assert (NEW in calls) == on, calls                # the pass really took the route under test
        want = oenc(2 * (img / 255.0) - 1.0)
    d_switch = float((out[True] - out[False]).abs().max())
    d_oracle = float((out[False].cpu() - want).abs().max())
    print(f'{norm_fn}: max |on - off| = {d_switch:.3e}; old route vs CPU oracle = {d_oracle:.3e}; max |out| = {float(want.abs().max()):.3e}')
    assert torch.equal(out[True], out[False])
