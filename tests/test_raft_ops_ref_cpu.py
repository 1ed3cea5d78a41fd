"""CPU: the float64 restatements of tests/raft_ops_ref.py against torch's own operators in float64, so that the truth the GPU tests of
tests/test_gpu_raft_ops_edges.py compare with cannot drift along with the kernels."""
import pytest
import torch
import torch.nn.functional as F

import raft_ops_ref as ref
from oracle import raft as oraft


def rel(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('b,c,h,w', [(2, 7, 5, 6), (1, 3, 1, 4), (1, 4, 2, 1), (3, 1, 1, 1), (1, 9, 4, 12)])
def test_conv3x3_to2_is_conv2d_with_zero_padding(b, c, h, w):
    g = torch.Generator().manual_seed(b * 100 + c)
    x = torch.randn(b, c, h, w, generator=g)
    wt, bias, add = torch.randn(2, c, 3, 3, generator=g), torch.randn(2, generator=g), torch.randn(b, 2, h, w, generator=g) * 10
    want = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
    assert rel(ref.conv3x3_to2(x, wt, bias), want) <= 1e-12
    assert rel(ref.conv3x3_to2(x, wt, None, add), want - bias.double()[None, :, None, None] + add.double()) <= 1e-12
    assert ref.conv3x3_to2(x, wt, bias).dtype == torch.float64
    co, fl = ref.flow_update(x, wt, bias, add)
    assert rel(co, want + add.double()) <= 1e-12
    assert torch.equal(fl, co - oraft.coords_grid(b, h, w).double())


def test_conv3x3_to2_nonfinite_reaches_what_conv2d_says():
    g = torch.Generator().manual_seed(1)
    b, c, h, w = 2, 5, 6, 8
    x = torch.randn(b, c, h, w, generator=g)
    wt, bias = torch.randn(2, c, 3, 3, generator=g), torch.randn(2, generator=g)
    for (y, xx) in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        x[0, 1, y, xx] = float('inf')
    x[1, 2, 3, 4] = float('nan')
    x[1, 0, 2, w - 1] = float('-inf')
    got = ref.conv3x3_to2(x, wt, bias)
    want = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and torch.equal(torch.sign(got[torch.isinf(got)]), torch.sign(want[torch.isinf(want)]))
    fin = torch.isfinite(want)
    assert float((got[fin] - want[fin]).abs().max()) <= 1e-12 * float(want[fin].abs().max())
    bad = ~torch.isfinite(got[0, 0])                                         # a corner Inf: exactly its in-map 2x2 neighbourhood
    expect = torch.zeros(h, w, dtype=torch.bool)
    expect[:2, :2] = expect[:2, -2:] = expect[-2:, :2] = expect[-2:, -2:] = True
    assert torch.equal(bad, expect)
    assert int(torch.isnan(got[1, 0]).sum()) == 9                            # the NaN: its 3x3 neighbourhood


@pytest.mark.parametrize('b,h8,w8', [(1, 1, 1), (2, 5, 7), (1, 1, 6), (1, 6, 1)])
def test_upsample_convex_is_the_oracles(b, h8, w8):
    g = torch.Generator().manual_seed(h8 * 10 + w8)
    flow, mask = torch.randn(b, 2, h8, w8, generator=g) * 4, torch.randn(b, 576, h8, w8, generator=g) * 2
    want = oraft.upsample_flow(flow.double(), mask.double())
    got = ref.upsample_convex(flow, mask)
    assert got.dtype == torch.float64 and rel(got, want) <= 1e-12
    mask[0, 5 * 64 + 9] = float('-inf')
    mask[0, 3::64][:, 0, 0] = float('-inf')                                  # all nine of sub-pixel 3 of cell (0, 0)
    mask[b - 1, 2 * 64 + 17, h8 - 1, w8 - 1] = float('inf')
    flow[0, 0, 0, 0] = float('inf')
    flow[b - 1, 1, h8 - 1, w8 - 1] = float('nan')
    want = oraft.upsample_flow(flow.double(), mask.double())
    got = ref.upsample_convex(flow, mask)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
    fin = torch.isfinite(want)
    assert not bool(fin.any()) or float((got[fin] - want[fin]).abs().max()) <= 1e-12 * max(1.0, float(want[fin].abs().max()))
    eq = ref.upsample_convex(flow := torch.randn(1, 2, 3, 3, generator=g), torch.full((1, 576, 3, 3), 0.7))
    mean = F.avg_pool2d(8 * flow.double(), 3, stride=1, padding=1)           # nine equal logits: the mean of the zero-padded window
    assert float((eq[:, :, ::8, ::8] - mean).abs().max()) <= 1e-12


@pytest.mark.parametrize('relu', (False, True))
@pytest.mark.parametrize('with_res', (False, True))
def test_norm_epilogues_are_torchs(relu, with_res):
    g = torch.Generator().manual_seed(3)
    x, bias, res = torch.randn(2, 5, 6, 7, generator=g) * 3 + 1, torch.randn(5, generator=g), torch.randn(2, 5, 6, 7, generator=g)
    pre = x.double() + bias.double()[None, :, None, None]
    want = F.instance_norm(pre, eps=1e-5)
    bn = torch.nn.BatchNorm2d(5).double().eval()
    bn.running_mean.normal_(generator=g); bn.running_var.uniform_(0.5, 2.0, generator=g)
    bn.weight.data.normal_(generator=g); bn.bias.data.normal_(generator=g)
    with torch.no_grad():
        wantb = bn(pre)
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        shift = (bias.double() - bn.running_mean) * scale + bn.bias
    if relu:
        want, wantb = torch.relu(want), torch.relu(wantb)
    if with_res:
        want, wantb = torch.relu(res.double() + want), torch.relu(res.double() + wantb)
    r = res if with_res else None
    assert rel(ref.instnorm_act(x, bias, 1e-5, relu, r), want) <= 1e-12
    assert rel(ref.affine_act(x, scale, shift, relu, r), wantb) <= 1e-12
    one = ref.instnorm_act(torch.full((1, 2, 1, 1), 3.0), None, 1e-5, False, None)      # hw = 1: variance 0, the result 0
    assert float(one.abs().max()) == 0.0
    assert bool(torch.isnan(ref.bias_act(torch.tensor([[[[float('nan'), -1.0, 2.0]]]]), torch.tensor([0.5]), True))[0, 0, 0, 0])
    assert ref.bias_act(torch.tensor([[[[float('nan'), -1.0, 2.0]]]]), torch.tensor([0.5]), True)[0, 0, 0, 1:].tolist() == [0.0, 2.5]


def test_gates_are_sigmoid_and_tanh():
    g = torch.Generator().manual_seed(4)
    b, c, h, w = 2, 3, 4, 5
    zr, add, bias = torch.randn(b, 2 * c, h, w, generator=g) * 3, torch.randn(b, 2 * c, h, w, generator=g), torch.randn(2 * c, generator=g)
    hx = torch.randn(b, c + 2, h, w, generator=g)
    zr[0, 0, 0, :4] = torch.tensor([float('inf'), float('-inf'), 1e4, -1e4])
    z, rh = ref.gates_zr(zr, bias, add, hx, c)
    pre = zr.double() + add.double() + bias.double()[None, :, None, None]
    assert rel(z, torch.sigmoid(pre[:, :c])) <= 1e-12 and rel(rh, torch.sigmoid(pre[:, c:]) * hx.double()[:, :c]) <= 1e-12
    assert z[0, 0, 0, :4].tolist() == [1.0, 0.0, 1.0, 0.0]
    q, bq = torch.randn(b, c, h, w, generator=g) * 3, torch.randn(c, generator=g)
    hn = ref.gates_h(z.float(), q, bq, None, hx)
    zf = z.float().double()
    want = (1 - zf) * hx.double()[:, :c] + zf * torch.tanh(q.double() + bq.double()[None, :, None, None])
    assert rel(hn, want) <= 1e-12 and hn.dtype == torch.float64
