"""CPU: the float64 truth of the tail-backward kernels (tests/raft_tail_ref.py) -- its forward pinned to tests/raft_ops_ref.upsample_convex
and F.conv2d, its gradients to finite differences (torch.autograd.gradcheck in float64 at 3x4 with 4 / 8 / 18 channels)."""
import torch
import torch.nn.functional as F

import raft_ops_ref
import raft_tail_ref as ref


def test_forward_is_the_pinned_upsampling_and_conv2d():
    P = {k: v.double() for k, v in ref.make_params(8, 18, seed=3).items()}
    c = ref.make_case(2, 3, 5, 8, seed=3)
    net, prev = c['net'].double(), c['flow_prev'].double()
    up, low, m = ref.tail(net, prev, P)
    t_f = torch.relu(F.conv2d(net, P['fh1_w'], P['fh1_b'], padding=1))
    t_m = torch.relu(F.conv2d(net, P['m0_w'], P['m0_b'], padding=1))
    want_low = prev + F.conv2d(t_f, P['fh2_w'], P['fh2_b'], padding=1)
    want_m = 0.25 * F.conv2d(t_m, P['m2_w'], P['m2_b'])
    assert torch.equal(low, want_low) and torch.equal(m, want_m)
    want = raft_ops_ref.upsample_convex(want_low, want_m)
    assert float((up - want).abs().max()) <= 1e-13 * float(want.abs().max())          # (another order of the nine products)
    # saturated logits: one weight is 1, the others exactly 0 -- no NaN
    sat = 80.0 * torch.sign(torch.randn(1, 576, 3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(0)))
    fl = torch.randn(1, 2, 3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert float((ref.upsample_convex(fl, sat) - raft_ops_ref.upsample_convex(fl, sat)).abs().max()) <= 1e-13 * 8 * float(fl.abs().max())


def test_gradcheck_float64():
    cin, hid = 4, 8
    P = {k: v.double() for k, v in ref.make_params(cin, hid, seed=5).items()}
    c = ref.make_case(1, 3, 4, cin, seed=5)
    assert ref.relu_margin(c['net'], P) > 1e-4                       # finite differences of 1e-6 cross no ReLU kink
    leaves = [c['net'].double().requires_grad_(True), c['flow_prev'].double().requires_grad_(True)] + \
             [P[k].clone().requires_grad_(True) for k in ref.PARAMS]

    def f(net, prev, *ps):
        return ref.tail(net, prev, dict(zip(ref.PARAMS, ps)))[0]
    assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-6, rtol=1e-4)
    # the up-sampling alone, with 18-wide leading maps of logits beside it (9 x 64 channels by definition)
    g = torch.Generator().manual_seed(7)
    fl = torch.randn(1, 2, 3, 4, dtype=torch.float64, generator=g).requires_grad_(True)
    mk = (2.0 * torch.randn(1, 576, 3, 4, dtype=torch.float64, generator=g)).requires_grad_(True)
    assert torch.autograd.gradcheck(ref.upsample_convex, [fl, mk], eps=1e-6, atol=1e-6, rtol=1e-4)
    # d / d delta = d / d flow_low: flow_prev's gradient is the 1/8 flow's
    up, low, m = ref.tail(leaves[0], leaves[1], dict(zip(ref.PARAMS, leaves[2:])))
    gup = c['grad_up'].double()
    g_prev = torch.autograd.grad((up * gup).sum(), leaves[1])[0]
    low2, m2 = low.detach().requires_grad_(True), m.detach()
    g_low = torch.autograd.grad((ref.upsample_convex(low2, m2) * gup).sum(), low2)[0]
    assert torch.equal(g_prev, g_low)
