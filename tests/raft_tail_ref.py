"""A torch restatement of the tail of RAFT's last update iteration, differentiable in any dtype -- the truth of the backward kernels of
csrc/raft_backward.hip (tests/test_gpu_raft_backward.py) when run in float64 on the CPU:

    t_f = relu(conv3x3(net; fh1));  delta = conv3x3(t_f; fh2);  t_m = relu(conv3x3(net; m0));  m = 0.25 * conv1x1(t_m; m2)
    flow_up = upsample_convex(flow_prev + delta, m)

A function of weight TENSORS: channel counts are free (gradcheck runs it with 4 / 8 / 18 channels; the mask head's output is 576 = 9 x 64
by the up-sampling's definition).  Its forward is pinned to tests/raft_ops_ref.upsample_convex and F.conv2d (tests/test_raft_tail_ref_cpu.py)."""
import torch
import torch.nn.functional as F

PARAMS = ('fh1_w', 'fh1_b', 'fh2_w', 'fh2_b', 'm0_w', 'm0_b', 'm2_w', 'm2_b')          # raft_grad.raft_tail_backward's order


def upsample_convex(flow, mask):
    """core/RAFT/core/raft.py RAFT.upsample_flow, in the dtype of its arguments (mask = the logits, the 0.25 already applied)."""
    b, _, hh, ww = flow.shape
    p = torch.softmax(mask.reshape(b, 1, 9, 8, 8, hh, ww), dim=2)
    up = F.unfold(8.0 * flow, (3, 3), padding=1).reshape(b, 2, 9, 1, 1, hh, ww)
    return (p * up).sum(dim=2).permute(0, 1, 4, 2, 5, 3).reshape(b, 2, 8 * hh, 8 * ww)


def pre_activations(net, P):
    """The two pre-ReLU maps (conv3x3(net; fh1), conv3x3(net; m0))."""
    return F.conv2d(net, P['fh1_w'], P['fh1_b'], padding=1), F.conv2d(net, P['m0_w'], P['m0_b'], padding=1)


def tail(net, flow_prev, P):
    """-> (flow_up, flow_low = flow_prev + delta, m)."""
    a_f, a_m = pre_activations(net, P)
    delta = F.conv2d(torch.relu(a_f), P['fh2_w'], P['fh2_b'], padding=1)
    m = 0.25 * F.conv2d(torch.relu(a_m), P['m2_w'], P['m2_b'])
    low = flow_prev + delta
    return upsample_convex(low, m), low, m


def make_params(cin, hid, seed, scale=1.0):
    """Seeded head weights (float32): fh1, m0 (hid,cin,3,3); fh2 (2,hid,3,3); m2 (576,hid,1,1), fan-in scaled."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(fh1_w=r(hid, cin, 3, 3) * scale / (9 * cin) ** 0.5, fh1_b=0.1 * r(hid), fh2_w=r(2, hid, 3, 3) / (9 * hid) ** 0.5, fh2_b=0.1 * r(2),
                m0_w=r(hid, cin, 3, 3) * scale / (9 * cin) ** 0.5, m0_b=0.1 * r(hid), m2_w=4.0 * r(576, hid, 1, 1) / hid ** 0.5, m2_b=0.1 * r(576))


def make_case(b, hh, ww, cin, seed):
    """Seeded net (tanh range), previous 1/8 flow (pixels) and the up-sampled flow's incoming gradient (float32)."""
    g = torch.Generator().manual_seed(seed + 1000)
    return dict(net=torch.tanh(torch.randn(b, cin, hh, ww, generator=g)), flow_prev=3.0 * torch.randn(b, 2, hh, ww, generator=g),
                grad_up=torch.randn(b, 2, 8 * hh, 8 * ww, generator=g))


def tail_grads(case, P, dtype):
    """(d_net, {name: gradient}) of sum(flow_up * grad_up) by autograd in ``dtype`` on the CPU, and the forward's (low, m)."""
    net = case['net'].to(dtype).clone().requires_grad_(True)
    Pd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    up, low, m = tail(net, case['flow_prev'].to(dtype), Pd)
    grads = torch.autograd.grad((up * case['grad_up'].to(dtype)).sum(), [net] + [Pd[k] for k in PARAMS])
    return grads[0], dict(zip(PARAMS, grads[1:])), low.detach(), m.detach()


def relu_margin(net, P):
    """min |pre-activation| / max |pre-activation| over both ReLU layers, in float64: a unit nearer to zero than f32 rounding could be
    decided differently by a float32 kernel and this float64 truth."""
    a_f, a_m = pre_activations(net.double(), {k: v.double() for k, v in P.items()})
    return min(float(a.abs().min() / a.abs().max()) for a in (a_f, a_m))


def ratio(got, truth):
    """max |got - truth| / max |truth| over every element (float64); an all-zero truth admits only zeros: 0.0 then, else inf."""
    got, truth = got.detach().cpu().double(), truth.detach().cpu().double()
    assert got.shape == truth.shape, (got.shape, truth.shape)
    err, scale = float((got - truth).abs().max()), float(truth.abs().max())
    if scale == 0.0:
        return 0.0 if err == 0.0 else float('inf')
    return err / scale
