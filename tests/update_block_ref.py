"""Test infrastructure: float64 / float32 CPU restatement of ONE application of RAFT's update block without its heads, and of N of them
through time, with ``flow`` and ``corr`` as constants (upstream detaches coords1 at the top of every iteration) -- the truth
raft_grad.update_step_backward and the node through time are held to.  Pinned to oracle.raft.BasicUpdateBlock by tests/test_update_block_ref_cpu.py."""
import torch
import torch.nn.functional as F

# (name, cout, cin, kh, kw) in raft_grad.UPDATE_PARAMS' order: 12 tensors of the SepConvGRU, 10 of the motion encoder
LAYERS = (('z1', 128, 384, 1, 5), ('r1', 128, 384, 1, 5), ('q1', 128, 384, 1, 5), ('z2', 128, 384, 5, 1), ('r2', 128, 384, 5, 1),
          ('q2', 128, 384, 5, 1), ('c1', 256, 324, 1, 1), ('c2', 192, 256, 3, 3), ('f1', 128, 2, 7, 7), ('f2', 64, 128, 3, 3), ('cv', 126, 256, 3, 3))
PARAMS = tuple(f'{n}_{t}' for n, *_ in LAYERS for t in ('w', 'b'))
ORACLE = dict(z1='gru.convz1', r1='gru.convr1', q1='gru.convq1', z2='gru.convz2', r2='gru.convr2', q2='gru.convq2', c1='encoder.convc1',
              c2='encoder.convc2', f1='encoder.convf1', f2='encoder.convf2', cv='encoder.conv')
RELUS = ('c1', 'c2', 'f1', 'f2', 'cv')


def make_params(seed):
    """The 22 tensors, float32, at the scale of a default-initialised layer (uniform +-1/sqrt(fan_in))."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for n, cout, cin, kh, kw in LAYERS:
        s = (cin * kh * kw) ** -0.5
        P[n + '_w'] = (2 * torch.rand(cout, cin, kh, kw, generator=g) - 1) * s
        P[n + '_b'] = (2 * torch.rand(cout, generator=g) - 1) * s
    return P


def make_case(b, h, w, seed, steps=1):
    """Inputs of ``steps`` applications: net_0 (tanh-ranged), inp (ReLU-ranged), per step a flow and a looked-up window, and d net_N."""
    g = torch.Generator().manual_seed(seed + 1000)
    return dict(net=torch.tanh(torch.randn(b, 128, h, w, generator=g)), inp=torch.relu(torch.randn(b, 128, h, w, generator=g)),
                flow=[2.0 * torch.randn(b, 2, h, w, generator=g) for _ in range(steps)],
                corr=[2.0 * torch.randn(b, 324, h, w, generator=g) for _ in range(steps)], d_net=torch.randn(b, 128, h, w, generator=g))


def _conv(x, P, n):
    w = P[n + '_w']
    return F.conv2d(x, w, P[n + '_b'], padding=(w.shape[2] // 2, w.shape[3] // 2))


def encoder_pre(flow, corr, P):
    """The five pre-activations in front of the motion encoder's ReLUs, by name."""
    pre = {'c1': _conv(corr, P, 'c1')}
    pre['c2'] = _conv(torch.relu(pre['c1']), P, 'c2')
    pre['f1'] = _conv(flow, P, 'f1')
    pre['f2'] = _conv(torch.relu(pre['f1']), P, 'f2')
    pre['cv'] = _conv(torch.cat((torch.relu(pre['c2']), torch.relu(pre['f2'])), 1), P, 'cv')
    return pre


def step(net, inp, corr, flow, P):
    """net_k of BasicUpdateBlock.forward(net, inp, corr, flow) (core/RAFT/core/update.py), restated."""
    x = torch.cat((inp, torch.relu(encoder_pre(flow, corr, P)['cv']), flow), 1)
    for hf in ('1', '2'):
        hx = torch.cat((net, x), 1)
        z, r = torch.sigmoid(_conv(hx, P, 'z' + hf)), torch.sigmoid(_conv(hx, P, 'r' + hf))
        q = torch.tanh(_conv(torch.cat((r * net, x), 1), P, 'q' + hf))
        net = (1 - z) * net + z * q
    return net


def bptt_grads(case, P, dtype, steps=None):
    """(d net_0, d inp, {name: gradient}) of sum(net_N * d_net) after ``steps`` applications, by autograd in ``dtype``."""
    steps = len(case['flow']) if steps is None else steps
    Pd = {k: v.to(dtype).requires_grad_(True) for k, v in P.items()}
    net0, inp = case['net'].to(dtype).requires_grad_(True), case['inp'].to(dtype).requires_grad_(True)
    net = net0
    for k in range(steps):
        net = step(net, inp, case['corr'][k].to(dtype), case['flow'][k].to(dtype), Pd)
    g = torch.autograd.grad((net * case['d_net'].to(dtype)).sum(), [net0, inp] + [Pd[k] for k in PARAMS])
    return g[0], g[1], dict(zip(PARAMS, g[2:]))


def step_grads(case, P, dtype):
    return bptt_grads(case, P, dtype, steps=1)


def states(case, P, dtype=torch.float64):
    """[net_0, net_1, ...]: the entry states of the steps."""
    Pd = {k: v.to(dtype) for k, v in P.items()}
    out = [case['net'].to(dtype)]
    for k in range(len(case['flow'])):
        out.append(step(out[-1], case['inp'].to(dtype), case['corr'][k].to(dtype), case['flow'][k].to(dtype), Pd))
    return out


def ratio(got, want):
    """max |got - want| / max |want|."""
    want = want.double()
    return float((got.detach().cpu().double() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def relu_margin(case, P):
    """min over the five encoder ReLUs and all steps of  min |pre-activation| / max |pre-activation|  (float64)."""
    Pd = {k: v.double() for k, v in P.items()}
    m = 1.0
    for k in range(len(case['flow'])):
        for pre in encoder_pre(case['flow'][k].double(), case['corr'][k].double(), Pd).values():
            m = min(m, float(pre.abs().min() / pre.abs().max()))
    return m
