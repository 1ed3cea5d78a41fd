"""CPU: tests/update_block_ref.py, the truth of the update block's backward, pinned -- its forward against oracle.raft.BasicUpdateBlock with
the same weights (float64), one of its gradients against central differences, and the properties its callers rely on."""
import operator

import torch

import update_block_ref as ref


def _oracle_block(P):
    from oracle import raft as oracle_raft
    blk = oracle_raft.BasicUpdateBlock().double()
    with torch.no_grad():
        for n, path in ref.ORACLE.items():
            m = operator.attrgetter(path)(blk)
            m.weight.copy_(P[n + '_w'].double())
            m.bias.copy_(P[n + '_b'].double())
    return blk


def test_forward_is_the_oracles_update_block():
    P, c = ref.make_params(3), ref.make_case(2, 5, 7, 3, steps=2)
    blk = _oracle_block(P)
    Pd = {k: v.double() for k, v in P.items()}
    net = want = c['net'].double()
    with torch.no_grad():
        for k in range(2):
            net = ref.step(net, c['inp'].double(), c['corr'][k].double(), c['flow'][k].double(), Pd)
            want = blk(want, c['inp'].double(), c['corr'][k].double(), c['flow'][k].double())[0]
            assert float((net - want).abs().max()) <= 1e-12
    assert torch.equal(ref.states(c, P)[2], net)


def test_a_gradient_against_central_differences():
    P, c = ref.make_params(5), ref.make_case(1, 3, 4, 5, steps=2)
    d_net0, d_inp, g = ref.bptt_grads(c, P, torch.float64)
    Pd = {k: v.double() for k, v in P.items()}

    def loss(Pq, net0=None, inp=None):
        net = c['net'].double() if net0 is None else net0
        for k in range(2):
            net = ref.step(net, c['inp'].double() if inp is None else inp, c['corr'][k].double(), c['flow'][k].double(), Pq)
        return float((net * c['d_net'].double()).sum())
    eps = 1e-6
    for name, idx in (('q1_w', (7, 200, 0, 3)), ('z2_w', (100, 5, 4, 0)), ('c1_w', (30, 300, 0, 0)), ('f1_w', (9, 1, 6, 2)), ('cv_b', (17,))):
        hi, lo = dict(Pd), dict(Pd)
        hi[name], lo[name] = Pd[name].clone(), Pd[name].clone()
        hi[name][idx] += eps
        lo[name][idx] -= eps
        fd = (loss(hi) - loss(lo)) / (2 * eps)
        assert abs(fd - float(g[name][idx])) <= 1e-6 * max(1.0, abs(fd)), (name, fd, float(g[name][idx]))
    for which, grad, idx in (('net', d_net0, (0, 50, 1, 2)), ('inp', d_inp, (0, 90, 2, 0))):
        base = c[which].double()
        hi, lo = base.clone(), base.clone()
        hi[idx] += eps
        lo[idx] -= eps
        kw = (lambda t: dict(net0=t)) if which == 'net' else (lambda t: dict(inp=t))
        fd = (loss(Pd, **kw(hi)) - loss(Pd, **kw(lo))) / (2 * eps)
        assert abs(fd - float(grad[idx])) <= 1e-6 * max(1.0, abs(fd)), which


def test_order_and_margin():
    """PARAMS is raft_grad.UPDATE_PARAMS' order; the margin is that of the five encoder ReLUs and does not depend on the hidden state."""
    assert len(ref.PARAMS) == 22 and ref.PARAMS[:2] == ('z1_w', 'z1_b') and ref.PARAMS[12:14] == ('c1_w', 'c1_b') and ref.PARAMS[-1] == 'cv_b'
    P, c = ref.make_params(1), ref.make_case(1, 3, 4, 1)
    m = ref.relu_margin(c, P)
    assert 0.0 <= m < 1.0
    c2 = dict(c, net=torch.zeros_like(c['net']))
    assert ref.relu_margin(c2, P) == m
    assert ref.ratio(torch.ones(3), torch.ones(3)) == 0.0 and abs(ref.ratio(torch.tensor([1.0, 2.5]), torch.tensor([1.0, 2.0])) - 0.25) < 1e-15
