"""CPU: the plumbing of raft_grad's node with a gradient per iteration (``grad_all_flows``: GradPass.earlier), the two stage functions
replaced by small torch fakes that log their calls -- no GPU, no library.  One pass of batch 1 and three iterations at depth 'update' and at
depth 'heads'; every state's first element is its k, so a fake knows which iteration it was handed.  Checked: where the earlier
predictions leave the node, the order of the calls, that a tail's d_net joins the carried gradient in front of the right step, that a
prediction without a gradient costs no tail and the steps above the first gradient are not run, the heads' sum in descending k, the
steps' parameter sum (one f64 sum per parameter and banded weight gradients once an earlier prediction has a gradient, the float32
chain and the plain call otherwise), and that
a gradient on the last prediction alone gives the log and the results of a record without the extra outputs."""
import pytest
import torch

N = 3


@pytest.fixture()
def fakes(rpe, monkeypatch):
    from rpe_amd import raft_grad
    log, banded = [], []
    monkeypatch.setattr(raft_grad, "_test_banded", banded, raising=False)

    def tail(net, flow_low, grad_up, fh, mk):
        k = int(net.flatten()[0])
        assert net.is_contiguous() and flow_low.is_contiguous() and int(flow_low.flatten()[0]) == k and net.shape[1] == 4 and flow_low.shape[1] == 2
        log.append(('tail', k, float(grad_up.flatten()[0])))
        return torch.full_like(net, 2.0 ** k), tuple(torch.full_like(w, 2.0 ** k) for w in fh + mk)

    def step(hx, inp, corr, d_net, params, ret_d_corr=False, wgrad_bands=False):
        k = int(hx.flatten()[0])
        log.append(('step', k, float(d_net.flatten()[0])))
        banded.append(wgrad_bands)
        return d_net + 100.0, torch.full_like(inp, 2.0 ** k), tuple(torch.full_like(w, 2.0 ** k) for w in params)
    monkeypatch.setattr(raft_grad, 'raft_tail_backward', tail)
    monkeypatch.setattr(raft_grad, 'update_step_backward', step)
    def sum_groups(parts, bias=None, relu=False, out=None):                # the steps' parameter sum, once an earlier prediction has a gradient
        assert bias is None and not relu and out is None and parts.dim() == 5 and parts.is_contiguous() and parts.shape[0] > 1
        log.append(('sum', parts.shape[0]))
        return parts.double().sum(0).float()
    monkeypatch.setattr(raft_grad, 'copy_planes', lambda src, dst: dst.copy_(src))
    monkeypatch.setattr(raft_grad, 'sum_groups', sum_groups)
    return raft_grad, log


class _Pyr:
    def lookup(self, coords):
        return coords[:, :1].expand(-1, 324, -1, -1)


def _record(raft_grad, depth, earlier=True):
    fill = lambda ch, v, h=2, w=3: torch.full((1, ch, h, w), float(v))
    rec = raft_grad.GradPass(fill(2, 0, 16, 24), fill(4, N), fill(2, N))
    if depth == 'update':
        rec.net0, rec.inp, rec.pyr = fill(4, 0), fill(4, 0), _Pyr()
        rec.states = [(fill(10, k), fill(2, k)) for k in range(N)]     # (h_k: 4 channels | motion slot | flow_k: the last two)
    elif earlier:
        rec.tail_states = [(fill(4, k), fill(2, k)) for k in range(1, N)]
    if earlier:
        rec.earlier = [fill(2, -k, 16, 24) for k in range(1, N)]
    assert rec.depth == depth
    return rec.rows(0, 1)


def _params(n):
    return tuple(torch.zeros(j % 3 + 1, requires_grad=True) for j in range(n))


def _run(raft_grad, log, depth, weights, earlier=True):
    """loss = sum_k weights[k] sum(prediction k + 1) -> (the log, the record, heads, update parameters)."""
    del log[:]
    rec = _record(raft_grad, depth, earlier)
    heads, upd = _params(8), (_params(22) if depth == 'update' else None)
    if earlier:
        outs, early = raft_grad.attach([rec], (heads[:4], heads[4:]), upd, ret_earlier=True)
        flows = early[0] + [outs[0]]
        assert len(early[0]) == N - 1 and all(f.grad_fn is outs[0].grad_fn for f in flows)
        assert [float(f.detach().flatten()[0]) for f in flows] == [-1.0, -2.0, 0.0]                      # the record's values, in order
    else:
        flows = [None] * (N - 1) + raft_grad.attach([rec], (heads[:4], heads[4:]), upd)
    loss = sum(w * f.sum() for w, f in zip(weights, flows) if w)
    loss.backward()
    return list(log), rec, heads, upd


def test_every_prediction_update(fakes):
    raft_grad, log = fakes
    got, rec, heads, upd = _run(raft_grad, log, 'update', (0.5, 0.25, 1.0))
    # tail N = 3 (d net_3 = 8), step 3; prediction 2's tail (+ 4) in front of step 2; prediction 1's (+ 2) in front of step 1
    assert got == [('tail', 3, 1.0), ('step', 2, 8.0), ('tail', 2, 0.25), ('step', 1, 112.0), ('tail', 1, 0.5), ('step', 0, 214.0)] + [('sum', 3)] * 22
    assert float(rec.net0.grad.flatten()[0]) == 314.0 and float(rec.hidden.grad.flatten()[0]) == 8.0
    assert float(rec.inp.grad.flatten()[0]) == 4.0 + 2.0 + 1.0
    assert all(float(p.grad.flatten()[0]) == 8.0 + 4.0 + 2.0 for p in heads) and all(float(p.grad.flatten()[0]) == 7.0 for p in upd)


def test_first_prediction_only_runs_one_tail_and_one_step(fakes):
    raft_grad, log = fakes
    got, rec, heads, upd = _run(raft_grad, log, 'update', (1.0, 0, 0))
    assert got == [('tail', 1, 1.0), ('step', 0, 2.0)]
    assert float(rec.net0.grad.flatten()[0]) == 102.0 and rec.hidden.grad is None
    assert all(float(p.grad.flatten()[0]) == 2.0 for p in heads) and all(float(p.grad.flatten()[0]) == 1.0 for p in upd)
    got, rec, heads, upd = _run(raft_grad, log, 'update', (0, 1.0, 0))
    assert got == [('tail', 2, 1.0), ('step', 1, 4.0), ('step', 0, 104.0)] + [('sum', 2)] * 22
    assert all(float(p.grad.flatten()[0]) == 3.0 for p in upd)
    assert all(raft_grad._test_banded)                                  # every step so far ran under an earlier prediction's gradient


def test_last_prediction_only_is_the_node_without_the_extra_outputs(fakes):
    raft_grad, log = fakes
    a = _run(raft_grad, log, 'update', (0, 0, 1.0))
    b = _run(raft_grad, log, 'update', (0, 0, 1.0), earlier=False)
    assert a[0] == b[0] == [('tail', 3, 1.0), ('step', 2, 8.0), ('step', 1, 108.0), ('step', 0, 208.0)]
    assert len(raft_grad._test_banded) == 6 and not any(raft_grad._test_banded)          # the steps of before, called as before
    for x, y in zip(a[2] + a[3] + (a[1].net0, a[1].inp, a[1].hidden), b[2] + b[3] + (b[1].net0, b[1].inp, b[1].hidden)):
        assert torch.equal(x.grad, y.grad)


def test_heads_depth_runs_the_tails_alone(fakes):
    raft_grad, log = fakes
    got, rec, heads, _ = _run(raft_grad, log, 'heads', (0.5, 0, 1.0))
    assert got == [('tail', 3, 1.0), ('tail', 1, 0.5)]
    assert all(float(p.grad.flatten()[0]) == 8.0 + 2.0 for p in heads) and float(rec.hidden.grad.flatten()[0]) == 8.0
    got, _, heads, _ = _run(raft_grad, log, 'heads', (1.0, 1.0, 0))
    assert got == [('tail', 2, 1.0), ('tail', 1, 1.0)] and all(float(p.grad.flatten()[0]) == 6.0 for p in heads)


def test_nothing_differentiated_launches_nothing(fakes):
    raft_grad, log = fakes
    rec = _record(raft_grad, 'update')
    heads, upd = _params(8), _params(22)
    outs, early = raft_grad.attach([rec], (heads[:4], heads[4:]), upd, ret_earlier=True)
    other = torch.zeros(1, requires_grad=True)
    (other.sum() + 0 * outs[0].detach().sum()).backward()
    assert log == [] and all(p.grad is None for p in heads + upd)
