"""CPU: the plumbing of raft_grad's one autograd node (attach / _RaftGradFn / GradPass) with the five stage functions replaced by small
torch fakes that log their calls -- no GPU, no library.  Three passes of batch 1 (rows of one record of batch 3), two saved states each,
maps 2 x 3, at each of the three depths: the order of the calls, the skipped pass, every leaf's .grad, the order of the parameter sums
(float32 values whose sum has other bits in any other order), the refusal of mixed depths, and GradPass.rows."""
import pytest
import torch

N_PASS, N_STEP = 3, 2
U = 2.0 ** -24
# the fakes' parameter gradients: value[pass] of the tail, value[pass][k] of step k, times 2^j for parameter j (a power of two scales
# every rounding alike).  Chosen so that the node's order -- steps in descending k, then passes in the given order -- is the only one
# of the four orders below with these bits (the tests assert that of the values themselves)
HEAD = (1.0, U, U)
STEP = ((1.0, 1.0), (U, 2 * U), (U, U))                                  # STEP[p][k]


class _Pyr:
    """Stands in for the pass's pyramid: the 'window' at some coordinates is their first plane, 324 times."""

    def __init__(self):
        self.lookups = 0

    def lookup(self, coords):
        self.lookups += 1
        return coords[:, :1].expand(-1, 324, -1, -1)


def _code(t):
    """(pass, k) a fake's input was filled with."""
    v = int(t.flatten()[0])
    return v // 10, v % 10


@pytest.fixture()
def fakes(rpe, monkeypatch):
    """raft_grad with its five stage functions replaced -> (raft_grad, the call log)."""
    from rpe_amd import raft_grad
    log = []

    def tail(net, flow_low, grad_up, fh, mk):
        p = _code(net)[0]
        assert _code(flow_low)[0] == p and not net.requires_grad and len(fh) == len(mk) == 4
        log.append(('tail', p))
        return torch.full_like(net, 2.0 ** p), tuple(torch.full_like(w, HEAD[p] * 2.0 ** j) for j, w in enumerate(fh + mk))

    def step(hx, inp, corr, d_net, params, ret_d_corr=False):
        p, k = _code(hx)
        assert _code(corr) == (p, k) and corr.shape[:2] == (1, 324) and _code(inp)[0] == p and len(params) == 22
        log.append(('step', p, k, float(d_net.flatten()[0])))
        out = (2.0 * d_net, torch.full_like(inp, 2.0 ** (3 * p + k)), tuple(torch.full_like(w, STEP[p][k] * 2.0 ** j) for j, w in enumerate(params)))
        return out + (torch.full_like(corr, 2.0 ** k),) if ret_d_corr else out

    def volume(b, h8, w8, levels=4, device='cpu'):
        return torch.zeros(b, h8 * w8, 5, device=device)

    def lookup_adjoint(coords, d_corr, G):
        log.append(('lookup', *_code(coords)))
        return G.add_(d_corr.flatten()[0])

    def build_adjoint(G, fmap1, fmap2, levels=4):
        p = _code(fmap1)[0]
        assert _code(fmap2)[0] == p and levels == 4 and not fmap1.requires_grad
        log.append(('build', p))
        return torch.full_like(fmap1, float(G.flatten()[0]) * 2.0 ** p), torch.full_like(fmap2, -float(G.flatten()[0]) * 2.0 ** p)
    monkeypatch.setattr(raft_grad, 'raft_tail_backward', tail)
    monkeypatch.setattr(raft_grad, 'update_step_backward', step)
    monkeypatch.setattr(raft_grad.ops, 'corr_grad_volume', volume)
    monkeypatch.setattr(raft_grad.ops, 'corr_lookup_backward', lookup_adjoint)
    monkeypatch.setattr(raft_grad.ops, 'corr_build_backward', build_adjoint)
    return raft_grad, log


def _whole(raft_grad, depth):
    """One record of batch 3 as RAFT.grad_pass would fill it: row p of every tensor is filled with 10 p (+ k for the states of step k)."""
    rows = 10.0 * torch.arange(N_PASS).view(N_PASS, 1, 1, 1)
    fill = lambda ch, k=0, h=2, w=3: (rows + k).expand(N_PASS, ch, h, w).contiguous()
    rec = raft_grad.GradPass(fill(2, h=16, w=24), fill(4), fill(2))
    if depth != 'heads':
        rec.net0, rec.inp, rec.pyr = fill(4), fill(4), _Pyr()
        rec.states = [(fill(8, k), fill(2, k)) for k in range(N_STEP)]
    if depth == 'corr':
        rec.fmap1, rec.fmap2 = fill(6), fill(6)
    assert rec.depth == depth
    return rec


def _params(n):
    return tuple(torch.zeros(j % 3 + 1, requires_grad=True) for j in range(n))


def _attach(raft_grad, depth):
    whole = _whole(raft_grad, depth)
    passes = [whole.rows(p, p + 1) for p in range(N_PASS)]
    heads, upd = _params(8), None if depth == 'heads' else _params(22)
    flows = raft_grad.attach(passes, (heads[:4], heads[4:]), upd)
    assert len(flows) == N_PASS and all(torch.equal(f, p.flow_up) and f.requires_grad for f, p in zip(flows, passes))
    assert flows[0].grad_fn.passes == passes
    return whole, passes, heads, upd or (), flows


def _want_log(depth, which):
    log = []
    for p in which:
        log.append(('tail', p))
        for k in reversed(range(N_STEP)) if depth != 'heads' else ():
            log.append(('step', p, k, 2.0 ** p * 2.0 ** (N_STEP - 1 - k)))       # the tail's d net_N, doubled by every step behind it
            if depth == 'corr':
                log.append(('lookup', p, k))
        if depth == 'corr':
            log.append(('build', p))
    return log


def _f32_sum(terms):
    """((t0 + t1) + t2) + ... in float32."""
    acc = torch.tensor(terms[0], dtype=torch.float32)
    for t in terms[1:]:
        acc = acc + torch.tensor(t, dtype=torch.float32)
    return acc


def _update_sum(which):
    """The node's order: per pass the steps in descending k, then the passes in the given order."""
    return _f32_sum([float(_f32_sum([STEP[p][k] for k in reversed(range(N_STEP))])) for p in which])


def test_the_values_tell_the_orders_apart():
    every = list(range(N_PASS))
    assert not torch.equal(_f32_sum([HEAD[p] for p in every]), _f32_sum([HEAD[p] for p in reversed(every)]))
    node = _update_sum(every)
    flat = _f32_sum([STEP[p][k] for p in every for k in reversed(range(N_STEP))])                                   # one running sum
    steps_first = _f32_sum([float(_f32_sum([STEP[p][k] for p in every])) for k in reversed(range(N_STEP))])         # passes inside, steps outside
    assert not any(torch.equal(node, other) for other in (_update_sum(list(reversed(every))), flat, steps_first))


@pytest.mark.parametrize('skip', [None, 1])
@pytest.mark.parametrize('depth', ['heads', 'update', 'corr'])
def test_calls_leaves_and_parameter_sums(fakes, depth, skip):
    """``skip``: that pass's flow is left out of the loss -- it adds nothing to the log or to a sum and gets None everywhere."""
    raft_grad, log = fakes
    whole, passes, heads, upd, flows = _attach(raft_grad, depth)
    which = [p for p in range(N_PASS) if p != skip]
    sum(flows[p].sum() for p in which).backward()
    assert log == _want_log(depth, which)
    for p, rec in enumerate(passes):
        assert rec.flow_up.grad is None and rec.flow_low.grad is None
        if p == skip:
            assert all(t.grad is None for t in rec.tensors().values())
            continue
        assert torch.equal(rec.hidden.grad, torch.full_like(rec.hidden, 2.0 ** p))
        if depth != 'heads':
            assert torch.equal(rec.net0.grad, torch.full_like(rec.net0, 2.0 ** p * 2.0 ** N_STEP))
            assert torch.equal(rec.inp.grad, torch.full_like(rec.inp, sum(2.0 ** (3 * p + k) for k in range(N_STEP))))
        if depth == 'corr':
            g = sum(2.0 ** k for k in range(N_STEP)) * 2.0 ** p          # both lookup adjoints went into the volume the build's read
            assert torch.equal(rec.fmap1.grad, torch.full_like(rec.fmap1, g)) and torch.equal(rec.fmap2.grad, torch.full_like(rec.fmap2, -g))
    if depth != 'heads':
        assert whole.pyr.lookups == N_STEP * len(which)                  # one lookup per step of a pass that ran, none for a skipped one
    for j, w in enumerate(heads):
        assert torch.equal(w.grad, torch.full_like(w, float(_f32_sum([HEAD[p] for p in which])) * 2.0 ** j)), j
    for j, w in enumerate(upd):
        assert torch.equal(w.grad, torch.full_like(w, float(_update_sum(which)) * 2.0 ** j)), j


def test_mixed_depths_are_refused(fakes):
    raft_grad, log = fakes
    from rpe_amd._lib import RpeError
    shallow, deep = _whole(raft_grad, 'heads').rows(0, 1), _whole(raft_grad, 'update').rows(0, 1)
    heads, upd = _params(8), _params(22)
    for passes, update_params in (([shallow, deep], upd), ([deep, shallow], upd), ([deep, _whole(raft_grad, 'corr').rows(0, 1)], upd),
                                  ([shallow], upd), ([deep], None)):
        with pytest.raises(RpeError, match='raft_grad.attach'):
            raft_grad.attach(passes, (heads[:4], heads[4:]), update_params)
    assert log == []


def test_rows_makes_fresh_leaves_and_slices_every_state(fakes):
    raft_grad, _ = fakes
    whole = _whole(raft_grad, 'corr')
    rec = whole.rows(1, 3)
    assert rec.depth == 'corr' and rec.pyr is whole.pyr
    for name in raft_grad.GradPass.TENSORS:
        assert torch.equal(getattr(rec, name), getattr(whole, name)[1:3]), name
    assert rec.hidden.is_leaf and rec.hidden.requires_grad and rec.hidden.data_ptr() == whole.hidden[1:3].data_ptr()      # detached, not copied
    for name in ('net0', 'inp', 'fmap1', 'fmap2'):
        t = getattr(rec, name)
        assert t.is_leaf and t.requires_grad and t.is_contiguous() and t.data_ptr() != getattr(whole, name)[1:3].data_ptr(), name
    assert not any(t.requires_grad for t in whole.tensors().values()) and not rec.flow_up.requires_grad and not rec.flow_low.requires_grad
    assert len(rec.states) == N_STEP
    for (hx, co), (whx, wco) in zip(rec.states, whole.states):
        assert torch.equal(hx, whx[1:3]) and torch.equal(co, wco[1:3])
    # the window: looked up once per k against the whole pass's pyramid at the whole pass's coordinates, these rows of it
    for k in (1, 1, 0):
        assert torch.equal(rec.corr(k), whole.pyr.lookup(whole.states[k][1])[1:3])
    assert whole.pyr.lookups == 2 + 3
    inner = rec.rows(1, 2)                                               # rows of rows: row 2 of the whole pass
    assert torch.equal(inner.hidden, whole.hidden[2:3]) and torch.equal(inner.corr(0), whole.pyr.lookup(whole.states[0][1])[2:3])
    shallow = _whole(raft_grad, 'heads').rows(0, 1)
    assert shallow.depth == 'heads' and shallow.states is None and shallow.net0 is None and shallow.fmap1 is None and list(shallow.tensors()) == ['flow_up', 'hidden', 'flow_low']
