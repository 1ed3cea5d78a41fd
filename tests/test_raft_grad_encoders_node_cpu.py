"""CPU: the plumbing of raft_grad's node at its fourth depth, 'encoders', with the five stage functions, encoder_backward and sum_groups
replaced by small torch fakes that log their calls -- no GPU, no library.  Three passes of batch 1 arranged as PoseNet arranges them: the
time pass and stereo2 are rows of one batched record whose sources are (A | B) -> (B | D) with contexts (A | B), stereo1 is a record of its
own, A -> C with context A, and the node takes them in the order (time, stereo1, stereo2): A -> B, A -> C, B -> D.  Two saved states each,
maps 2 x 3.  Checked: the call log (the depth-'corr' log, then exactly one fnet and one cnet call), the image batches and their order, every
d_out row as the sum of the right leaves' gradients, a pass left out of the loss, a gradient on hidden_out alone and on context_out
alone, an encoder without a trainable parameter, and the refusals of attach."""
import pytest
import torch

N_STEP = 2
U = 2.0 ** -24
N_F, N_C = 3, 5                                                          # the fake encoders' parameter counts
# what the fake build adjoint hands back as d fmap1 / d fmap2 of pass p: float32 values of which every pair that meets in one image's sum
# -- (F1[0], F1[1]) in A, (F2[0], F1[2]) in B -- has a sum that float32 cannot hold exactly, so one rounding is visible
F1 = (1.0, U, 3 * U)
F2 = (1.0 + 2 * U, 5.0, 7.0)


class _Pyr:
    def lookup(self, coords):
        return coords[:, :1].expand(-1, 324, -1, -1)


class _Enc:
    """Stands in for an encoder module: a name and parameters."""

    def __init__(self, name, n):
        self.name, self.params = name, [torch.zeros(j % 3 + 1, requires_grad=True) for j in range(n)]


def _code(t):
    v = int(t.flatten()[0])
    return v // 10, v % 10


@pytest.fixture()
def fakes(rpe, monkeypatch):
    from rpe_amd import raft_grad
    log = []

    def tail(net, flow_low, grad_up, fh, mk):
        p = _code(net)[0]
        log.append(('tail', p))
        return torch.full_like(net, 2.0 ** p), tuple(torch.full_like(w, 2.0 ** (p + j)) for j, w in enumerate(fh + mk))

    def step(hx, inp, corr, d_net, params, ret_d_corr=False):
        p, k = _code(hx)
        assert ret_d_corr and _code(corr) == (p, k)
        log.append(('step', p, k, float(d_net.flatten()[0])))
        return (2.0 * d_net, torch.full_like(inp, 2.0 ** (3 * p + k)), tuple(torch.full_like(w, 2.0 ** (p + j)) for j, w in enumerate(params)),
                torch.full_like(corr, 2.0 ** k))

    def volume(b, h8, w8, levels=4, device='cpu'):
        return torch.zeros(b, h8 * w8, 5, device=device)

    def lookup_adjoint(coords, d_corr, G):
        log.append(('lookup', *_code(coords)))
        return G.add_(d_corr.flatten()[0])

    def build_adjoint(G, fmap1, fmap2, levels=4):
        p = _code(fmap1)[0]
        log.append(('build', p))
        return torch.full_like(fmap1, F1[p]), torch.full_like(fmap2, F2[p])

    def encoder(enc, images, d_out, raw255=True, split_act=False, route=None):
        assert raw255 and split_act == (enc.name == 'cnet') and isinstance(images, list)
        log.append((enc.name, [im for batch in images for im in batch], d_out.clone()))
        return [torch.full_like(w, 2.0 ** j) for j, w in enumerate(enc.params)]

    def sum_groups(parts, bias=None, relu=False, out=None):
        assert bias is None and not relu and out is None and parts.dim() == 5 and parts.is_contiguous() and parts.shape[0] > 1
        acc = parts[0].double()
        for t in parts[1:]:
            acc = acc + t.double()
        return acc.float()
    monkeypatch.setattr(raft_grad, 'raft_tail_backward', tail)
    monkeypatch.setattr(raft_grad, 'update_step_backward', step)
    monkeypatch.setattr(raft_grad.ops, 'corr_grad_volume', volume)
    monkeypatch.setattr(raft_grad.ops, 'corr_lookup_backward', lookup_adjoint)
    monkeypatch.setattr(raft_grad.ops, 'corr_build_backward', build_adjoint)
    monkeypatch.setattr(raft_grad, 'encoder_backward', encoder)
    monkeypatch.setattr(raft_grad, 'sum_groups', sum_groups)
    monkeypatch.setattr(raft_grad, 'encoder_params', lambda enc: list(enc.params))
    return raft_grad, log


def _record(raft_grad, codes, sources):
    """A record of batch len(codes) as RAFT.grad_pass would fill it: row i of every tensor is filled with 10 codes[i] (+ k for step k's states)."""
    rows = 10.0 * torch.tensor(codes, dtype=torch.float32).view(-1, 1, 1, 1)
    fill = lambda ch, k=0, h=2, w=3: (rows + k).expand(len(codes), ch, h, w).contiguous()
    rec = raft_grad.GradPass(fill(2, h=16, w=24), fill(4), fill(2))
    rec.net0, rec.inp, rec.pyr = fill(4), fill(4), _Pyr()
    rec.states = [(fill(8, k), fill(2, k)) for k in range(N_STEP)]
    rec.fmap1, rec.fmap2 = fill(6), fill(6)
    assert rec.depth == 'corr'
    rec.sources = sources
    assert rec.depth == ('corr' if sources is None else 'encoders')
    return rec


def _images():
    """The four distinct images as PoseNet holds them: four batches of one row, each row filled with its own value."""
    return {name: torch.full((1, 3, 16, 24), float(v)) for v, name in enumerate('ABCD')}


def _passes(raft_grad, im):
    """(time, stereo1, stereo2) = A -> B, A -> C, B -> D with contexts A, A, B; time and stereo2 are rows 0 and 1 of one batched record."""
    A, B, C, D = (im[k] for k in 'ABCD')
    batched = _record(raft_grad, (0, 2), (((A, B), 0, 2), ((B, D), 0, 2), ((A, B), 0, 2)))
    stereo1 = _record(raft_grad, (1,), ((A, 0, 1), (C, 0, 1), (A, 0, 1))).rows(0, 1)
    return [batched.rows(0, 1), stereo1, batched.rows(1, 2)]


def _params(n):
    return tuple(torch.zeros(j % 3 + 1, requires_grad=True) for j in range(n))


def _attach(raft_grad, train=('fnet', 'cnet')):
    im = _images()
    passes = _passes(raft_grad, im)
    heads, upd = _params(8), _params(22)
    fnet, cnet = _Enc('fnet', N_F), _Enc('cnet', N_C)
    for enc in (fnet, cnet):
        for w in enc.params:
            w.requires_grad_(enc.name in train)
    outs = raft_grad.attach(passes, (heads[:4], heads[4:]), upd, (fnet, cnet))
    assert len(outs) == 3 and all(len(o) == 3 for o in outs)
    for (flow, hid, ctx), rec in zip(outs, passes):
        assert torch.equal(flow, rec.flow_up) and torch.equal(hid, rec.hidden) and torch.equal(ctx, rec.inp)
        assert flow.requires_grad and hid.requires_grad and ctx.requires_grad and hid.grad_fn is flow.grad_fn and ctx.grad_fn is flow.grad_fn
    assert outs[0][0].grad_fn.passes == passes
    return im, passes, heads, upd, fnet, cnet, outs


def _corr_log(which, d_net=None, tail=None):
    """The depth-'corr' log of the passes ``which``; ``d_net[p]``: the gradient step N of pass p starts from (default: the fake tail's 2^p)."""
    log = []
    for p in which:
        if tail is None or p in tail:
            log.append(('tail', p))
        d = 2.0 ** p if d_net is None else d_net[p]
        for k in reversed(range(N_STEP)):
            log += [('step', p, k, d * 2.0 ** (N_STEP - 1 - k)), ('lookup', p, k)]
        log.append(('build', p))
    return log


def _same(images, want):
    return len(images) == len(want) and all(a.data_ptr() == b[0].data_ptr() and torch.equal(a, b[0]) for a, b in zip(images, want))


def _f64_sum(*terms):
    return float(torch.tensor(sum(float(torch.tensor(t, dtype=torch.float32)) for t in terms), dtype=torch.float64).float())


def _rows(d_out):
    return [float(row.flatten()[0]) for row in d_out]


def test_the_values_show_the_one_rounding():
    for a, b in ((F1[0], F1[1]), (F2[0], F1[2])):
        exact = float(torch.tensor(a, dtype=torch.float32)) + float(torch.tensor(b, dtype=torch.float32))
        assert float(torch.tensor(exact, dtype=torch.float64).float()) != exact          # the sum rounds: a sum taken elsewhere, or twice, shows


def test_shared_images_go_through_each_encoder_once(fakes):
    raft_grad, log = fakes
    im, passes, heads, upd, fnet, cnet, outs = _attach(raft_grad)
    sum(o[0].sum() for o in outs).backward()
    assert log[:-2] == _corr_log((0, 1, 2))
    (name_f, images_f, d_f), (name_c, images_c, d_c) = log[-2:]
    assert (name_f, name_c) == ('fnet', 'cnet')
    assert _same(images_f, [im[k] for k in 'ABCD']) and _same(images_c, [im[k] for k in 'AB'])
    # A: fmap1 of time + fmap1 of stereo1; B: fmap2 of time + fmap1 of stereo2; C: fmap2 of stereo1; D: fmap2 of stereo2
    assert d_f.shape == (4, 6, 2, 3) and all(bool((row == row.flatten()[0]).all()) for row in d_f)
    assert _rows(d_f) == [_f64_sum(F1[0], F1[1]), _f64_sum(F2[0], F1[2]), F2[1], F2[2]]
    # the context: cat(d net0, d inp) of time + stereo1 for A, of stereo2 for B
    net0 = [2.0 ** p * 2.0 ** N_STEP for p in range(3)]
    inp = [sum(2.0 ** (3 * p + k) for k in range(N_STEP)) for p in range(3)]
    assert d_c.shape == (2, 8, 2, 3)
    assert [float(r.flatten()[0]) for r in d_c[:, :4]] == [_f64_sum(net0[0], net0[1]), net0[2]] and bool((d_c[:, :4] == d_c[:, :1]).all())
    assert [float(r.flatten()[0]) for r in d_c[:, 4:]] == [_f64_sum(inp[0], inp[1]), inp[2]] and bool((d_c[:, 4:] == d_c[:, 4:5]).all())
    for p, rec in enumerate(passes):
        assert torch.equal(rec.hidden.grad, torch.full_like(rec.hidden, 2.0 ** p))
        assert torch.equal(rec.net0.grad, torch.full_like(rec.net0, net0[p])) and torch.equal(rec.inp.grad, torch.full_like(rec.inp, inp[p]))
        assert torch.equal(rec.fmap1.grad, torch.full_like(rec.fmap1, F1[p])) and torch.equal(rec.fmap2.grad, torch.full_like(rec.fmap2, F2[p]))
    for j, w in enumerate(heads + upd):
        jj, steps = (j, 1) if j < 8 else (j - 8, N_STEP)                 # (every step of a pass hands back the same value: exact sums)
        assert torch.equal(w.grad, torch.full_like(w, (1.0 + 2.0 + 4.0) * steps * 2.0 ** jj)), j
    for enc in (fnet, cnet):                                             # the gradients leave the node once: .grad is what the fake returned
        for j, w in enumerate(enc.params):
            assert torch.equal(w.grad, torch.full_like(w, 2.0 ** j)), (enc.name, j)


def test_a_pass_left_out_drops_its_contributions_and_its_images(fakes):
    raft_grad, log = fakes
    im, passes, heads, upd, fnet, cnet, outs = _attach(raft_grad)
    (outs[0][0].sum() + outs[2][0].sum()).backward()                    # stereo1 (A -> C) is left out
    assert log[:-2] == _corr_log((0, 2))
    (_, images_f, d_f), (_, images_c, d_c) = log[-2:]
    assert _same(images_f, [im[k] for k in 'ABD']) and _same(images_c, [im[k] for k in 'AB'])
    assert _rows(d_f) == [F1[0], _f64_sum(F2[0], F1[2]), F2[2]]
    assert [float(r.flatten()[0]) for r in d_c[:, :4]] == [4.0, 16.0]
    assert all(t.grad is None for t in passes[1].tensors().values())


def test_hidden_out_alone_runs_the_steps_without_the_tail(fakes):
    raft_grad, log = fakes
    im, passes, heads, upd, fnet, cnet, outs = _attach(raft_grad)
    (3.0 * outs[1][1]).sum().backward()
    assert log[:-2] == _corr_log((1,), d_net={1: 3.0}, tail=())
    (_, images_f, d_f), (_, images_c, d_c) = log[-2:]
    assert _same(images_f, [im[k] for k in 'AC']) and _same(images_c, [im['A']])
    assert torch.equal(passes[1].hidden.grad, torch.full_like(passes[1].hidden, 3.0))
    assert torch.equal(passes[1].net0.grad, torch.full_like(passes[1].net0, 3.0 * 2.0 ** N_STEP))
    assert all(w.grad is None for w in heads) and all(torch.equal(w.grad, torch.full_like(w, N_STEP * 2.0 ** (1 + j))) for j, w in enumerate(upd))
    assert all(t.grad is None for p in (0, 2) for t in passes[p].tensors().values())


def test_hidden_out_is_added_to_the_tails_gradient_once(fakes):
    raft_grad, log = fakes
    im, passes, heads, upd, fnet, cnet, outs = _attach(raft_grad)
    (outs[2][0].sum() + (3.0 * outs[2][1]).sum()).backward()
    assert log[:-2] == _corr_log((2,), d_net={2: 4.0 + 3.0})
    assert torch.equal(passes[2].hidden.grad, torch.full_like(passes[2].hidden, 7.0))


def test_context_out_lands_in_inp_and_in_cnets_gradient(fakes):
    raft_grad, log = fakes
    im, passes, heads, upd, fnet, cnet, outs = _attach(raft_grad)
    (5.0 * outs[2][2]).sum().backward()                                  # alone: nothing of RAFT's own backward runs
    assert [entry[0] for entry in log] == ['cnet']
    _, images_c, d_c = log[0]
    assert _same(images_c, [im['B']]) and bool((d_c[:, :4] == 0).all()) and bool((d_c[:, 4:] == 5.0).all())
    assert torch.equal(passes[2].inp.grad, torch.full_like(passes[2].inp, 5.0)) and passes[2].net0.grad is None and passes[2].hidden.grad is None
    assert all(w.grad is None for w in heads + upd + tuple(fnet.params)) and all(w.grad is not None for w in cnet.params)
    # with the flow: once, behind the steps' sum
    log.clear()
    im, passes, heads, upd, fnet, cnet, outs = _attach(raft_grad)
    (outs[0][0].sum() + (5.0 * outs[0][2]).sum()).backward()
    want = sum(2.0 ** k for k in range(N_STEP)) + 5.0
    assert torch.equal(passes[0].inp.grad, torch.full_like(passes[0].inp, want))
    assert log[-1][0] == 'cnet' and bool((log[-1][2][:, 4:] == want).all())


def test_an_encoder_without_trainable_parameters_is_not_called(fakes):
    raft_grad, log = fakes
    im, passes, heads, upd, fnet, cnet, outs = _attach(raft_grad, train=('fnet',))
    sum(o[0].sum() for o in outs).backward()
    assert log[:-1] == _corr_log((0, 1, 2)) and log[-1][0] == 'fnet'
    assert all(w.grad is None for w in cnet.params) and all(w.grad is not None for w in fnet.params)


def test_encoders_go_with_their_depth_only(fakes):
    raft_grad, log = fakes
    from rpe_amd._lib import RpeError
    im = _images()
    deep = _passes(raft_grad, im)
    heads, upd = _params(8), _params(22)
    fnet, cnet = _Enc('fnet', N_F), _Enc('cnet', N_C)
    corr = _record(raft_grad, (0,), None).rows(0, 1)
    assert corr.depth == 'corr'
    for passes, encoders in ((deep, None), ([corr], (fnet, cnet)), ([deep[0], corr], (fnet, cnet)), ([corr, deep[0]], None)):
        with pytest.raises(RpeError, match='raft_grad.attach'):
            raft_grad.attach(passes, (heads[:4], heads[4:]), upd, encoders)
    assert log == []


def test_rows_narrows_the_sources(fakes):
    raft_grad, _ = fakes
    im = _images()
    A, B, D = im['A'], im['B'], im['D']
    whole = _record(raft_grad, (0, 2), (((A, B), 0, 2), ((B, D), 0, 2), ((A, B), 0, 2)))
    rec = whole.rows(1, 2)
    assert rec.depth == 'encoders' and [s[1:] for s in rec.sources] == [(1, 2)] * 3 and rec.sources[0][0][1] is B
    assert [(t is B or t is D, r) for s in rec.sources for t, r in raft_grad._source_rows(s)] == [(True, 0)] * 3
    assert raft_grad._source_rows(rec.sources[1])[0][0] is D and raft_grad._source_rows(rec.rows(0, 1).sources[0])[0][0] is B
    assert raft_grad.GradPass.TENSORS == ('flow_up', 'hidden', 'flow_low', 'net0', 'inp', 'fmap1', 'fmap2')
    assert raft_grad.GradPass.LEAVES == ('hidden', 'net0', 'inp', 'fmap1', 'fmap2') and raft_grad.STAGES == ('heads', 'update', 'corr', 'encoders')
