"""GPU: the backward of RAFT's update block through time (csrc/update_backward.hip, raft_grad.update_step_backward, raft_grad.attach,
RAFT.forward(grad_update=True), PoseNet.freeze_flow(False, parts='update')).  Truth is float64 autograd on the CPU over the restatement
tests/update_block_ref.py.  Bounds as in test_gpu_raft_backward.py: where a result is a plain sum of products, the derived per-element
bound n * 2^-24 * sum |a| |b| (n = terms + partials); elsewhere twice the error of the same restatement run in float32 on the CPU, relative
to max |truth|.  The plumbing is compared bit for bit."""
import pytest
import torch
import torch.nn.functional as F

import update_block_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# -------------------------------------------------------------------------------------------------------------------- weight gradient
def _wgrad(x, dy, kernel, dtype):
    """(dW, db) of y = conv(x; W) + b ('same') by autograd on the CPU."""
    kh, kw = kernel
    w = torch.zeros(dy.shape[1], x.shape[1], kh, kw, dtype=dtype, requires_grad=True)
    bias = torch.zeros(dy.shape[1], dtype=dtype, requires_grad=True)
    y = F.conv2d(x.to(dtype), w, bias, padding=(kh // 2, kw // 2))
    return torch.autograd.grad((y * dy.to(dtype)).sum(), [w, bias])


def _chunks(K):
    chunk = max(1024, (-(-K // 64) + 31) // 32 * 32)                    # include/rpe.h, rpe_conv_bwd_weight
    return -(-K // chunk)


WCASES = [((1, 1, 1), 384, 256, (1, 5)), ((1, 1, 1), 384, 128, (5, 1)),         # all taps but one are padding
          ((2, 3, 4), 384, 256, (1, 5)), ((2, 4, 3), 384, 128, (5, 1)),         # width / height below the tap count
          ((1, 25, 41), 384, 128, (1, 5)),                                      # 1025 pixels: chunk + 1
          ((2, 3, 5), 2, 128, (7, 7)), ((1, 8, 12), 2, 128, (7, 7))]


@pytest.mark.parametrize('shape,cin,cout,kernel', WCASES)
def test_weight_gradient_new_sizes_within_the_derived_bound(rpe, shape, cin, cout, kernel):
    from rpe_amd import ops
    b, hh, ww = shape
    g = _gen(17)
    x, dy = torch.randn(b, cin, hh, ww, generator=g), torch.randn(b, cout, hh, ww, generator=g)
    w64, b64 = _wgrad(x, dy, kernel, torch.float64)
    w32, _ = _wgrad(x, dy, kernel, torch.float32)
    wabs, babs = _wgrad(x.abs(), dy.abs(), kernel, torch.float64)       # sum |dy| |x| over each element's terms
    K = b * hh * ww
    n = K + _chunks(K)
    dw, db = ops.conv_bwd_weight(x.to(DEV), dy.to(DEV), kernel)
    dw2, db2 = ops.conv_bwd_weight(x.to(DEV), dy.to(DEV), kernel)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)                # two runs, the same bits
    ew, eb = (dw.cpu().double() - w64).abs(), (db.cpu().double() - b64).abs()
    e32 = float((w32.double() - w64).abs().max())
    print(f'weight gradient {shape} {cin}->{cout} {kernel}: max err {float(ew.max()):.3e} (bound at that element '
          f'{float((n * U * wabs).flatten()[ew.argmax()]):.3e}); float32 CPU backward {e32:.3e}')
    assert bool((ew <= n * U * wabs).all()), float((ew / (n * U * wabs).clamp_min(1e-300)).max())
    assert bool((eb <= n * U * babs).all())
    dws, dbs = ops.conv_bwd_weight(x.to(DEV), dy.to(DEV), kernel, scale=0.25)
    assert torch.equal(dws, 0.25 * dw) and torch.equal(dbs, 0.25 * db)


@pytest.mark.parametrize('kernel,cin,cout', [((1, 5), 128, 256), ((5, 1), 128, 128), ((7, 7), 2, 128)])
def test_weight_gradient_new_sizes_on_channel_slices(rpe, kernel, cin, cout):
    """x and dy as channel slices of wider buffers (a batch stride beyond the slice): the bits of the dense call."""
    from rpe_amd import ops
    g = _gen(19)
    xb, yb = torch.randn(2, cin + 22, 6, 10, generator=g).to(DEV), torch.randn(2, cout + 44, 6, 10, generator=g).to(DEV)
    x, dy = xb[:, 11:11 + cin], yb[:, 30:30 + cout]
    dense = ops.conv_bwd_weight(x.contiguous(), dy.contiguous(), kernel)
    sliced = ops.conv_bwd_weight(x, dy, kernel)
    assert torch.equal(dense[0], sliced[0]) and torch.equal(dense[1], sliced[1])


# ----------------------------------------------------------------------------------------------------------------------- gate backward
def _gate_case(b, hh, ww, seed, scale=1.0, saturated=False):
    g = _gen(seed)
    t = lambda: torch.randn(b, 128, hh, ww, generator=g)
    pre = {k: (40.0 * torch.sign(t()) if saturated else scale * t()) for k in ('az', 'ar', 'aq')}
    return dict(pre, h=torch.tanh(t()), d=t(), drh=t())


def _gate_truth(c, dtype):
    """One half's elementwise part by autograd: h' = (1 - z) h + z q and rh = r h, seeded with d and drh -> (d az, d aq, d ar, d h)."""
    az, ar, aq, h = (c[k].to(dtype).requires_grad_(True) for k in ('az', 'ar', 'aq', 'h'))
    z, r, q = torch.sigmoid(az), torch.sigmoid(ar), torch.tanh(aq)
    loss = (((1 - z) * h + z * q) * c['d'].to(dtype)).sum() + (r * h * c['drh'].to(dtype)).sum()
    return torch.autograd.grad(loss, [az, aq, ar, h])


def _gate_gpu(c, ops, wide=False):
    """The two kernels on the post-activation values the recompute kernels give; ``wide``: the stacked z | r buffer inside guards."""
    b, _, hh, ww = c['h'].shape
    dev = {k: v.to(DEV) for k, v in c.items()}
    new = lambda ch=128: torch.empty(b, ch, hh, ww, device=DEV)
    z, r, rh, q, hn = new(), new(), new(), new(), new()
    ops.gru_gates_zr_recompute(torch.cat((dev['az'], dev['ar']), 1), dev['h'], z, r, rh)
    ops.gru_gates_h_recompute(dev['aq'], z, dev['h'], q, hn)
    buf = torch.full((b, 256 + 14, hh, ww), 7.0, device=DEV) if wide else new(256)
    dzr = buf[:, 5:261] if wide else buf
    dq, dh = new(), new()
    ops.gru_gates_zq_backward(dev['d'], dev['h'], z, q, dzr[:, :128], dq, dh)
    drh = dev['drh'].clone()
    ops.gru_gates_r_backward(drh, dev['h'], r, dh, dzr[:, 128:], drh)                    # d h in place over d (r h), as the step does
    return (dzr[:, :128], dq, dzr[:, 128:], drh), buf, (z, r, rh, q, hn)


@pytest.mark.parametrize('shape', [(2, 3, 5), (1, 8, 12)])
def test_gate_backward_against_float64(rpe, shape):
    from rpe_amd import ops
    c = _gate_case(*shape, seed=37)
    t64, t32 = _gate_truth(c, torch.float64), _gate_truth(c, torch.float32)
    got, _, fwd = _gate_gpu(c, ops)
    again, _, _ = _gate_gpu(c, ops)
    for name, g, a, w64, w32 in zip(('d_z_pre', 'd_q_pre', 'd_r_pre', 'd_h'), got, again, t64, t32):
        r, r32 = ref.ratio(g, w64), ref.ratio(w32, w64)
        print(f'gate backward {shape} {name}: GPU {r:.3e}  float32 on the CPU {r32:.3e}')
        assert bool(torch.isfinite(g).all()) and r <= 2.0 * r32, (name, r, r32)
        assert torch.equal(g, a), name
    # the recomputed gates themselves: one rounding of the float64 values
    z64, r64, q64 = torch.sigmoid(c['az'].double()), torch.sigmoid(c['ar'].double()), torch.tanh(c['aq'].double())
    for name, g, w in (('z', fwd[0], z64), ('r', fwd[1], r64), ('q', fwd[3], q64), ('rh', fwd[2], r64 * c['h'].double()),
                       ('h_new', fwd[4], (1 - z64) * c['h'].double() + z64 * q64)):
        assert float((g.cpu().double() - w.detach()).abs().max()) <= 3 * U, name


def test_gate_backward_saturated_zero_and_guarded(rpe):
    from rpe_amd import ops
    c = _gate_case(2, 3, 5, seed=41, saturated=True)                    # pre-activations +-40: z, r = 1 or 4e-18, q = +-1 in float32
    t64 = _gate_truth(c, torch.float64)
    got, buf, _ = _gate_gpu(c, ops, wide=True)
    for name, g, w64 in zip(('d_z_pre', 'd_q_pre', 'd_r_pre', 'd_h'), got, t64):
        assert bool(torch.isfinite(g).all()), name
        assert not bool(g.cpu()[w64 == 0].any()), name                  # exact zeros where the truth is zero
        assert float((g.cpu().double() - w64).abs().max()) <= 2 * U * float(w64.abs().max()) + 1e-12, name
    assert not bool(got[1].any())                                       # 1 - q^2 vanishes at q = +-1, in float32 as in float64
    assert bool((buf[:, :5] == 7.0).all()) and bool((buf[:, 261:] == 7.0).all())          # the guards around the stacked z | r buffer
    # no incoming gradient: all zeros
    c0 = dict(_gate_case(2, 3, 5, seed=43), d=torch.zeros(2, 128, 3, 5), drh=torch.zeros(2, 128, 3, 5))
    for g in _gate_gpu(c0, ops)[0]:
        assert not bool(g.any())


# ----------------------------------------------------------------------------------------------------------------------------- one step
# Seeds chosen on the CPU (float64) so that no pre-activation of the motion encoder's five ReLUs lies within 1e-5 of max |pre-activation|
# of zero (about one seed in ten at these sizes): a unit that close could be decided differently by the float32 kernels and the float64
# truth.  The test asserts the condition; it is a condition on the inputs.
STEP_CASES = [((1, 8, 12), 41), ((1, 5, 7), 3)]
BPTT_CASE = ((1, 5, 7), 38, 3)


def _hx(net, flow):
    """The workspace's layout (h | motion slot | flow); the slot holds junk that must not be read."""
    b, _, hh, ww = net.shape
    return torch.cat((net, torch.full((b, 126, hh, ww), 1e30), flow), 1).to(DEV)


def _check(tag, results, w64, w32):
    missed = []
    for name, got in results:
        r, r32 = ref.ratio(got, w64[name]), ref.ratio(w32[name], w64[name])
        print(f'{tag} {name}: GPU {r:.3e}  float32 on the CPU {r32:.3e}')
        if not (bool(torch.isfinite(got).all()) and r <= 2.0 * r32):
            missed.append((name, r, r32))
    assert not missed, missed


def _named(d_net, d_inp, grads):
    return dict(grads, d_net_prev=d_net, d_inp=d_inp)


@pytest.mark.parametrize('shape,seed', STEP_CASES)
def test_one_step_against_float64(rpe, shape, seed):
    """(1,8,12): the tuned route (rpe_conv_fused on groups), (1,5,7): the generic one (rpe_conv_direct) -- all 24 results."""
    from rpe_amd import raft_grad
    P, c = ref.make_params(seed), ref.make_case(*shape, seed)
    assert ref.relu_margin(c, P) > 1e-5
    w64, w32 = _named(*ref.step_grads(c, P, torch.float64)), _named(*ref.step_grads(c, P, torch.float32))
    params = tuple(P[k].to(DEV) for k in ref.PARAMS)
    args = (_hx(c['net'], c['flow'][0]), c['inp'].to(DEV), c['corr'][0].to(DEV), c['d_net'].to(DEV), params)
    d_net, d_inp, grads = raft_grad.update_step_backward(*args)
    again = raft_grad.update_step_backward(*args)
    assert len(grads) == 22 and torch.equal(d_net, again[0]) and torch.equal(d_inp, again[1]) and all(torch.equal(a, b) for a, b in zip(grads, again[2]))
    _check(f'one step {shape}', [('d_net_prev', d_net), ('d_inp', d_inp)] + list(zip(ref.PARAMS, grads)), w64, w32)


# ------------------------------------------------------------------------------------------------------------------------ through time
def test_bptt_against_float64_and_single_step_bits(rpe):
    """The chain the node runs behind the tail -- steps N .. 1 on the entry states, the gradients summed in descending k -- against float64
    autograd through all three steps; the node itself is held to this chain bit for bit by the plumbing tests below.  The entry states
    are the restatement's float64 ones, rounded.  One step of the chain IS the one-step op."""
    from rpe_amd import raft_grad
    shape, seed, steps = BPTT_CASE
    P, c = ref.make_params(seed), ref.make_case(*shape, seed, steps=steps)
    assert ref.relu_margin(c, P) > 1e-5
    w64, w32 = _named(*ref.bptt_grads(c, P, torch.float64)), _named(*ref.bptt_grads(c, P, torch.float32))
    params = tuple(P[k].to(DEV) for k in ref.PARAMS)
    nets = ref.states(c, P)
    states, corr = [_hx(nets[k].float(), c['flow'][k]) for k in range(steps)], [t.to(DEV) for t in c['corr']]
    inp, d = c['inp'].to(DEV), c['d_net'].to(DEV)
    one = raft_grad.update_step_backward(states[-1], inp, corr[-1], d, params)
    total, d_inp = None, None
    for k in reversed(range(steps)):
        d, di, g = raft_grad.update_step_backward(states[k], inp, corr[k], d, params)
        d_inp = di if d_inp is None else d_inp + di
        if k == steps - 1:
            assert torch.equal(d, one[0]) and torch.equal(di, one[1]) and all(torch.equal(a, b) for a, b in zip(g, one[2]))
        total = list(g) if total is None else [a + b for a, b in zip(total, g)]
    _check(f'bptt {shape} x {steps}', [('d_net_prev', d), ('d_inp', d_inp)] + list(zip(ref.PARAMS, total)), w64, w32)


# --------------------------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope='module')
def raft_model(rpe):
    from rpe_amd import raft, synth
    return synth.init_synthetic_weights(raft.RAFT(synth.model_config(128, 160, iters=3))).eval().to(DEV)


def _grad_pass(model, im1, im2, G):
    for p in model.parameters():
        p.grad = None
    flows, hidden, context, low, net0, inp = model(im1, im2, ret_lowres=True, grad_update=True)
    node = flows[-1].grad_fn
    (flows[-1] * G).sum().backward()
    return flows, hidden, context, low, net0, inp, node


@pytest.mark.parametrize('h,w', [(128, 160), (136, 168)])
def test_grad_update_is_the_plain_pass_plus_one_node(rpe, raft_model, h, w):
    """(128,160): 16 x 20 maps, the tuned route; (136,168): 17 x 21 maps, the generic one.  The pass's outputs, the saved states, the
    recomputed window and every gradient bit for bit against the plain passes and the hand chain."""
    from rpe_amd import raft_grad
    g = _gen(31)
    im1, im2 = (255.0 * torch.rand(2, 3, h, w, generator=g)).to(DEV), (255.0 * torch.rand(2, 3, h, w, generator=g)).to(DEV)
    G = torch.randn(2, 2, h, w, generator=g).to(DEV)
    model = raft_model
    fh, mk = model.head_params()
    upd = model.update_params()
    assert len(upd) == 22
    for p in fh + mk + upd:
        p.requires_grad_(True)
    try:
        flows, hidden, context, low, net0, inp, node = _grad_pass(model, im1, im2, G)
        last_corr = model._workspace(2, h // 8, w // 8, im1.device)['corr'].clone()      # the forward's lookup output of iteration 3
        plain = model(im1, im2, ret_lowres=True)
        assert torch.equal(flows[-1], plain[0][-1]) and torch.equal(hidden, plain[1]) and torch.equal(context, plain[2]) and torch.equal(low, plain[3])
        assert all(t.is_leaf and t.requires_grad for t in (hidden, net0, inp)) and torch.equal(inp, plain[2])
        states, corr_of = node.passes[0].states, node.passes[0].corr
        assert len(states) == 3 and all(tuple(s.shape) == (2, 256, h // 8, w // 8) and tuple(co.shape) == (2, 2, h // 8, w // 8) for s, co in states)
        assert torch.equal(net0, states[0][0][:, :128]) and not bool(states[0][0][:, 254:].any())
        for k in (2, 3):                                                # h_{k-1}, flow_k = the results of a (k - 1)-iteration plain pass
            short = model(im1, im2, iters=k - 1, ret_lowres=True)
            assert torch.equal(states[k - 1][0][:, :128], short[1]) and torch.equal(states[k - 1][0][:, 254:], short[3]), k
        assert torch.equal(corr_of(2), last_corr)
        # the hand chain
        d, pg = raft_grad.raft_tail_backward(plain[1], plain[3], G, fh, mk)
        assert torch.equal(hidden.grad, d)
        total, d_inp = None, None
        for k in (2, 1, 0):
            d, di, sg = raft_grad.update_step_backward(states[k][0], plain[2].contiguous(), corr_of(k), d, upd)
            d_inp = di if d_inp is None else d_inp + di
            total = list(sg) if total is None else [a + b for a, b in zip(total, sg)]
        assert torch.equal(net0.grad, d) and torch.equal(inp.grad, d_inp)
        for p, want in zip(fh + mk + upd, list(pg) + total):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0 and torch.equal(p.grad, want)
        assert all(p.grad is None for p in model.parameters() if all(p is not q for q in fh + mk + upd))
        first = [p.grad.clone() for p in fh + mk + upd] + [hidden.grad.clone(), net0.grad.clone(), inp.grad.clone()]
        # a second run: the same bits
        r2 = _grad_pass(model, im1, im2, G)
        second = [p.grad for p in fh + mk + upd] + [r2[1].grad, r2[4].grad, r2[5].grad]
        assert all(torch.equal(a, b) for a, b in zip(first, second))
        # row 0 of the 2-pair pass = the 1-pair pass
        r1 = _grad_pass(model, im1[:1], im2[:1], G[:1])
        for name, a, b in (('hidden', r1[1].grad, first[-3]), ('net_0', r1[4].grad, first[-2]), ('inp', r1[5].grad, first[-1])):
            assert torch.equal(a[0], b[0]), name
    finally:
        for p in model.parameters():
            p.requires_grad_(False)
            p.grad = None


def test_grad_update_refusals_launch_nothing(rpe):
    from rpe_amd import _lib, raft, synth
    img = torch.zeros(1, 3, 128, 160, device=DEV)
    for key in ('update_fp16', 'mixed_precision'):
        model = raft.RAFT(dict(synth.model_config(128, 160), **{key: True})).eval().to(DEV)
        with _lib.CountingLib() as count, pytest.raises(_lib.RpeError, match=key):
            model(img, img, grad_update=True)
        assert count.calls == 0
    model = raft.RAFT(synth.model_config(128, 160)).eval().to(DEV)
    with _lib.CountingLib() as count, pytest.raises(_lib.RpeError, match='upsample'):
        model(img, img, grad_update=True, upsample=False)
    assert count.calls == 0


# ---------------------------------------------------------------------------------------------------------------------------- PoseNet
def _posenet_case():
    from rpe_amd import pose_net, synth
    h, w = 352, 352                                          # the 44 x 44 grid: the smallest the weight heads take
    model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(h, w, iters=3, lbgfs_iters=100))).to(DEV)
    model.train().freeze_flow(True)
    a = {k: v.to(DEV) for k, v in synth.stereo_frames(3, 1, h, w).items()}
    return model, a


def _step(model, a, target, **kw):
    model.zero_grad(set_to_none=True)
    out = model(a['image1l'], a['image2l'], a['K'], a['baseline'], a['image2r'], a['image2r'], mask1=a['mask1'], mask2=a['mask2'],
                ret_confmap=True, **kw)
    (out[0] - target).abs().sum().backward()
    return out, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def test_posenet_trains_the_update_block(rpe):
    """Three iterations per pass (the chain's length does not change what is checked; twelve cost four times the launches)."""
    from rpe_amd import raft_grad
    model, a = _posenet_case()
    target = torch.tensor([[0.004, -0.003, 0.002, 0.01, -0.008, 0.006]], device=DEV)
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):      # (the module route of the weight heads)
        model.freeze_flow(False, parts='heads')
        _, g_heads = _step(model, a, target, ret_flows=True)
        model.freeze_flow(True).freeze_flow(False, parts='update')
        assert model.flow_update_trainable() and model.flow_heads_trainable()
        model.zero_grad(set_to_none=True)
        out = model(a['image1l'], a['image2l'], a['K'], a['baseline'], a['image2r'], a['image2r'], mask1=a['mask1'], mask2=a['mask2'],
                    ret_confmap=True, ret_flows=True)
        node = out[-1]['time_flow'].grad_fn
        lows = [rec.flow_low for rec in node.passes]
        (out[0] - target).abs().sum().backward()
        g_on = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    ub = [(k, p) for k, p in model.named_parameters() if k.startswith('flow.update_block.')]
    assert len(ub) == 30
    for k, p in ub:
        assert k in g_on and bool(torch.isfinite(g_on[k]).all()) and float(g_on[k].abs().max()) > 0.0, k
    assert all(p.grad is None for k, p in model.flow.named_parameters() if not k.startswith('update_block.'))
    heads = model.flow_head_params()
    for k, p in ub:
        if any(p is q for q in heads):
            assert torch.equal(g_on[k], g_heads[k]), k              # the heads' gradients: those of parts='heads', bit for bit
    # the hand chain over (time, stereo1, stereo2) on what the node saved
    flows = out[-1]
    fh, mk = model.flow.head_params()
    upd = model.flow.update_params()
    total = None
    for i, key in enumerate(('time', 'stereo1', 'stereo2')):
        hidden, low, inp = flows['hidden'][key], lows[i], flows['inp'][key]
        gup = flows[('time_flow', 'stereo_flow1', 'stereo_flow2')[i]].grad
        d, pg = raft_grad.raft_tail_backward(hidden.detach(), low, gup.contiguous(), fh, mk)
        states, corr_of = node.passes[i].states, node.passes[i].corr
        assert len(states) == 3
        ug, d_inp = None, None
        for k in (2, 1, 0):
            d, di, sg = raft_grad.update_step_backward(states[k][0], inp.detach(), corr_of(k), d, upd)
            d_inp = di if d_inp is None else d_inp + di
            ug = list(sg) if ug is None else [x + y for x, y in zip(ug, sg)]
        assert torch.equal(flows['net0'][key].grad, d) and torch.equal(inp.grad, d_inp), key
        both = list(pg) + ug
        total = both if total is None else [x + y for x, y in zip(total, both)]
    for p, want in zip(fh + mk + upd, total):
        assert torch.equal(p.grad, want)
    model.freeze_flow(True)
    assert not model.flow_update_trainable() and not model.flow_heads_trainable()
    with pytest.raises(NotImplementedError, match='stop at the flows'):
        model.freeze_flow(False)
