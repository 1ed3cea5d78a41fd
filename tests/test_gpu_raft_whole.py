"""GPU: whole-network training -- raft_grad's depth 'encoders' through RAFT.forward(grad_encoders=True) and PoseNet
(freeze_flow(False, parts='raft')).  128 x 128 pairs (the smallest the four-level pyramid takes), 2 iterations; PoseNet at 352 x 352 (the
smallest grid the weight heads take).  Truth for the two new paths (hidden_out, context_out) and the shared images: float64 autograd on the
CPU through the whole model (tests/raft_whole_ref.py); the bar is the project's -- an error relative to max |truth| of at most twice that of
the same autograd in float32 on the CPU.  ReLU decisions are discrete: SEED is the first from 53 on for which the float32 and the float64
CPU references decide every ReLU input alike (searched on the CPU with raft_whole_ref.forward_states; asserted below on the states the GPU
pass saved: a condition on the inputs)."""
import pytest
import torch

import raft_whole_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED = 53


def _model(seed):
    from rpe_amd import raft, synth
    model = synth.init_synthetic_weights(raft.RAFT(synth.model_config(128, 128, iters=2))).eval()
    case = ref.make_case(model, seed)
    model = model.to(DEV)
    for p in model.parameters():
        p.requires_grad_(True)
    return model, case


def _params(model):
    """The 124: fnet's 32, cnet's 62, the eight heads', the 22 of the update block -- raft_whole_ref.whole_truth's order."""
    from rpe_amd import raft_grad
    fh, mk = model.head_params()
    params = raft_grad.encoder_params(model.fnet) + raft_grad.encoder_params(model.cnet) + list(fh + mk + model.update_params())
    assert len(params) == 124 and len({id(p) for p in params}) == 124 == len(list(model.parameters()))
    return params


def test_one_call_equals_two_calls(rpe):
    model, case = _model(SEED)
    im1, im2, gup = case['images'][0].to(DEV), case['images'][1].to(DEV), case['g_up'][:1].to(DEV)
    params = _params(model)

    def run(whole):
        for p in params:
            p.grad = None
        r = model(im1, im2, ret_lowres=True, **(dict(grad_encoders=True) if whole else dict(grad_corr=True)))
        rec = r[0][-1].grad_fn.passes[0]
        (r[0][-1] * gup).sum().backward()
        if not whole:
            assert all(p.grad is None for p in params[:94])
            model.backward_encoders(im1, im2, r[6], r[7], r[4], r[5])
        leaves = [rec.hidden, r[4], r[5], r[6], r[7]]
        assert all(t.is_leaf for t in leaves) and leaves[1] is rec.net0 and leaves[4] is rec.fmap2
        return r, [p.grad.clone() for p in params], [t.grad.clone() for t in leaves]
    ra, pa, la = run(True)
    rb, pb, lb = run(False)
    assert ra[1].grad_fn is ra[0][-1].grad_fn and ra[2].grad_fn is ra[0][-1].grad_fn and rb[1].is_leaf      # hidden_out, context_out: the node's
    assert torch.equal(ra[0][-1], rb[0][-1]) and all(torch.equal(a, b) for a, b in zip(ra[1:], rb[1:]))
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a, b), i
    for i, (a, b) in enumerate(zip(la, lb)):
        assert torch.equal(a, b), i


def _two_passes(model, case):
    """Rows of ONE batched pass over three images encoded once, PoseNet.stages' own arrangement: A -> B and B -> C with contexts A, B."""
    from rpe_amd import raft_grad
    A, B, C = (im.to(DEV) for im in case['images'])
    for p in model.parameters():
        p.grad = None
    with torch.no_grad():
        f = model.encode_features([A, B, C])
        cn = model.encode_context([A, B])
        _, whole = model.grad_pass((f[:2], f[1:]), cn, stages='encoders', upsample=True,
                                   sources=(((A, B, C), 0, 2), ((A, B, C), 1, 3), ((A, B), 0, 2)))
    passes = [whole.rows(0, 1), whole.rows(1, 2)]
    outs = raft_grad.attach(passes, model.head_params(), model.update_params(), (model.fnet, model.cnet))
    g_up, g_hid, g_ctx = (case[k].to(DEV) for k in ('g_up', 'g_hid', 'g_ctx'))
    loss = sum((flow * g_up[i:i + 1]).sum() + (hid * g_hid[i:i + 1]).sum() + (ctx * g_ctx[i:i + 1]).sum() for i, (flow, hid, ctx) in enumerate(outs))
    loss.backward()
    return whole, [p.grad.clone() for p in _params(model)]


def test_both_new_paths_and_shared_images_against_float64(rpe, monkeypatch):
    """All 124 parameters against float64 through the whole model, loss on the flow, hidden_out and context_out of both passes; two runs,
    the same bits.  (One MI355X run: 0.08 to 1.94 of float32 on the CPU, the worst cnet's layer2[1].conv2.weight.)"""
    from rpe_amd import raft_grad
    model, case = _model(SEED)
    calls = []
    inner = raft_grad.encoder_backward
    monkeypatch.setattr(raft_grad, 'encoder_backward', lambda enc, images, *a, **kw: (calls.append(sum(im.shape[0] for im in images)), inner(enc, images, *a, **kw))[1])
    whole, got = _two_passes(model, case)
    assert calls == [3, 2]                                              # B is shared: each encoder once, on the distinct images
    _, again = _two_passes(model, case)
    coords, flows = [co.cpu() for _, co in whole.states], [st[:, 254:].cpu() for st, _ in whole.states]
    args = (model, case['images'], (0, 1), (1, 2), (0, 1), coords, flows, case['g_up'], case['g_hid'], case['g_ctx'])
    w64, s64, net64 = ref.whole_truth(*args, torch.float64)
    w32, s32, net32 = ref.whole_truth(*args, torch.float32)
    print(f'whole forward: net_N of the pass {ref.ratio(whole.hidden, net64):.3e}  float32 on the CPU {ref.ratio(net32, net64):.3e}')
    same, differ = ref.same_relu_decisions(s32, s64)
    assert same, f'seed {SEED}: float32 and float64 decide {differ} ReLU inputs differently'
    names = [f'fnet.p{i}' for i in range(32)] + [f'cnet.p{i}' for i in range(62)] + [f'heads.p{i}' for i in range(8)] + [f'update.p{i}' for i in range(22)]
    fnet_conv_bias = {f'fnet.p{i}' for i in range(1, 30, 2)}            # cancelled by the instance norm: exact zeros
    missed, worst = [], (0.0, None)
    for name, g, a, t64, t32 in zip(names, got, again, w64, w32):
        assert torch.equal(g, a), name                                  # two runs, the same bits
        assert bool(torch.isfinite(g).all()), name
        if name in fnet_conv_bias:
            assert not bool(g.any()) and float(t64.abs().max()) < 1e-9, name
            continue
        assert float(g.abs().max()) > 0, name
        r, r32 = ref.ratio(g, t64), ref.ratio(t32, t64)
        worst = max(worst, (r / max(r32, 1e-300), name))
        print(f'whole {name}: GPU {r:.3e}  float32 on the CPU {r32:.3e}  ratio {r / max(r32, 1e-300):.2f}')
        if not r <= 2.0 * r32:
            missed.append((name, r, r32))
    print(f'whole: worst ratio {worst[0]:.2f} ({worst[1]})')
    assert not missed, missed


# ---------------------------------------------------------------------------------------------------------------------------- PoseNet
def _posenet(train_heads_hip):
    from rpe_amd import pose_net, synth
    h, w = 352, 352
    # (three iterations and the solver's 100, as test_posenet_trains_the_update_block: with two the synthetic weights' stereo flow leaves
    # too few valid depths, the layer's linear system is singular and its backward returns zeros for the whole batch)
    cfg = dict(synth.model_config(h, w, iters=3, lbgfs_iters=100), train_heads_hip=train_heads_hip)
    model = synth.init_synthetic_weights(pose_net.PoseNet(cfg)).to(DEV)
    model.train().freeze_flow(True)
    a = {k: v.to(DEV) for k, v in synth.stereo_frames(3, 1, h, w).items()}
    a['image1r'] = (0.98 * a['image2r']).contiguous()                  # a fourth image of its own: identity, not content, tells images apart
    return model, a


def _step(model, a, target):
    model.zero_grad(set_to_none=True)
    out = model(a['image1l'], a['image2l'], a['K'], a['baseline'], a['image1r'], a['image2r'], mask1=a['mask1'], mask2=a['mask2'],
                ret_confmap=True, ret_flows=True)
    (out[0] - target).abs().sum().backward()
    return out, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('train_heads_hip', [False, True])
def test_posenet_trains_raft_whole(rpe, monkeypatch, train_heads_hip):
    from rpe_amd import raft_grad
    model, a = _posenet(train_heads_hip)
    target = torch.tensor([[0.004, -0.003, 0.002, 0.01, -0.008, 0.006]], device=DEV)
    calls = []
    inner = raft_grad.encoder_backward
    monkeypatch.setattr(raft_grad, 'encoder_backward', lambda enc, images, *x, **kw: (calls.append((enc, sum(im.shape[0] for im in images))), inner(enc, images, *x, **kw))[1])
    own = lambda grads: {k: g for k, g in grads.items() if not k.startswith('flow.')}
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):      # (the module route of the weight heads)
        frozen, g_frozen = _step(model, a, target)
        model.freeze_flow(False, parts='update')
        upd, _ = _step(model, a, target)
        inp_update = upd[-1]['inp']['time'].grad.clone()
        assert calls == []
        model.freeze_flow(True).freeze_flow(False, parts='raft')
        out, g_on = _step(model, a, target)
        assert calls == [(model.flow.fnet, 4), (model.flow.cnet, 2)]
        # unchanged by depth: pose, both depths, the weight maps, the gradients of the weight heads and loss_weight
        assert all(torch.equal(out[i], frozen[i]) for i in range(3)) and all(torch.equal(x, y) for x, y in zip(out[3], frozen[3]))
        assert sorted(own(g_on)) == sorted(g_frozen) and 'loss_weight' in g_frozen and any(k.startswith('weight_head') for k in g_frozen)
        assert float(g_frozen['loss_weight'].abs().max()) > 0                # (the layer's backward ran: it hands back zeros where its solve fails)
        for k in g_frozen:
            assert torch.equal(g_on[k], g_frozen[k]), k
        leaves = out[-1]
        assert {k for k in leaves if isinstance(leaves[k], dict)} == {k for k in upd[-1] if isinstance(upd[-1][k], dict)} | {'fmap1', 'fmap2'}      # as at 'corr'
        # every parameter of RAFT has its gradient, the encoders' what the leaves' .grad give by hand: each image's d_out assembled
        # in the node's order with plain float32 adds (a two-term sum in f64 rounded once is the float32 sum)
        assert all(('flow.' + k) in g_on and bool(torch.isfinite(g_on['flow.' + k]).all()) for k, _ in model.flow.named_parameters())
        gr = lambda field, key: leaves[field][key].grad
        d_f = torch.cat((gr('fmap1', 'time') + gr('fmap1', 'stereo1'), gr('fmap2', 'time') + gr('fmap1', 'stereo2'), gr('fmap2', 'stereo1'),
                         gr('fmap2', 'stereo2')), dim=0)
        both = lambda key: torch.cat((gr('net0', key), gr('inp', key)), dim=1)
        d_c = torch.cat((both('time') + both('stereo1'), both('stereo2')), dim=0)
        want = inner(model.flow.fnet, [a['image1l'], a['image2l'], a['image1r'], a['image2r']], d_f, raw255=True) \
            + inner(model.flow.cnet, [a['image1l'], a['image2l']], d_c, raw255=True, split_act=True)
        params = raft_grad.encoder_params(model.flow.fnet) + raft_grad.encoder_params(model.flow.cnet)
        assert len(want) == len(params) == 94
        for i, (p, w) in enumerate(zip(params, want)):
            assert torch.equal(p.grad, w), i
        assert any(float(p.grad.abs().max()) > 0 for p in params[:32]) and all(float(p.grad.abs().max()) > 0 for p in params[32:])
        # the weight heads' context gradient reaches inp of the time pass (and only with use_weights)
        inp_raft = leaves['inp']['time'].grad.clone()
        assert inp_raft.shape == inp_update.shape and float((inp_raft - inp_update).abs().max()) > 0
        model.use_weights = False
        try:
            model.freeze_flow(True).freeze_flow(False, parts='update')
            plain_update = _step(model, a, target)[0][-1]['inp']['time'].grad.clone()
            model.freeze_flow(True).freeze_flow(False, parts='raft')
            plain_raft = _step(model, a, target)[0][-1]['inp']['time'].grad.clone()
        finally:
            model.use_weights = True
        assert torch.equal(plain_raft, plain_update)
        # parts='fnet': cnet is not run
        calls.clear()
        model.freeze_flow(True).freeze_flow(False, parts='fnet')
        _step(model, a, target)
        assert calls == [(model.flow.fnet, 4)]
        assert all(p.grad is None for p in model.flow.cnet.parameters()) and all(p.grad is not None for p in model.flow.fnet.parameters())
        assert all(torch.equal(p.grad, w) for p, w in zip(params[:32], want[:32]))
