"""GPU: the backward of RAFT's output heads (csrc/raft_backward.hip, raft_grad.raft_tail_backward, RAFT.forward(grad_heads=True),
PoseNet.freeze_flow(False, parts='heads')).  Truth is float64 autograd on the CPU over the restatement tests/raft_tail_ref.py.
Bounds: where a result is a plain sum of products, the derived per-element bound n * 2^-24 * sum |a| |b| (n = terms + partials: any f32
summation order satisfies it, an indexing error does not); elsewhere the project's usual rule, twice the error of the same restatement run
in float32 on the CPU, relative to max |truth|.  The plumbing is compared bit for bit."""
import pytest
import torch
import torch.nn.functional as F

import raft_tail_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ up-sampling backward
def _up_case(b, hh, ww, seed, saturated=False):
    g = _gen(seed)
    flow = 3.0 * torch.randn(b, 2, hh, ww, generator=g)
    mask = 80.0 * torch.sign(torch.randn(b, 576, hh, ww, generator=g)) if saturated else 2.0 * torch.randn(b, 576, hh, ww, generator=g)
    return flow, mask, torch.randn(b, 2, 8 * hh, 8 * ww, generator=g)


def _up_grads(flow, mask, gup, dtype):
    fl, mk = flow.to(dtype).requires_grad_(True), mask.to(dtype).requires_grad_(True)
    return torch.autograd.grad((ref.upsample_convex(fl, mk) * gup.to(dtype)).sum(), [fl, mk])


@pytest.mark.parametrize('shape,saturated', [((1, 1, 1), False), ((2, 3, 5), False), ((1, 8, 12), False), ((1, 5, 7), False), ((2, 3, 5), True),
                                             ((1, 15, 29), False)])
def test_upsample_backward_against_float64(rpe, shape, saturated):
    """(1,1,1): every neighbour is padding; (1,15,29): more than one 14 x 14 tile in both directions, the last ones partial."""
    from rpe_amd import ops
    flow, mask, gup = _up_case(*shape, seed=11, saturated=saturated)
    t64, t32 = _up_grads(flow, mask, gup, torch.float64), _up_grads(flow, mask, gup, torch.float32)
    got = ops.upsample_convex_backward(gup.to(DEV), flow.to(DEV), mask.to(DEV))
    again = ops.upsample_convex_backward(gup.to(DEV), flow.to(DEV), mask.to(DEV))
    for name, g, a, w64, w32 in zip(('d_flow', 'd_mask'), got, again, t64, t32):
        r, r32 = ref.ratio(g, w64), ref.ratio(w32, w64)
        print(f'upsample backward {shape} saturated={saturated} {name}: GPU {r:.3e}  float32 on the CPU {r32:.3e}')
        assert bool(torch.isfinite(g).all()) and r <= 2.0 * r32, (name, r, r32)
        assert torch.equal(g, a), name
    # an all-zero truth comes out all zero: no incoming gradient; and a zero flow leaves the logits without one
    z = ops.upsample_convex_backward(torch.zeros_like(gup).to(DEV), flow.to(DEV), mask.to(DEV))
    assert not bool(z[0].any()) and not bool(z[1].any())
    z = ops.upsample_convex_backward(gup.to(DEV), torch.zeros_like(flow).to(DEV), mask.to(DEV))
    assert not bool(z[1].any()) and ref.ratio(z[0], _up_grads(torch.zeros_like(flow), mask, gup, torch.float64)[0]) <= 2.0 * ref.ratio(
        _up_grads(torch.zeros_like(flow), mask, gup, torch.float32)[0], _up_grads(torch.zeros_like(flow), mask, gup, torch.float64)[0])


# -------------------------------------------------------------------------------------------------------------------- weight gradient
def _wgrad(x, dy, k, dtype):
    """(dW, db) of y = conv(x; W) + b ('same') by autograd on the CPU."""
    cout, cin = dy.shape[1], x.shape[1]
    w = torch.zeros(cout, cin, k, k, dtype=dtype, requires_grad=True)
    bias = torch.zeros(cout, dtype=dtype, requires_grad=True)
    y = F.conv2d(x.to(dtype), w, bias, padding=k // 2)
    return torch.autograd.grad((y * dy.to(dtype)).sum(), [w, bias])


def _chunks(K):
    chunk = max(1024, (-(-K // 64) + 31) // 32 * 32)                    # include/rpe.h, rpe_conv_bwd_weight
    return -(-K // chunk)


WCASES = [((1, 1, 1), 128, 256, 3), ((2, 3, 5), 128, 256, 3), ((3, 8, 12), 128, 256, 3), ((1, 25, 41), 128, 256, 3),       # 1025 pixels: chunk + 1
          ((2, 3, 5), 256, 576, 1), ((2, 3, 5), 256, 2, 3), ((2, 5, 7), 12, 40, 3), ((1, 33, 37), 20, 2, 3)]


@pytest.mark.parametrize('shape,cin,cout,k', WCASES)
def test_weight_gradient_within_the_derived_bound(rpe, shape, cin, cout, k):
    from rpe_amd import ops
    b, hh, ww = shape
    g = _gen(17)
    x, dy = torch.randn(b, cin, hh, ww, generator=g), torch.randn(b, cout, hh, ww, generator=g)
    w64, b64 = _wgrad(x, dy, k, torch.float64)
    w32, b32 = _wgrad(x, dy, k, torch.float32)
    wabs, babs = _wgrad(x.abs(), dy.abs(), k, torch.float64)            # sum |dy| |x| over each element's terms
    K = b * hh * ww
    n = K + _chunks(K)
    dw, db = ops.conv_bwd_weight(x.to(DEV), dy.to(DEV), (k, k))
    dw2, db2 = ops.conv_bwd_weight(x.to(DEV), dy.to(DEV), (k, k))
    assert torch.equal(dw, dw2) and torch.equal(db, db2)                # two runs, the same bits
    ew, eb = (dw.cpu().double() - w64).abs(), (db.cpu().double() - b64).abs()
    e32 = float((w32.double() - w64).abs().max())
    print(f'weight gradient {shape} {cin}->{cout} {k}x{k}: max err {float(ew.max()):.3e} (bound at that element '
          f'{float((n * U * wabs).flatten()[ew.argmax()]):.3e}); float32 CPU backward {e32:.3e}; ratio {float(ew.max()) / max(e32, 1e-300):.2f}')
    assert bool((ew <= n * U * wabs).all()), float((ew / (n * U * wabs).clamp_min(1e-300)).max())
    assert bool((eb <= n * U * babs).all())
    # scaled results (the mask head's 0.25): exactly the scaled bits
    dws, dbs = ops.conv_bwd_weight(x.to(DEV), dy.to(DEV), (k, k), scale=0.25)
    assert torch.equal(dws, 0.25 * dw) and torch.equal(dbs, 0.25 * db)


def test_weight_gradient_on_channel_slices(rpe):
    """x and dy as channel slices of wider buffers (a batch stride beyond the slice): the bits of the dense call."""
    from rpe_amd import ops
    g = _gen(19)
    xb, yb = torch.randn(2, 150, 6, 10, generator=g).to(DEV), torch.randn(2, 300, 6, 10, generator=g).to(DEV)
    x, dy = xb[:, 11:139], yb[:, 30:286]
    for k in (3, 1):
        dense = ops.conv_bwd_weight(x.contiguous(), dy.contiguous(), (k, k))
        sliced = ops.conv_bwd_weight(x, dy, (k, k))
        assert torch.equal(dense[0], sliced[0]) and torch.equal(dense[1], sliced[1]), k


# --------------------------------------------------------------------------------------------------------------------- backward-data
@pytest.mark.parametrize('hh,ww', [(8, 12), (5, 7)])
def test_backward_data_through_the_transposed_packings(rpe, hh, ww):
    """dX = conv(dY; W^T flipped) on the forward's kernels: the tuned route (8x12: rpe_conv_fused) and the generic one (5x7:
    rpe_conv_direct), each on groups of input channels added in f64; the group sum itself; and the small kernels."""
    from rpe_amd import ops, raft_grad
    P = {k: v.to(DEV) for k, v in ref.make_params(128, 256, seed=23).items()}
    fh, mk = tuple(P[k] for k in ref.PARAMS[:4]), tuple(P[k] for k in ref.PARAMS[4:])
    T = raft_grad._packed(raft_grad._TailPacked, fh + mk)
    g = _gen(29)
    b = 2
    # the two 256 -> 128 3x3 layers, stacked: d_net = conv_T(g_f; fh1) + conv_T(g_m; m0)
    gg = torch.randn(b, 512, hh, ww, generator=g)
    d_net = T.conv_split('w3t', gg.to(DEV), T.w3t, None, False, raft_grad.TAIL_GROUP_3X3_BWD).cpu().double()
    wf, wm = P['fh1_w'].cpu().double(), P['m0_w'].cpu().double()
    want = F.conv_transpose2d(gg[:, :256].double(), wf, padding=1) + F.conv_transpose2d(gg[:, 256:].double(), wm, padding=1)
    bound = F.conv_transpose2d(gg[:, :256].double().abs(), wf.abs(), padding=1) + F.conv_transpose2d(gg[:, 256:].double().abs(), wm.abs(), padding=1)
    err = (d_net - want).abs()
    print(f'backward-data 3x3 {hh}x{ww}: max err {float(err.max()):.3e}, bound there {float((512 * 9 * U * bound).flatten()[err.argmax()]):.3e}')
    assert bool((err <= 512 * 9 * U * bound).all())
    # the 576 -> 256 1x1 layer (x 0.25)
    gm = torch.randn(b, 576, hh, ww, generator=g)
    out = T.conv_split('w1t', gm.to(DEV), T.w1t, None, False, raft_grad.TAIL_GROUP_1X1)
    w2 = 0.25 * P['m2_w'].cpu().double()
    want, bound = F.conv_transpose2d(gm.double(), w2), F.conv_transpose2d(gm.double().abs(), w2.abs())
    assert bool(((out.cpu().double() - want).abs() <= 576 * U * bound).all())
    # the group sum: f64 in group order, bias and ReLU, into a channel slice
    parts, bias = torch.randn(5, b, 7, hh, ww, generator=g), torch.randn(7, generator=g)
    buf = torch.full((b, 9, hh, ww), 7.0, device=DEV)
    ops.sum_groups(parts.to(DEV), bias.to(DEV), relu=True, out=buf[:, 1:8])
    want = torch.relu((parts.double().sum(0) + bias.double()[None, :, None, None]).float())
    assert torch.equal(buf[:, 1:8].cpu(), want) and bool((buf[:, 0] == 7.0).all()) and bool((buf[:, 8] == 7.0).all())
    assert torch.equal(ops.sum_groups(parts.to(DEV)).cpu(), parts.double().sum(0).float())
    # the 2 -> 256 layer with t_f's ReLU mask, and the mask alone
    dd, act = torch.randn(b, 2, hh, ww, generator=g), torch.randn(b, 256, hh, ww, generator=g)
    got = ops.conv3x3_to2_bwd_data(dd.to(DEV), P['fh2_w'], act=act.to(DEV)).cpu().double()
    w2 = P['fh2_w'].cpu().double()
    want = F.conv_transpose2d(dd.double(), w2, padding=1) * (act > 0)
    bound = F.conv_transpose2d(dd.double().abs(), w2.abs(), padding=1)
    assert bool(((got - want).abs() <= 18 * U * bound).all()) and bool((got[(act <= 0)] == 0).all())
    buf = torch.randn(b, 300, hh, ww, generator=g).to(DEV)
    keep = buf.clone()
    ops.relu_backward(buf[:, 20:276], act.to(DEV))
    assert torch.equal(buf[:, 20:276], keep[:, 20:276] * (act.to(DEV) > 0)) and torch.equal(buf[:, :20], keep[:, :20]) and torch.equal(buf[:, 276:], keep[:, 276:])


# ------------------------------------------------------------------------------------------------------------------------- whole tail
# Seeds chosen on the CPU (float64) so that no pre-activation of t_f or t_m lies within 1e-5 of max |pre-activation| of zero: a ReLU unit
# that close could be decided differently by the float32 kernels and the float64 truth, and the comparison below would then measure that
# one decision instead of the arithmetic.  The test asserts the condition; it is a condition on the inputs.
TAIL_CASES = [((2, 8, 12), 319), ((1, 5, 7), 5)]


@pytest.mark.parametrize('shape,seed', TAIL_CASES)
def test_whole_tail_against_float64(rpe, shape, seed):
    """raft_grad.raft_tail_backward against the float64 restatement under the twice-float32 rule, all nine results.  (With the forward kernels run
    over all input channels at once, d_net, fh2_w and m2_w came out at 2.3 - 4.4 times the float32 figure -- their k-ordered f32 sums of
    1152 and 4608 terms --; on groups of input channels added in f64 every result is at 0.1 - 1.6 times it.)"""
    from rpe_amd import raft_grad
    P = ref.make_params(128, 256, seed)
    c = ref.make_case(*shape, 128, seed)
    assert ref.relu_margin(c['net'], P) > 1e-5
    dn64, g64, low64, _ = ref.tail_grads(c, P, torch.float64)
    dn32, g32, _, _ = ref.tail_grads(c, P, torch.float32)
    Pd = {k: v.to(DEV) for k, v in P.items()}
    d_net, grads = raft_grad.raft_tail_backward(c['net'].to(DEV), low64.float().to(DEV), c['grad_up'].to(DEV), tuple(Pd[k] for k in ref.PARAMS[:4]),
                                          tuple(Pd[k] for k in ref.PARAMS[4:]))
    again = raft_grad.raft_tail_backward(c['net'].to(DEV), low64.float().to(DEV), c['grad_up'].to(DEV), tuple(Pd[k] for k in ref.PARAMS[:4]),
                                   tuple(Pd[k] for k in ref.PARAMS[4:]))
    assert torch.equal(d_net, again[0]) and all(torch.equal(a, b) for a, b in zip(grads, again[1]))
    missed = []
    for name, got, w64, w32 in [('d_net', d_net, dn64, dn32)] + [(k, g, g64[k], g32[k]) for k, g in zip(ref.PARAMS, grads)]:
        r, r32 = ref.ratio(got, w64), ref.ratio(w32, w64)
        print(f'whole tail {shape} {name}: GPU {r:.3e}  float32 on the CPU {r32:.3e}')
        if not r <= 2.0 * r32:
            missed.append((name, r, r32))
    assert not missed, missed


# --------------------------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope='module')
def raft_model(rpe):
    from rpe_amd import raft, synth
    return synth.init_synthetic_weights(raft.RAFT(synth.model_config(128, 160))).eval().to(DEV)


@pytest.mark.parametrize('h,w', [(128, 160), (136, 168)])
def test_grad_heads_is_the_plain_pass_plus_one_node(rpe, raft_model, h, w):
    """(128,160): 16 x 20 maps, the tuned route; (136,168): 17 x 21 maps, the generic route -- the smallest maps of either kind a RAFT pass takes
    (the correlation's four levels need a 1/8 map of at least 16 x 16: 64 x 96 and 72 x 104 images are refused by both correlation routes).  Predictions and hidden state are the plain pass's bits; after a backward the eight .grads and
    hidden.grad are the bits of a direct raft_grad.raft_tail_backward call on the pass's own outputs."""
    from rpe_amd import raft_grad
    g = _gen(31)
    im1, im2 = (255.0 * torch.rand(2, 3, h, w, generator=g)).to(DEV), (255.0 * torch.rand(2, 3, h, w, generator=g)).to(DEV)
    G = torch.randn(2, 2, h, w, generator=g).to(DEV)
    model = raft_model
    fh, mk = model.head_params()
    for p in fh + mk:
        p.requires_grad_(True)
        p.grad = None
    plain = model(im1, im2, ret_lowres=True)
    flows, hidden, context, low = model(im1, im2, ret_lowres=True, grad_heads=True)
    assert torch.equal(flows[-1], plain[0][-1]) and torch.equal(hidden, plain[1]) and torch.equal(context, plain[2]) and torch.equal(low, plain[3])
    assert hidden.is_leaf and hidden.requires_grad and flows[-1].requires_grad
    (flows[-1] * G).sum().backward()
    d_net, grads = raft_grad.raft_tail_backward(plain[1], plain[3], G, fh, mk)
    assert torch.equal(hidden.grad, d_net)
    for p, want in zip(fh + mk, grads):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0 and torch.equal(p.grad, want)
    assert all(p.grad is None for p in model.parameters() if all(p is not q for q in fh + mk))
    for p in fh + mk:
        p.requires_grad_(False)
        p.grad = None


def test_grad_heads_refusals_launch_nothing(rpe):
    from rpe_amd import _lib, raft, synth
    img = torch.zeros(1, 3, 128, 160, device=DEV)
    for key in ('update_fp16', 'mixed_precision'):
        model = raft.RAFT(dict(synth.model_config(128, 160), **{key: True})).eval().to(DEV)
        with _lib.CountingLib() as count, pytest.raises(_lib.RpeError, match=key):
            model(img, img, grad_heads=True)
        assert count.calls == 0
    model = raft.RAFT(synth.model_config(128, 160)).eval().to(DEV)
    keep, raft.CONV_BF16X3 = raft.CONV_BF16X3, True
    try:
        with _lib.CountingLib() as count, pytest.raises(_lib.RpeError, match='CONV_BF16X3'):
            model(img, img, grad_heads=True)
        assert count.calls == 0
    finally:
        raft.CONV_BF16X3 = keep


# ---------------------------------------------------------------------------------------------------------------------------- PoseNet
def _posenet_case():
    from rpe_amd import pose_net, synth
    h, w = 352, 352                                          # the 44 x 44 grid: the smallest the weight heads take
    model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(h, w, iters=12, lbgfs_iters=100))).to(DEV)
    model.train().freeze_flow(True)
    a = {k: v.to(DEV) for k, v in synth.stereo_frames(3, 1, h, w).items()}
    return model, a


def _step(model, a, target, **kw):
    model.zero_grad(set_to_none=True)
    out = model(a['image1l'], a['image2l'], a['K'], a['baseline'], a['image2r'], a['image2r'], mask1=a['mask1'], mask2=a['mask2'],
                ret_confmap=True, **kw)
    (out[0] - target).abs().sum().backward()
    return out, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def test_posenet_trains_the_output_heads(rpe):
    from rpe_amd import raft_grad
    model, a = _posenet_case()
    target = torch.tensor([[0.004, -0.003, 0.002, 0.01, -0.008, 0.006]], device=DEV)
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):      # (the module route of the weight heads)
        frozen, g_frozen = _step(model, a, target)
        model.freeze_flow(False, parts='heads')
        out, g_on = _step(model, a, target, ret_flows=True)
        heads = model.flow_head_params()
        names = [k for k, p in model.named_parameters() if any(p is q for q in heads)]
        assert len(names) == 8
        for k in names:
            assert k in g_on and bool(torch.isfinite(g_on[k]).all()) and float(g_on[k].abs().max()) > 0.0, k
        assert all(p.grad is None for k, p in model.flow.named_parameters() if 'flow.' + k not in names)
        # the hand chain: the flows' gradients -> raft_tail_backward per pass, summed in the node's order (time, stereo1, stereo2)
        flows = out[-1]
        hid = flows['hidden']
        n = 1
        with torch.no_grad():
            d1, sf1, v1, pass1 = model.flow2depth(a['image1l'], a['image2r'], a['baseline'].expand(1).contiguous(), grad='heads')
            f, cn = model._encode_both((a['image1l'], a['image2l'], a['image2r']), (a['image1l'], a['image2l']))
            r = model.flow(None, None, upsample=True, fmaps=(f[:2 * n], f[n:]), cnet=cn, ret_lowres=True)
        assert torch.equal(sf1, flows['stereo_flow1']) and torch.equal(r[0][-1][:n], flows['time_flow']) and torch.equal(r[0][-1][n:], flows['stereo_flow2'])
        fh, mk = model.flow.head_params()
        passes = [(flows['time_flow'].grad, r[1][:n], r[3][:n]), (flows['stereo_flow1'].grad, pass1.hidden.detach(), pass1.flow_low), (flows['stereo_flow2'].grad, r[1][n:], r[3][n:])]
        total, d_nets = None, []
        for gup, net, low in passes:
            d_net, pg = raft_grad.raft_tail_backward(net.contiguous(), low.contiguous(), gup.contiguous(), fh, mk)
            d_nets.append(d_net)
            total = list(pg) if total is None else [x + y for x, y in zip(total, pg)]
        for p, want in zip(fh + mk, total):
            assert torch.equal(p.grad, want)
        assert torch.equal(hid['stereo1'].grad, d_nets[1]) and torch.equal(hid['stereo2'].grad, d_nets[2])
        assert bool(torch.isfinite(hid['time'].grad).all()) and not torch.equal(hid['time'].grad, d_nets[0])      # (+ the weight heads' input gradient)
        # outputs and the other gradients are those of the frozen call; frozen again, the call is the parent's
        for i in range(3):
            assert torch.equal(out[i], frozen[i]), i
        for k in g_frozen:
            assert torch.equal(g_on[k], g_frozen[k]), k
        model.freeze_flow(True)
        again, g_again = _step(model, a, target)
        assert sorted(g_again) == sorted(g_frozen) and all(torch.equal(g_again[k], g_frozen[k]) for k in g_frozen)
        assert all(torch.equal(again[i], frozen[i]) for i in range(3))
    with pytest.raises(NotImplementedError, match='stop at the flows'):
        model.freeze_flow(False)
