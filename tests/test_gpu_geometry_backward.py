"""GPU: the backward of the fused geometry stage (csrc/geometry_backward.hip: rpe_depth_backproject_warp_backward, rpe_flow2depth_backward)
through ops, its autograd wiring (ops.geometry_stage, ops.flow2depth_grad) and PoseNet.forward(..., ret_flows=True).

Truth: torch autograd in float64 on the CPU over tests/geometry_grad_ref.py (pinned to the reference by tests/test_geometry_backward_host.py).
Measure, per output: max |kernel - f64| / max |f64| over every element.  Bound: TWICE the same quantity for the restatement run in float32
on the CPU with the same inputs -- both are float32-grade evaluations of one formula (the kernel takes its sampling positions and depth
validity in float32 exactly as torch does) that differ in summation order and contraction; twice is the margin the fused kernels' edge tests
allow for that.  An output whose float64 truth is all zeros must be all zeros.  The cases keep every sampling position's fractional part in
[0.05, 0.95] and every disparity 1e-3 from its thresholds, and each test asserts on the CPU side that float32 and float64 then take the
same tap and clamp decisions, so no element is left out.

Measured on an MI355X (ratios kernel / float32 restatement, worst output of each case): see NOTES.md, "Backward of the geometry stage"."""
import ctypes
import functools
import warnings

import pytest
import torch

import geometry_grad_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BWD_ARGS = ('stereo_flow2', 'time_flow', 'baseline', 'K', 'depth1', 'image2l', 'stereo_flow1', 'mask2')
SHAPES = [(1, 8, 8), (2, 16, 24), (3, 24, 40)]


def kernel(c, up, want=ref.GRADS):
    from rpe_amd import ops
    g = {'grad_' + k: (None if up.get(k) is None else up[k].to(DEV)) for k in ref.UPSTREAM}
    return ops.depth_backproject_warp_backward(*[c[k].to(DEV) for k in BWD_ARGS], **g, want=want)


@functools.lru_cache(maxsize=None)
def truth(n, h, w, only=None, **kw):
    """(case, upstream, float64 gradients, float32 gradients) of a seeded case: computed once, shared, never modified."""
    c = ref.case(n, h, w, **kw)
    ref.decisions(c)
    up = ref.upstream(n, h, w, only=only)
    return c, up, ref.stage_grads(c, up, torch.float64), ref.stage_grads(c, up, torch.float32)


def check_parity(got, g64, g32, label):
    for k in ref.GRADS:
        rk, r32 = ref.ratio(got[k], g64[k]), ref.ratio(g32[k], g64[k])
        print(f'{label} {k}: kernel {rk:.3e}  float32 restatement {r32:.3e}')
        assert rk <= 2.0 * r32, (label, k, rk, r32)


@pytest.mark.parametrize('only', [None, 'pcl1', 'pcl2w', 'inp1', 'inp2'])
@pytest.mark.parametrize('n,h,w', SHAPES)
def test_parity_against_float64(rpe, n, h, w, only):
    c, up, g64, g32 = truth(n, h, w, only)
    check_parity(kernel(c, up), g64, g32, f'{n}x{h}x{w} {only or "all"}')


def test_flow2depth_backward_and_grad_form(rpe):
    from rpe_amd import ops
    c = ref.case(3, 24, 40, seed=2)
    ref.decisions(c)
    gd = torch.randn(3, 1, 24, 40, generator=torch.Generator().manual_seed(5))
    got = ops.flow2depth_backward(c['stereo_flow1'].to(DEV), c['baseline'].to(DEV), gd.to(DEV)).cpu()

    def by_autograd(dtype):
        s = c['stereo_flow1'].to(dtype).clone().requires_grad_(True)
        return torch.autograd.grad((ref.flow2depth(s, c['baseline'].to(dtype))[0] * gd.to(dtype)).sum(), s)[0]
    g64, g32 = by_autograd(torch.float64), by_autograd(torch.float32)
    rk, r32 = ref.ratio(got, g64), ref.ratio(g32, g64)
    print(f'flow2depth_backward: kernel {rk:.3e}  float32 restatement {r32:.3e}')
    assert rk <= 2.0 * r32 and float(got[:, 1].abs().max()) == 0.0
    clamped = ~ref.flow2depth(c['stereo_flow1'], c['baseline'])[1]
    assert bool(clamped.any()) and float(got[:, 0:1][clamped].abs().max()) == 0.0
    s = c['stereo_flow1'].to(DEV).requires_grad_(True)
    depth, valid = ops.flow2depth_grad(s, c['baseline'].to(DEV))
    d0, v0 = ops.flow2depth(s.detach(), c['baseline'].to(DEV))
    assert torch.equal(depth, d0) and torch.equal(valid, v0) and depth.requires_grad and not valid.requires_grad
    (depth * gd.to(DEV)).sum().backward()
    assert torch.equal(s.grad.cpu(), got)


def test_integer_positions_and_last_row_and_column(rpe):
    """Integer flows: positions exactly on pixels, the last row and column included.  In float32 such a position is the integer or a hair
    beside it, and the gradient with respect to the position jumps there; the kernel differentiates the taps its forward reads
    (rpe_warp_taps), so the truth is torch's float64 gradient of grid_sample's own arithmetic AT THOSE TAPS (ref.remap_at_taps)."""
    from rpe_amd import ops
    n, h, w = 2, 16, 24
    c = ref.case(n, h, w, seed=3, integer_positions=True)
    ref.decisions(c, positions_too=False)
    taps = {k: v.cpu() for k, v in ops.warp_taps(c['time_flow'].to(DEV)).items()}
    px, py = ref.positions(c['time_flow'], torch.float32)
    on_pixel = (px == px.round()) & (py == py.round())
    assert int(on_pixel.sum()) > n * h * w // 2 and bool((px == w - 1).any()) and bool((py == h - 1).any())
    assert torch.equal(taps['x0'].long(), px.floor().long()) and torch.equal(taps['y0'].long(), py.floor().long())
    s = ref.remap_at_taps(taps)
    up = ref.upstream(n, h, w, seed=3)
    g64, g32 = ref.stage_grads(c, up, torch.float64, sampler=s), ref.stage_grads(c, up, torch.float32, sampler=s)
    check_parity(kernel(c, up), g64, g32, 'integer positions')


def test_clamped_row_and_null_outputs(rpe):
    n, h, w = 2, 16, 24
    c, up, g64, g32 = truth(n, h, w, None, seed=4, clamp_row=1)
    full = kernel(c, up)
    check_parity(full, g64, g32, 'clamped row')
    cloud_only = kernel(c, dict(up, inp1=None, inp2=None))
    assert float(cloud_only['stereo_flow2'][1].abs().max()) == 0.0 and float(cloud_only['stereo_flow2'][0].abs().max()) > 0.0
    stack_only = kernel(c, dict(up, pcl1=None, pcl2w=None, inp1=None))
    assert float((full['stereo_flow2'][1, 1] - stack_only['stereo_flow2'][1, 1]).abs().max()) == 0.0       # .y never sees the cloud
    # an all-clamped row's .x is the direct inp2 path alone, up to the float64 sum's one rounding
    r = ref.ratio(full['stereo_flow2'][1, 0], g64['stereo_flow2'][1, 0])
    assert r <= 2.0 * ref.ratio(g32['stereo_flow2'][1, 0], g64['stereo_flow2'][1, 0])
    for want in (['time_flow'], ['stereo_flow2'], ['stereo_flow1', 'depth1'], ['depth1', 'stereo_flow2']):
        part = kernel(c, up, want=want)
        assert sorted(part) == sorted(want)
        for k in want:
            assert torch.equal(part[k], full[k]), (want, k)


def test_many_to_one_scatter(rpe):
    """Every destination samples the same source cell: four lists of h*w entries each (heapsort route), the rest empty."""
    n, h, w = 1, 16, 24
    c, up, g64, g32 = truth(n, h, w, None, seed=6, many_to_one=True)
    a, b = kernel(c, up), kernel(c, up)
    check_parity(a, g64, g32, 'many to one')
    assert int((g64['stereo_flow2'].abs().sum(1) > 0).sum()) == 4
    for k in ref.GRADS:
        assert torch.equal(a[k], b[k]), k


def test_deterministic_and_independent_of_the_batch(rpe):
    n, h, w = 3, 24, 40
    c, up, _, _ = truth(n, h, w, None)
    a, b = kernel(c, up), kernel(c, up)
    for k in ref.GRADS:
        assert torch.equal(a[k], b[k]), k
    for r in range(n):
        alone = kernel({k: v[r:r + 1].clone() for k, v in c.items()}, {k: v[r:r + 1].clone() for k, v in up.items()})
        for k in ref.GRADS:
            assert torch.equal(alone[k][0], a[k][r]), (r, k)
    # a NaN in one row's upstream gradient stays in that row
    bad = {k: v.clone() for k, v in up.items()}
    bad['pcl2w'][1, 0, 5, 7] = float('nan')
    bad['inp2'][1, 3, 1, 2] = float('nan')
    bad['pcl1'][1, 2, 0, 0] = float('nan')
    g = kernel(c, bad)
    for k in ref.GRADS:
        assert torch.equal(g[k][0], a[k][0]) and torch.equal(g[k][2], a[k][2]), k
    assert bool(torch.isnan(g['time_flow'][1]).any()) and bool(torch.isnan(g['depth1'][1]).any())


def test_guard_bytes_around_every_output(rpe):
    """The raw entry point, every output a region of a larger buffer of 0xA5 bytes (regions start 16 bytes past a 256-byte boundary): no
    byte outside the regions changes, and the regions hold the bits ops.depth_backproject_warp_backward returns."""
    from rpe_amd._lib import lib, ptr, stream_ptr
    n, h, w = 3, 24, 40
    c, up, _, _ = truth(n, h, w, None)
    want = kernel(c, up)
    ins = [c[k].to(DEV).contiguous() for k in BWD_ARGS]
    ins[-1] = ins[-1].view(torch.uint8)
    gin = [up[k].to(DEV).contiguous() for k in ref.UPSTREAM]
    pad = 256 + 16
    bufs = {}
    for k, ch in (('time_flow', 2), ('stereo_flow2', 2), ('stereo_flow1', 2), ('depth1', 1)):
        nbytes = n * ch * h * w * 4
        bufs[k] = (torch.full((pad + nbytes + 256,), 0xA5, dtype=torch.uint8, device=DEV), nbytes)
    ws_bytes = lib().rpe_depth_backproject_warp_backward_workspace_bytes(n, h, w)
    ws = torch.full((ws_bytes + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0 and all(b.data_ptr() % 256 == 0 for b, _ in bufs.values())
    vp = lambda b: ctypes.c_void_p(b.data_ptr() + pad)                     # noqa: E731
    st = lib().rpe_depth_backproject_warp_backward(*[ptr(t) for t in ins], n, h, w, *[ptr(t) for t in gin],
                                                   *[vp(bufs[k][0]) for k in ref.GRADS], ctypes.c_void_p(ws.data_ptr() + 256), stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    for k, (b, nbytes) in bufs.items():
        assert bool((b[:pad] == 0xA5).all()) and bool((b[pad + nbytes:] == 0xA5).all()), k
        assert torch.equal(b[pad:pad + nbytes].view(torch.float32).view_as(want[k]), want[k]), k
    assert bool((ws[:256] == 0xA5).all()) and bool((ws[256 + ws_bytes:] == 0xA5).all())


def test_autograd_wiring(rpe):
    from rpe_amd import ops
    n, h, w = 2, 16, 24
    c, up, _, _ = truth(n, h, w, None)
    d = {k: v.to(DEV) for k, v in c.items()}
    plain = ops.depth_backproject_warp(*[d[k] for k in ref.INPUTS])
    leaves = {k: d[k].clone().requires_grad_(True) for k in ref.GRADS}
    g = ops.geometry_stage(*[leaves.get(k, d[k]) for k in ref.INPUTS])
    assert sorted(g) == sorted(plain) and g['pcl2'] is None
    for k in ('depth2', 'mask2', 'pcl1', 'pcl2w', 'mask2w', 'inp1', 'inp2'):
        assert torch.equal(g[k], plain[k]), k
    assert all(g[k].requires_grad for k in ref.UPSTREAM) and not any(g[k].requires_grad for k in ('depth2', 'mask2', 'mask2w'))
    sum((g[k] * up[k].to(DEV)).sum() for k in ref.UPSTREAM).backward()
    raw = kernel(c, up)
    for k in ref.GRADS:
        assert torch.equal(leaves[k].grad, raw[k]), k
    # an output nothing differentiates is the kernel's NULL, not a tensor of zeros
    leaves = {k: d[k].clone().requires_grad_(True) for k in ref.GRADS}
    g = ops.geometry_stage(*[leaves.get(k, d[k]) for k in ref.INPUTS])
    (g['pcl2w'] * up['pcl2w'].to(DEV)).sum().backward()
    raw = kernel(c, dict(up, pcl1=None, inp1=None, inp2=None))
    for k in ref.GRADS:
        assert torch.equal(leaves[k].grad, raw[k]), k


# ----------------------------------------------------------------------------------------------------------------------- PoseNet level
def _posenet_case(train_heads_hip=False):
    from rpe_amd import pose_net, synth
    # the smallest size the heads take as modules: a 44x44 grid (TinyUNet needs 44; its module route's centre crop needs the skip and the
    # up-sampled map to differ by an even count, which a 45-wide grid does not give)
    h, w = 352, 352
    cfg = dict(synth.model_config(h, w, iters=12, lbgfs_iters=100), train_heads_hip=train_heads_hip)
    model = synth.init_synthetic_weights(pose_net.PoseNet(cfg)).to(DEV)
    model.train().freeze_flow(True)
    a = {k: v.to(DEV) for k, v in synth.stereo_frames(3, 1, h, w).items()}   # a rigid scene with a known small motion: the solve converges
    return model, a


def _step(model, a, target, **kw):
    model.zero_grad(set_to_none=True)
    out = model(a['image1l'], a['image2l'], a['K'], a['baseline'], a['image2r'], a['image2r'], mask1=a['mask1'], mask2=a['mask2'],
                ret_confmap=True, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                                     # converged: no optimality warning, no zeroed gradients
        (out[0] - target).abs().sum().backward()
    return out, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('train_heads_hip', [False, True])
def test_posenet_flow_gradients_match_float64_chain(rpe, train_heads_hip):
    """Acceptance: d loss / d (time_flow, stereo_flow1, stereo_flow2) of the supervised L1 pose loss from PoseNet.forward(ret_flows=True)
    against a float64 CPU evaluation of the same chain -- the oracle's pose-layer gradient (fed the GPU's flows, weight maps and solved
    pose), the heads as float64 modules, the stage restatement -- within twice the error of that chain run in float32 on the CPU.
    On both head routes: the chain's head part reaches the flows only through the input gradients the heads' backward returns, so a route
    that stopped returning them (config['train_heads_hip']: csrc/unet_train.hip) would miss this bound, not pass silently."""
    import copy
    from oracle import pose_grad
    from rpe_amd import ops
    model, a = _posenet_case(train_heads_hip)
    problem = model.pose_head.problem
    seen, real = {}, problem.solve

    def recording(*xs):
        r = real(*xs)
        seen['vec7'] = r[1][0].detach().clone()
        return r
    problem.solve = recording
    target = torch.tensor([[0.004, -0.003, 0.002, 0.01, -0.008, 0.006]], device=DEV)
    out, _ = _step(model, a, target, ret_flows=True)
    problem.solve = real
    pose_tan, (w2d, w3d), flows = out[0], out[3], out[-1]
    assert sorted(flows) == ['stereo_flow1', 'stereo_flow2', 'time_flow']
    for k, f in flows.items():
        assert f.grad is not None and bool(torch.isfinite(f.grad).all()) and float(f.grad.abs().max()) > 0.0, k
    # the rest of the chain's inputs, from the GPU
    n, b, K = 1, a['baseline'].expand(1).contiguous(), a['K'].expand(1, 3, 3).contiguous()
    fl = {k: v.detach() for k, v in flows.items()}
    depth1, valid1 = ops.flow2depth(fl['stereo_flow1'], b)
    g = ops.depth_backproject_warp(fl['stereo_flow2'], fl['time_flow'], b, K, depth1, a['image1l'], a['image2l'], fl['stereo_flow1'],
                                   a['mask2'].bool())
    with torch.no_grad():
        r = model.stages(a['image1l'], a['image2l'], K, b, depth1, a['image2r'], a['mask1'].bool() & valid1, a['mask2'].bool().clone(),
                         fl['stereo_flow1'], heads=False)
    assert torch.equal(r['time_flow'], fl['time_flow']) and torch.equal(r['stereo_flow2'], fl['stereo_flow2'])
    hidden, context = r['hidden'].cpu(), r['context'].cpu()
    lw = model.loss_weight.detach().cpu()[None, :].repeat(n, 1)
    v = torch.sign(pose_tan.detach() - target).cpu().double()
    cpu = lambda t: t.detach().cpu()                                       # noqa: E731
    layer, fY, _ = pose_grad.layer_backward(cpu(fl['time_flow']), cpu(g['pcl1']), cpu(g['pcl2w']), cpu(w2d), cpu(w3d),
                                            cpu(a['mask1'].bool() & valid1), cpu(g['mask2w']), cpu(K), lw, cpu(seen['vec7']), v)
    assert float(fY.abs().max()) <= 1e-3 and float(layer['flow'].abs().max()) > 0.0          # the solve met the layer's convergence test
    case = dict(stereo_flow2=cpu(fl['stereo_flow2']), time_flow=cpu(fl['time_flow']), baseline=cpu(b), K=cpu(K), image1l=cpu(a['image1l']),
                image2l=cpu(a['image2l']), stereo_flow1=cpu(fl['stereo_flow1']))
    ref.decisions(case, positions_too=False, margins=False)               # (RAFT's own flows: float32 and float64 clamp the same pixels)

    def chain(dtype):
        heads = [copy.deepcopy(h).cpu().to(dtype).train() for h in (model.weight_head_2d, model.weight_head_3d)]
        for hd in heads:
            hd[0].train_hip = False                                        # the truth's heads are torch modules on the CPU
        c = {k: t.to(dtype) for k, t in case.items()}
        leaves = {k: c[k].clone().requires_grad_(True) for k in ('time_flow', 'stereo_flow1', 'stereo_flow2')}
        d1 = ref.flow2depth(leaves['stereo_flow1'], c['baseline'])[0]
        o = ref.stage(leaves['stereo_flow2'], leaves['time_flow'], c['baseline'], c['K'], d1, c['image1l'], c['image2l'], leaves['stereo_flow1'])
        hc = (hidden.to(dtype), context.to(dtype))
        w1 = heads[0](torch.cat((o['inp1'], *hc), dim=1))
        w2 = heads[1](torch.cat((o['inp1'], o['inp2'], *hc), dim=1))
        total = sum((x * layer[k].to(dtype)).sum() for x, k in ((leaves['time_flow'], 'flow'), (o['pcl1'], 'pcl1'), (o['pcl2w'], 'pcl2'),
                                                                  (w1, 'w1'), (w2, 'w2')))
        return dict(zip(leaves, torch.autograd.grad(total, list(leaves.values()))))
    g64, g32 = chain(torch.float64), chain(torch.float32)
    for k in ('time_flow', 'stereo_flow1', 'stereo_flow2'):
        rk, r32 = ref.ratio(flows[k].grad, g64[k]), ref.ratio(g32[k], g64[k])
        print(f'PoseNet d loss / d {k}: GPU {rk:.3e}  float32 chain on the CPU {r32:.3e}')
        assert rk <= 2.0 * r32, (k, rk, r32)


@pytest.mark.parametrize('train_heads_hip', [True, False])
def test_posenet_flag_has_no_side_effect(rpe, monkeypatch, train_heads_hip):
    """Outputs, loss_weight and head-parameter gradients with the flag on and off: torch.equal, on both head routes.  The module route's
    weight gradients come from PyTorch-ROCm's convolution backward, whose default algorithms are not reproducible from run to run (two
    DEFAULT calls were seen to differ in 4 of the 73 gradient tensors by 4.2e-7 of their scale on an MI355X), so both steps run under
    torch.backends.cudnn.flags(deterministic=True) -- MIOpen's deterministic mode, scoped to this test -- in which default against default,
    flagged against flagged and flagged against default were all bit-equal.  The hand-written route (config['train_heads_hip']) is
    deterministic by construction; the mode does not touch it."""
    from rpe_amd import ops
    model, a = _posenet_case(train_heads_hip)
    target = torch.zeros(1, 6, device=DEV)
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        on, g_on = _step(model, a, target, ret_flows=True)
        assert all(f.grad is not None and float(f.grad.abs().max()) > 0.0 for f in on[-1].values())
        with monkeypatch.context() as m:                                    # the default call must not route through the autograd functions

            def refuse(*args, **kw):
                raise AssertionError('the default PoseNet.forward must not call the differentiable geometry stage')
            m.setattr(ops, 'geometry_stage', refuse)
            m.setattr(ops, 'flow2depth_grad', refuse)
            m.setattr(ops, 'depth_backproject_warp_backward', refuse)
            off, g_off = _step(model, a, target)
    assert len(off) == 4 and len(on) == 5
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and torch.equal(on[2], off[2])
    assert torch.equal(on[3][0], off[3][0]) and torch.equal(on[3][1], off[3][1])
    assert sorted(g_on) == sorted(g_off) and 'loss_weight' in g_on and any(k.startswith('weight_head') for k in g_on)
    for k in g_on:
        assert torch.equal(g_on[k], g_off[k]), k
    with pytest.raises(NotImplementedError, match='stop at the flows'):
        model.freeze_flow(False)
