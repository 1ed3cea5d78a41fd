"""GPU: the kernels of csrc/unet_train.hip ONE AT A TIME against float64, at the edges the whole-chain test (test_gpu_unet_train.py) does
not reach.  Each case runs one forward + backward through ops.unet_train_forward / _backward, reads every saved activation and every
activation gradient out of the workspace (ops.unet_train_workspace_views) and holds each stage's output against the float64 evaluation of
that stage from the buffers on its input side (tests/unet_train_ref.py: the restatement, the derivation of every bound, and the same
check the CPU mutation tests run).  Every element of every buffer is compared; max err / bound is printed per stage beside the figure of a
plain float32 CPU evaluation of the same stages (which is not expected to meet the long sums' bounds: the kernels add in float64)."""
import copy
import ctypes

import pytest
import torch

import unet_train_ref as R
from test_gpu_unet_train import forward_ref, make_net

pytestmark = pytest.mark.gpu


def make_case(cin, h8, w8, n, seed, out_size=None, train=True, ties=False):
    out_size = out_size or (8 * h8, 8 * w8)
    net = make_net(cin, out_size, seed).train(train)
    g = torch.Generator().manual_seed(seed + 2000)
    x = torch.randn(n, cin, h8, w8, generator=g)
    return net, (R.plant_ties(x) if ties else x), torch.randn(n, 1, *out_size, generator=g)


def run(net_cpu, parts, gout, sigmoid=False):
    """One forward + backward on a copy of the net -> (every buffer by ``walk``'s names on the CPU, the weight-gradient partials)."""
    from rpe_amd import ops, unet
    net = copy.deepcopy(net_cpu).cuda()
    ns = R.norms_of(net)
    norms = [(n.running_mean, n.running_var, n.num_batches_tracked, n.momentum, n.eps, n.training) for n in ns]
    params = [p.detach() for p in unet.train_params(net)]
    out, ctx = ops.unet_train_forward([p.cuda() if not p.is_cuda else p for p in parts], params, norms, net.out_sz, sigmoid)
    blob, gin = ops.unet_train_backward(gout.cuda(), out, ctx, input_grad=True)
    views = ops.unet_train_workspace_views(ctx)
    off = ops.unet_train_grad_offsets(ctx.cin)
    given = {k: v.cpu() for k, v in views.items() if k != 'wpart'}
    given.update(out=out.cpu(), gin=gin.cpu())
    for k, p in enumerate(params):
        given[f'grad.{k}'] = blob[off[k]:off[k + 1]].view(p.shape).cpu()
    for k, n in enumerate(ns):
        given[f'rm.{k}'], given[f'rv.{k}'], given[f'nbt.{k}'] = n.running_mean.cpu(), n.running_var.cpu(), int(n.num_batches_tracked)
    return given, views['wpart'].cpu()


def check(net, x, gout, given, tag, sigmoid=False, beside=True):
    inp = R.inputs_of(net, x, gout, sigmoid=sigmoid, count=True)
    figs, bad = R.check_run(inp, given, tag, beside=R.buffers(R.walk(inp, 'f32')) if beside else None)
    assert not bad, (tag, {k: figs[k] for k in bad})
    return inp


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(torch.int32) == b.view(torch.int32)).all())


# (cin, h8, w8, n, train): the smallest maps with batch statistics over one image; odd maps whose last row / column nothing pools, odd crop
# differences with dh != dw, two weight-gradient chunks; three chunks with a ragged last one; a pixel count that is exactly two chunks.
SHAPES = {'44x44-n1': (264, 44, 44, 1, True), '45x47-n3': (272, 45, 47, 3, True), '45x47-n3-frozen': (272, 45, 47, 3, False),
          '52x60-n3-three-chunks': (264, 52, 60, 3, True), '66x66-n2-exact-chunks': (8, 66, 66, 2, True)}


@pytest.mark.parametrize('name', list(SHAPES))
def test_every_stage_against_float64(rpe, name):
    cin, h8, w8, n, train = SHAPES[name]
    net, x, gout = make_case(cin, h8, w8, n, 41, train=train)
    given, wpart = run(net, [x], gout)
    inp = check(net, x, gout, given, name)
    pixels = n * (h8 - 2) * (w8 - 2)
    chunk, nchunk = R.wchunks(pixels)
    if name == '52x60-n3-three-chunks':
        assert (chunk, nchunk) == (4096, 3) and pixels % chunk == 508
    if name == '66x66-n2-exact-chunks':
        assert (chunk, nchunk) == (4096, 2) and pixels == 2 * chunk
    # the partials the last weight gradient (stage 0, conv1) left: each chunk's float64 sum, and their sum in index order rounded once
    count = 16 * cin * 9
    g, xs = given['g_r1.0'].double().permute(1, 0, 2, 3).reshape(16, -1), x.double()
    cols = torch.stack([xs[:, :, ky:ky + h8 - 2, kx:kx + w8 - 2] for ky in range(3) for kx in range(3)], 2).permute(1, 2, 0, 3, 4).reshape(cin * 9, -1)
    acc, flat = torch.zeros(count, dtype=torch.float64), wpart.reshape(-1)        # (partial z starts at z * count, whatever the largest weight)
    for z in range(nchunk):
        sl = slice(z * chunk, min((z + 1) * chunk, pixels))
        t, a = g[:, sl] @ cols[:, sl].T, g[:, sl].abs() @ cols[:, sl].abs().T
        part = flat[z * count:(z + 1) * count].reshape(16, cin * 9)
        worst = float(((part - t).abs() / ((chunk + 2) * R.E * a).clamp_min(1e-300)).max())
        print(f'{name} stage-0 weight-gradient partial {z} ({sl.stop - sl.start} pixels): max err / bound {worst:.3f}')
        assert bool(((part - t).abs() <= (chunk + 2) * R.E * a).all()), (z, worst)
        acc = acc + flat[z * count:(z + 1) * count]
    assert same_bits(acc.float().reshape(16, cin, 3, 3), given['grad.0'])
    if name.startswith('45x47'):
        # skip maps 41x43 and 16x17: row 40 / column 42 of stage 0 and column 16 of stage 1 are pooled by nothing, so they hold the skip
        # connection's share alone, bit for bit (here outside the centre crop: the share's absolute sum is zero and so is the restated share)
        ref = R.walk(inp, given=given)
        assert tuple(given['skip.0'].shape[-2:]) == (41, 43) and tuple(given['skip.1'].shape[-2:]) == (16, 17)
        s0, s1 = ref['share.0'][0].float(), ref['share.1'][0].float()
        assert same_bits(given['g_skip.0'][..., 40, :], s0[..., 40, :]) and same_bits(given['g_skip.0'][..., 42], s0[..., 42])
        assert same_bits(given['g_skip.1'][..., 16], s1[..., 16])
        assert float(ref['share.0'][1][..., 40, :].max()) == 0.0 and float(ref['share.1'][1][..., 16].max()) == 0.0
        assert float(given['g_pool.0'].abs().max()) > 0.0         # (something was there to be routed)


def test_parts_with_nan_neighbours_give_the_bits_of_the_dense_call(rpe):
    net, x, gout = make_case(272, 44, 44, 2, 43)
    dense, _ = run(net, [x], gout)
    xc = x.cuda()
    for cuts in ((0, 136, 272), (0, 8, 144, 272), (0, 8, 16, 144, 272)):
        wide = torch.full((2, 272 + 8 * len(cuts), 44, 44), float('nan'), device='cuda')
        parts, at = [], 4
        for a, b in zip(cuts, cuts[1:]):
            wide[:, at:at + b - a] = xc[:, a:b]
            parts.append(wide[:, at:at + b - a])
            at += b - a + 8
        got, _ = run(net, parts, gout)
        for k in dense:
            assert (dense[k] == got[k]) if isinstance(dense[k], int) else same_bits(dense[k], got[k]), (len(parts), k)


def test_planted_pool_ties_route_to_the_first_element(rpe):
    net, x, gout = make_case(264, 44, 44, 2, 45, ties=True)
    given, _ = run(net, [x], gout)
    check(net, x, gout, given, 'ties')
    sk = given['skip.0'][..., :10, :10]
    assert bool((sk.view(torch.int32) == sk.view(torch.int32)[..., :1, :1]).all())          # the tie, on the saved map itself
    # the corner lies outside the centre crop (rows and columns 16 .. 23 of the 40x40 map): the skip's share is exactly zero there
    gs, gp = given['g_skip.0'][..., :10, :10], given['g_pool.0'][..., :5, :5]
    assert float(gp.abs().min()) > 0.0
    assert same_bits(gs[..., 0::2, 0::2].contiguous(), gp.contiguous())
    for dy, dx in ((0, 1), (1, 0), (1, 1)):
        assert same_bits(gs[..., dy::2, dx::2].contiguous(), torch.zeros_like(gp))


def test_degenerate_statistics(rpe):
    """A stage-0 conv1 channel with zero weight and bias (zero variance: invstd = 1 / sqrt(eps), finite gradients, dgamma exactly 0), and
    conv1 biases that put every channel's mean at 50 standard deviations (mean / invstd within their one-rounding bounds)."""
    net, x, gout = make_case(264, 44, 44, 2, 47)
    c1 = net.encoder.enc_blocks[0].conv1
    with torch.no_grad():
        c1.weight[3].zero_(); c1.bias[3].zero_()
    given, _ = run(net, [x], gout)
    check(net, x, gout, given, 'zero-variance')
    assert same_bits(given['invstd.0'][3:4], (1.0 / torch.sqrt(torch.tensor([1e-5], dtype=torch.float32).double())).float())
    assert float(given['grad.2'][3]) == 0.0 and float(given['mean.0'][3]) == 0.0
    assert all(bool(torch.isfinite(given[f'grad.{k}']).all()) for k in range(36)) and bool(torch.isfinite(given['gin']).all())
    net, x, gout = make_case(264, 44, 44, 2, 48)
    c1 = net.encoder.enc_blocks[0].conv1
    with torch.no_grad():
        a = torch.nn.functional.conv2d(x.double(), c1.weight.double())
        c1.bias.copy_(50.0 * a.std((0, 2, 3)))
    given, _ = run(net, [x], gout)
    check(net, x, gout, given, 'mean = 50 std')
    a1 = given['a1.0'].double()
    ratio = a1.mean((0, 2, 3)).abs() / a1.std((0, 2, 3))
    assert float(ratio.min()) > 45.0


# the head map of a 44x44 grid is 4x4: the same size (every tap weight 0 or 1), one pixel, smaller on one axis and larger on the other
# (scale > 1 in k_t_resize_bwd's window), an output size the taps do not divide, the workload's 8x
@pytest.mark.parametrize('sigmoid', [False, True], ids=['plain', 'sigmoid'])
@pytest.mark.parametrize('out_size', [(4, 4), (1, 1), (2, 9), (350, 370), (352, 352)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_resize_sizes(rpe, out_size, sigmoid):
    net, x, gout = make_case(8, 44, 44, 2, 49, out_size=out_size)
    given, _ = run(net, [x], gout, sigmoid)
    assert tuple(given['hm'].shape[-2:]) == (4, 4)
    check(net, x, gout, given, f'resize {out_size} sigmoid={sigmoid}', sigmoid, beside=False)
    if out_size == (4, 4) and not sigmoid:
        assert same_bits(given['out'], given['hm']) and same_bits(given['g_hm'], gout)


@pytest.mark.parametrize('bias', [40.0, -40.0, -100.0])
def test_saturated_sigmoid(rpe, bias):
    """Head bias +40: exp(-v) is below half an ulp of 1, the output is exactly 1.0, y (1 - y) exactly 0 and with it every gradient.
    Head bias -100: exp(-v) overflows to inf, the output is exactly 0.0 and every gradient exactly 0.0; nothing is non-finite.
    Head bias -40: float32 holds 1 / (1 + e^40) = 4.2e-18, so neither the output nor the gradients are zeros there (in any float32
    evaluation): the output stays positive and below 2^-50 (the head map is below -35), and the stages keep their bounds."""
    net, x, gout = make_case(8, 44, 44, 2, 51)
    with torch.no_grad():
        net.head.bias.fill_(bias)
    given, _ = run(net, [x], gout, True)
    hm = given['hm']
    assert float(hm.min()) > 20.0 if bias > 0 else float(hm.max()) < (-90.0 if bias == -100.0 else -35.0)      # really saturated
    check(net, x, gout, given, f'sigmoid bias {bias}', True, beside=False)
    assert all(bool(torch.isfinite(v).all()) for v in given.values() if torch.is_tensor(v))
    if bias == -40.0:
        assert 0.0 < float(given['out'].min()) and float(given['out'].max()) < 2.0 ** -50
        return
    assert bool((given['out'] == (1.0 if bias > 0 else 0.0)).all())
    assert all(bool((given[f'grad.{k}'] == 0.0).all()) for k in range(36)) and bool((given['gin'] == 0.0).all())
    assert all(bool((v == 0.0).all()) for k, v in given.items() if k.startswith('g_'))


def test_zero_grad_out_gives_exact_zeros(rpe):
    net, x, gout = make_case(264, 45, 47, 2, 53)
    given, _ = run(net, [x], torch.zeros_like(gout))
    assert all(bool((given[f'grad.{k}'] == 0.0).all()) for k in range(36)) and bool((given['gin'] == 0.0).all())
    assert all(bool((v == 0.0).all()) for k, v in given.items() if k.startswith('g_'))


def test_nan_pixel_with_frozen_norms(rpe):
    net, x, gout = make_case(264, 45, 47, 2, 55, train=False)
    x[1, 100, 20, 21] = float('nan')
    given, _ = run(net, [x], gout)
    m = copy.deepcopy(net)
    xi = x.clone().requires_grad_(True)
    out = forward_ref(m, xi)
    out.backward(gout)
    assert bool(torch.isnan(out).any()) and not bool(torch.isnan(out).all())
    assert torch.equal(torch.isnan(given['out']), torch.isnan(out.detach()))
    assert torch.equal(torch.isnan(given['gin']), torch.isnan(xi.grad))
    check(net, x, gout, given, 'nan frozen', beside=False)          # a NaN truth asks for a NaN, everything else for its bound


def test_guards_and_workspace_contents_through_the_c_abi(rpe):
    """rpe_unet_train_forward / _backward called directly on guarded buffers: the bytes around out, the gradient blob, grad_input and both
    ends of the workspace stay as they were, and a workspace that held 0xFF bytes gives the bits of one that held zeros."""
    from rpe_amd import ops, unet
    L = rpe.lib()
    cin, n, h8, w8, H, W = 264, 2, 45, 47, 360, 376
    net, x, gout = make_case(cin, h8, w8, n, 57, out_size=(H, W))
    net = net.cuda()
    xc, gc = x.cuda(), gout.cuda()
    params = [p.detach() for p in unet.train_params(net)]
    G = 1024
    nws, nblob = L.rpe_unet_train_workspace_bytes(n, cin, h8, w8, H, W), L.rpe_unet_train_grad_floats(cin)
    results = []
    for fill in (0x00, 0xFF):
        ns = R.norms_of(copy.deepcopy(net))
        bufs = {k: torch.full((size + 2 * G,), 0xA5, dtype=torch.uint8, device='cuda')
                for k, size in (('out', 4 * n * H * W), ('blob', 4 * nblob), ('gin', 4 * x.numel()), ('ws', nws))}
        bufs['ws'][G:G + nws] = fill
        p = {k: ctypes.c_void_p(v.data_ptr() + G) for k, v in bufs.items()}
        assert bufs['ws'].data_ptr() % 256 == 0
        src, ch, bs = (ctypes.c_void_p * 1)(xc.data_ptr()), (ctypes.c_int * 1)(cin), (ctypes.c_longlong * 1)(cin * h8 * w8)
        prm = (ctypes.c_void_p * 36)(*[t.data_ptr() for t in params])
        rm = (ctypes.c_void_p * 5)(*[m.running_mean.data_ptr() for m in ns])
        rv = (ctypes.c_void_p * 5)(*[m.running_var.data_ptr() for m in ns])
        mom, eps = (ctypes.c_float * 5)(*[0.1] * 5), (ctypes.c_float * 5)(*[1e-5] * 5)
        stream = ops.stream_ptr()
        assert L.rpe_unet_train_forward(src, ch, bs, 1, prm, rm, rv, None, mom, eps, 31, n, h8, w8, H, W, 0, p['out'], p['ws'], stream) == 0
        assert L.rpe_unet_train_backward(ctypes.c_void_p(gc.data_ptr()), p['out'], src, ch, bs, 1, prm, 31, n, h8, w8, H, W, 0, p['blob'], p['gin'],
                                         p['ws'], stream) == 0
        torch.cuda.synchronize()
        for k, v in bufs.items():
            assert bool((v[:G] == 0xA5).all()) and bool((v[-G:] == 0xA5).all()), (fill, k)
        results.append({k: v[G:-G].clone() for k, v in bufs.items() if k != 'ws'})
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k


def test_two_runs_and_a_row_alone_give_the_same_bits(rpe):
    net, x, gout = make_case(264, 45, 47, 3, 59, train=False)
    a, _ = run(net, [x], gout)
    b, _ = run(net, [x], gout)
    for k in a:
        assert (a[k] == b[k]) if isinstance(a[k], int) else same_bits(a[k], b[k]), k
    one, _ = run(net, [x[:1]], gout[:1])
    assert same_bits(a['out'][:1], one['out']) and same_bits(a['gin'][:1], one['gin'])
    net.train()
    a, _ = run(net, [x], gout)
    b, _ = run(net, [x], gout)
    for k in a:
        assert (a[k] == b[k]) if isinstance(a[k], int) else same_bits(a[k], b[k]), k
