"""GPU: the backward of RAFT's encoders (csrc/encoder_backward.hip, raft_grad.residual_block_backward / encoder_backward,
RAFT.backward_encoders).  Truth is float64 autograd on the CPU over oracle/raft.py's ResidualBlock / BasicEncoder and
torch.nn.functional.conv2d.  Bounds: where a result is a plain sum of products, the derived per-element bound n * 2^-24 * sum |a| |b|
(n = terms + partials for the f32 matrix-core sums; n = 2 for a sum that runs in f64 and is rounded once); for elementwise results
2 * 2^-24 * max |truth| + 1e-12; for a block, an encoder and the chain, twice the error of the same float32 autograd on the CPU, relative to
max |truth|.  ReLU masks are discrete: the block and encoder cases run on seeds chosen on the CPU so that no ReLU input of the float64
reference lies within 1e-5 of zero (asserted; a condition on the inputs)."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ratio(got, want):
    return float((got.detach().cpu().double() - want.detach().double()).abs().max()) / max(float(want.detach().abs().max()), 1e-300)


def _chunks(K):
    chunk = max(1024, (-(-K // 64) + 31) // 32 * 32)                    # include/rpe.h, rpe_conv_bwd_weight's rule
    return -(-K // chunk)


def _out(n, k):
    return (n + 2 * (k // 2) - k) // 2 + 1


# ------------------------------------------------------------------------------------------------------------ strided weight gradient
def _wgrad(x, dy, k, dtype):
    w = torch.zeros(dy.shape[1], x.shape[1], k, k, dtype=dtype, requires_grad=True)
    bias = torch.zeros(dy.shape[1], dtype=dtype, requires_grad=True)
    y = F.conv2d(x.to(dtype), w, bias, stride=2, padding=k // 2)
    return torch.autograd.grad((y * dy.to(dtype)).sum(), [w, bias])


# (b, hi, wi), cin, cout, k: odd and even maps; the stem's ragged N tile (147 columns); K = 2 * 24 * 24 = 1152 > 1024: two chunks
WCASES = [((2, 5, 9), 5, 7, 3), ((2, 5, 9), 5, 7, 1), ((2, 6, 8), 5, 7, 3), ((2, 6, 8), 5, 7, 1), ((2, 10, 18), 3, 64, 7), ((2, 48, 48), 4, 8, 3)]


@pytest.mark.parametrize('shape,cin,cout,k', WCASES)
def test_strided_weight_gradient_within_the_derived_bound(rpe, shape, cin, cout, k):
    from rpe_amd import ops
    b, hi, wi = shape
    ho, wo = _out(hi, k), _out(wi, k)
    g = _gen(17)
    x, dy = torch.randn(b, cin, hi, wi, generator=g), torch.randn(b, cout, ho, wo, generator=g)
    w64, b64 = _wgrad(x, dy, k, torch.float64)
    wabs, babs = _wgrad(x.abs(), dy.abs(), k, torch.float64)              # sum |dy| |x| over each element's terms
    K = b * ho * wo
    assert _chunks(K) == (2 if shape == (2, 48, 48) else 1)
    n = K + _chunks(K)
    dw, db = ops.conv_s2_bwd_weight(x.to(DEV), dy.to(DEV), k)
    dw2, db2 = ops.conv_s2_bwd_weight(x.to(DEV), dy.to(DEV), k)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)                # two runs, the same bits
    ew, eb = (dw.cpu().double() - w64).abs(), (db.cpu().double() - b64).abs()
    print(f'strided weight gradient {shape} {cin}->{cout} k={k}: max err {float(ew.max()):.3e} (bound at that element '
          f'{float((n * U * wabs).flatten()[ew.argmax()]):.3e}), bias {float(eb.max()):.3e}')
    assert bool((ew <= n * U * wabs).all()), float((ew / (n * U * wabs).clamp_min(1e-300)).max())
    assert bool((eb <= n * U * babs).all())
    dws, dbs = ops.conv_s2_bwd_weight(x.to(DEV), dy.to(DEV), k, scale=0.25)
    assert torch.equal(dws, 0.25 * dw) and torch.equal(dbs, 0.25 * db)
    # operands as channel slices of larger buffers: the bits of the dense call
    xb, yb = torch.full((b, cin + 5, hi, wi), 1e30, device=DEV), torch.full((b, cout + 7, ho, wo), 1e30, device=DEV)
    xb[:, 2:2 + cin], yb[:, 3:3 + cout] = x.to(DEV), dy.to(DEV)
    dw3, db3 = ops.conv_s2_bwd_weight(xb[:, 2:2 + cin], yb[:, 3:3 + cout], k)
    assert torch.equal(dw3, dw) and torch.equal(db3, db)


@pytest.mark.parametrize('k', [3, 1, 7])
def test_strided_weight_gradient_leaves_the_guards(rpe, k):
    """The entry point on outputs inside guard values: nothing around d_weight and d_bias is written."""
    from rpe_amd import ops
    b, cin, cout, hi, wi = 2, 3, 7, 5, 9
    ho, wo = _out(hi, k), _out(wi, k)
    g = _gen(23)
    x, dy = torch.randn(b, cin, hi, wi, generator=g).to(DEV), torch.randn(b, cout, ho, wo, generator=g).to(DEV)
    per = cout * cin * k * k
    wbuf, bbuf = torch.full((per + 64,), 7.0, device=DEV), torch.full((cout + 64,), 7.0, device=DEV)
    L = rpe.lib()
    ws = torch.empty(L.rpe_conv_s2_bwd_weight_workspace_bytes(b, cin, cout, hi, wi, ho, wo, k), dtype=torch.uint8, device=DEV)
    vp = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    assert L.rpe_conv_s2_bwd_weight(vp(x), cin * hi * wi, vp(dy), cout * ho * wo, b, cin, cout, hi, wi, ho, wo, k, 1.0, vp(wbuf, 32), vp(bbuf, 32),
                                    vp(ws), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    dw, db = ops.conv_s2_bwd_weight(x, dy, k)
    assert torch.equal(wbuf[32:32 + per], dw.flatten()) and torch.equal(bbuf[32:32 + cout], db)
    for buf, m in ((wbuf, per), (bbuf, cout)):
        assert bool((buf[:32] == 7.0).all()) and bool((buf[32 + m:] == 7.0).all())


# -------------------------------------------------------------------------------------------------------------- strided data gradient
def _dgrad(dy, w, size, dtype):
    x = torch.zeros(dy.shape[0], w.shape[1], *size, dtype=dtype, requires_grad=True)
    y = F.conv2d(x, w.to(dtype), None, stride=2, padding=w.shape[2] // 2)
    return torch.autograd.grad((y * dy.to(dtype)).sum(), x)[0]


DCASES = [((2, 5, 9), 5, 7), ((2, 6, 8), 5, 7), ((1, 6, 8), 64, 96)]      # ... and one real layer shape


@pytest.mark.parametrize('k', [3, 1])
@pytest.mark.parametrize('shape,cin,cout', DCASES)
def test_strided_data_gradient_within_the_derived_bound(rpe, shape, cin, cout, k):
    """The sum over (cout, taps) runs in f64 and is rounded once: |err| <= 2^-25 |dx| <= 2^-24 sum |terms|; n = 2 leaves the f64 chain
    (cout * 4 terms at 2^-53 each) more room than it can use."""
    from rpe_amd import ops
    b, hi, wi = shape
    ho, wo = _out(hi, k), _out(wi, k)
    g = _gen(29)
    dy, w = torch.randn(b, cout, ho, wo, generator=g), torch.randn(cout, cin, k, k, generator=g)
    t64, tabs = _dgrad(dy, w, (hi, wi), torch.float64), _dgrad(dy.abs(), w.abs(), (hi, wi), torch.float64)
    buf = torch.full((b, cin + 6, hi, wi), 7.0, device=DEV)              # the result as a channel slice between guards
    dx = ops.conv_s2_bwd_data(dy.to(DEV), w.to(DEV), (hi, wi), out=buf[:, 3:3 + cin])
    again = ops.conv_s2_bwd_data(dy.to(DEV), w.to(DEV), (hi, wi))
    assert torch.equal(dx, again)
    assert bool((buf[:, :3] == 7.0).all()) and bool((buf[:, 3 + cin:] == 7.0).all())
    e = (dx.cpu().double() - t64).abs()
    print(f'strided data gradient {shape} {cin}->{cout} k={k}: max err {float(e.max()):.3e}, max |truth| {float(t64.abs().max()):.3e}')
    assert bool((e <= 2 * U * tabs).all()), float((e / (2 * U * tabs).clamp_min(1e-300)).max())
    assert not bool(dx.cpu()[tabs == 0].any())                          # exact zeros where no tap reaches
    if k == 1:
        reached = torch.zeros(hi, wi, dtype=torch.bool)
        reached[::2, ::2] = True                                        # one pixel in four; an odd last row / column of an even map is not among them
        assert bool(((tabs != 0).any(1).any(0) == reached).all()) and not bool(dx[:, :, ~reached.to(DEV)].any())
    else:
        assert bool((tabs != 0).all())


# ----------------------------------------------------------------------------------------------------------------------- norm adjoints
NCASES = [(2, 3, 3, 5), (2, 3, 2, 1), (2, 64, 16, 24), (2, 64, 3, 5)]


def _bn_case(b, c, hh, ww, seed):
    g = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(dy=r(b, c, hh, ww), z=r(b, c, hh, ww), gamma=1 + 0.3 * r(c), cbias=0.3 * r(c), mean=0.3 * r(c), var=0.5 + torch.rand(c, generator=g))


def _bn_gpu(c, ops):
    d = {k: v.to(DEV) for k, v in c.items()}
    return ops.bn_frozen_backward(d['dy'], d['z'], d['gamma'], d['cbias'], d['mean'], d['var'], 1e-5)


@pytest.mark.parametrize('b,c,hh,ww', NCASES)
def test_frozen_batch_norm_adjoint(rpe, b, c, hh, ww):
    from rpe_amd import ops
    case = _bn_case(b, c, hh, ww, 31)
    dy, z, gamma, cbias, mean, var = (case[k].double() for k in ('dy', 'z', 'gamma', 'cbias', 'mean', 'var'))
    zz, ga, cb = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), cbias.clone().requires_grad_(True)
    beta = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    y = F.batch_norm(zz + cb.view(1, c, 1, 1), mean, var, ga, beta, training=False, eps=1e-5)
    tz, tg, tbeta, tcb = torch.autograd.grad((y * dy).sum(), [zz, ga, beta, cb])
    dz, dg, dbeta, dcb = _bn_gpu(case, ops)
    again = _bn_gpu(case, ops)
    assert all(torch.equal(a, b_) for a, b_ in zip((dz, dg, dbeta, dcb), again))
    # the reductions: f64 sums rounded once (n = 2), against sum |terms| from float64
    inv = 1.0 / torch.sqrt(var + 1e-5)
    s0abs, s1abs = dy.abs().sum((0, 2, 3)), (dy.abs() * z.abs()).sum((0, 2, 3))
    for name, got, truth, tabs in (('d_beta', dbeta, tbeta, s0abs), ('d_gamma', dg, tg, (s1abs + (cbias - mean).abs() * s0abs) * inv),
                                   ('d_conv_bias', dcb, tcb, (gamma * inv).abs() * s0abs)):
        e = (got.cpu().double() - truth).abs()
        print(f'batch norm adjoint ({b},{c},{hh},{ww}) {name}: max err {float(e.max()):.3e}, max |truth| {float(truth.abs().max()):.3e}')
        assert bool((e <= 2 * U * tabs).all()), name
    assert float((dz.cpu().double() - tz).abs().max()) <= 2 * U * float(tz.abs().max()) + 1e-12
    # a NaN in dy stays inside its own channel's sums, and its own element of dz
    bad = dict(case, dy=case['dy'].clone())
    bad['dy'][0, 1, 0, 0] = float('nan')
    nz, ng, nb, ncb = _bn_gpu(bad, ops)
    keep = torch.arange(c) != 1
    for a, b_ in ((ng, dg), (nb, dbeta), (ncb, dcb)):
        assert bool(torch.isnan(a[1])) and torch.equal(a[keep.to(DEV)], b_[keep.to(DEV)])
    mask = torch.zeros(b, c, hh, ww, dtype=torch.bool)
    mask[0, 1, 0, 0] = True
    assert bool(torch.isnan(nz.cpu()[mask]).all()) and torch.equal(nz.cpu()[~mask], dz.cpu()[~mask])


@pytest.mark.parametrize('b,c,hh,ww', NCASES)
def test_instance_norm_adjoint(rpe, b, c, hh, ww):
    from rpe_amd import ops
    g = _gen(37)
    dy, z = torch.randn(b, c, hh, ww, generator=g), 0.3 + 1.7 * torch.randn(b, c, hh, ww, generator=g)
    zz = z.double().requires_grad_(True)
    tz = torch.autograd.grad((F.instance_norm(zz, eps=1e-5) * dy.double()).sum(), zz)[0]
    buf = torch.full((b, c + 4, hh, ww), 7.0, device=DEV)
    dz = ops.instnorm_backward(dy.to(DEV), z.to(DEV), 1e-5, dz=buf[:, 2:2 + c])
    assert torch.equal(dz, ops.instnorm_backward(dy.to(DEV), z.to(DEV), 1e-5))
    assert bool((buf[:, :2] == 7.0).all()) and bool((buf[:, 2 + c:] == 7.0).all())
    e = float((dz.cpu().double() - tz).abs().max())
    print(f'instance norm adjoint ({b},{c},{hh},{ww}): max err {e:.3e}, max |truth| {float(tz.abs().max()):.3e}')
    assert e <= 2 * U * float(tz.abs().max()) + 1e-12
    nd = dy.clone()
    nd[1, 2, 0, 0] = float('nan')                                        # a NaN in dy stays inside its own plane
    nz = ops.instnorm_backward(nd.to(DEV), z.to(DEV), 1e-5).cpu()
    plane = torch.zeros(b, c, dtype=torch.bool)
    plane[1, 2] = True
    assert bool(torch.isnan(nz[plane]).all()) and torch.equal(nz[~plane], dz.cpu()[~plane])


def test_split_activation_adjoint(rpe):
    from rpe_amd import ops
    g = _gen(41)
    pre, d = 1.5 * torch.randn(2, 8, 3, 5, generator=g), torch.randn(2, 8, 3, 5, generator=g)
    act = torch.cat((torch.tanh(pre[:, :3]), torch.relu(pre[:, 3:])), 1)
    truth = torch.cat((d[:, :3].double() * (1 - act[:, :3].double() ** 2), torch.where(act[:, 3:] > 0, d[:, 3:], torch.zeros(())).double()), 1)
    got = ops.split_act_backward(d.to(DEV), act.to(DEV), 3, out=torch.empty(2, 8, 3, 5, device=DEV)).cpu()
    assert float((got[:, :3].double() - truth[:, :3]).abs().max()) <= 2 * U * float(truth[:, :3].abs().max()) + 1e-12
    assert torch.equal(got[:, 3:].double(), truth[:, 3:])


# -------------------------------------------------------------------------------------------------------- one block and one encoder
def _seed_module(m, seed):
    """Weights seeded as synth.init_synthetic_weights does (default initialisers, in module order), then every batch norm's weight, bias
    and running statistics moved away from 1, 0, 0, 1 so that their gradients are exercised."""
    torch.manual_seed(seed)
    for s in m.modules():
        if isinstance(s, nn.Conv2d):
            s.reset_parameters()
        elif isinstance(s, nn.BatchNorm2d):
            s.reset_parameters()
            s.reset_running_stats()
    g = _gen(seed + 1000)
    with torch.no_grad():
        for s in m.modules():
            if isinstance(s, nn.BatchNorm2d):
                s.weight.copy_(1 + 0.2 * torch.randn(s.weight.shape, generator=g))
                s.bias.copy_(0.2 * torch.randn(s.bias.shape, generator=g))
                s.running_mean.copy_(0.2 * torch.randn(s.bias.shape, generator=g))
                s.running_var.copy_(0.7 + 0.6 * torch.rand(s.bias.shape, generator=g))
    return m.eval()


def _block_walk(blk, x, pres):
    """oracle ResidualBlock.forward with every ReLU input collected.  The last ReLU reads x + y: where that is exactly zero in a stride-1
    block both terms are ReLU outputs that are exactly zero in every precision, no decision is taken there, and those are left out."""
    p1 = blk.norm1(blk.conv1(x))
    y = torch.relu(p1)
    p2 = blk.norm2(blk.conv2(y))
    y = torch.relu(p2)
    if blk.downsample is not None:
        x = blk.downsample(x)
    p3 = x + y
    pres += [p1, p2, p3[p3 != 0]]
    return torch.relu(p3)


def _encoder_walk(enc, images, pres, split_act, raw255):
    """oracle BasicEncoder.forward, on raw 0..255 images with ``raw255`` (RAFT.forward's normalisation in front), [tanh | ReLU] behind
    with split_act."""
    p0 = enc.norm1(enc.conv1(2 * (images / 255.0) - 1.0 if raw255 else images))
    pres.append(p0)
    x = torch.relu(p0)
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for blk in layer:
            x = _block_walk(blk, x, pres)
    x = enc.conv2(x)
    if split_act:
        half = x.shape[1] // 2
        pres.append(x[:, half:])
        x = torch.cat((torch.tanh(x[:, :half]), torch.relu(x[:, half:])), 1)
    return x


def _margin(pres):
    return min(float(p.detach().abs().min()) for p in pres if p.numel())


def _reference(module, walk, dtype, order):
    """(the gradients of ``order`` and whatever else ``walk`` asks for, the ReLU margin) by autograd in ``dtype`` on a copy of ``module``."""
    import copy
    m = copy.deepcopy(module).to(dtype)
    for p in m.parameters():
        p.requires_grad_(True)
    pres = []
    loss, extra = walk(m, pres)
    grads = torch.autograd.grad(loss, order(m) + extra, allow_unused=True)
    return grads, _margin(pres)


def block_case(kind, stride, shape, seed):
    """The oracle block (64 -> 64 at stride 1, 64 -> 96 at stride 2), its input and the gradient of its output, all from ``seed``."""
    from oracle.raft import ResidualBlock
    b, hh, ww = shape
    blk = _seed_module(ResidualBlock(64, 64 if stride == 1 else 96, kind, stride), seed)
    g = _gen(seed + 2000)
    x = torch.relu(torch.randn(b, 64, hh, ww, generator=g))             # a block's input is a ReLU output
    d = torch.randn(b, blk.conv2.out_channels, _out(hh, 3) if stride == 2 else hh, _out(ww, 3) if stride == 2 else ww, generator=g)
    return blk, x, d


def block_reference(blk, x, d, dtype):
    from rpe_amd import raft_grad

    def walk(m, pres):
        xx = x.to(dtype).requires_grad_(True)
        return (_block_walk(m, xx, pres) * d.to(dtype)).sum(), [xx]
    return _reference(blk, walk, dtype, raft_grad.block_params)


def encoder_case(kind, shape, seed):
    from oracle.raft import BasicEncoder
    b, hh, ww = shape
    enc = _seed_module(BasicEncoder(output_dim=256, norm_fn=kind), seed)
    g = _gen(seed + 2000)
    # instance norm: raw 0..255 images.  Frozen batch norm does not normalise: on images in [-1, 1] these untrained weights give ReLU inputs
    # of std 0.3 - 0.5, about ten of 470 000 within 1e-5 of zero at 32 x 48, and no seed meets the margin; inputs of std 16 (raw255=False)
    # scale every layer alike (the output layer's tanh then reads values of std about 1) and leave one or two
    images = 255.0 * torch.rand(b, 3, hh, ww, generator=g) if kind == 'instance' else 16.0 * torch.randn(b, 3, hh, ww, generator=g)
    h8, w8 = hh, ww
    for _ in range(3):
        h8, w8 = _out(h8, 3), _out(w8, 3)
    return enc, images, torch.randn(b, 256, h8, w8, generator=g)


def encoder_reference(enc, images, d, split_act, raw255, dtype):
    from rpe_amd import raft_grad

    def walk(m, pres):
        return (_encoder_walk(m, images.to(dtype), pres, split_act, raw255) * d.to(dtype)).sum(), []
    return _reference(enc, walk, dtype, raft_grad.encoder_params)


# (norm kind, stride, (b, h, w) of the block's input) -> seed: the 1/2 maps of the 20 x 36, 32 x 48 and 64 x 96 images; 10 x 18 gives odd maps
# at stride 2, 32 x 48 at b = 1 takes conv_split's tuned route.  Seeds: the first from 1 whose float64 margin exceeds 1.5e-5.
BLOCK_SEEDS = {('batch', 1, (2, 10, 18)): 2, ('batch', 2, (2, 10, 18)): 5, ('batch', 2, (2, 16, 24)): 1, ('batch', 1, (1, 32, 48)): 815,
               ('batch', 2, (1, 32, 48)): 34, ('instance', 1, (2, 10, 18)): 1, ('instance', 2, (2, 10, 18)): 1, ('instance', 2, (2, 16, 24)): 3,
               ('instance', 1, (1, 32, 48)): 3, ('instance', 2, (1, 32, 48)): 2}
# (norm kind, (b, H, W) of the images) -> seed: a small one among those a search on the CPU found with a float64 margin above 1.1e-5 (about one
# seed in 1000 at 64 x 96 with instance norm, one in 5 with batch norm on its larger inputs: encoder_case)
ENCODER_SEEDS = {('batch', (2, 20, 36)): 2, ('batch', (2, 32, 48)): 2, ('batch', (1, 64, 96)): 9,
                 ('instance', (2, 20, 36)): 3, ('instance', (2, 32, 48)): 48, ('instance', (1, 64, 96)): 499}


def _to_product(oracle_module, product_module):
    product_module.load_state_dict(oracle_module.state_dict())
    return product_module.eval().to(DEV)


def _compare(tag, names, got, again, w64, w32, zeros=()):
    """``zeros``: the conv biases in front of an instance norm -- cancelled by it, exact zeros here (autograd leaves rounding noise there)."""
    missed = []
    for name, g, a, t64, t32 in zip(names, got, again, w64, w32):
        assert torch.equal(g, a), name                                  # two runs, the same bits
        if name in zeros:
            assert not bool(g.any()) and float(t64.abs().max()) < 1e-9, name
            continue
        r, r32 = ratio(g, t64), ratio(t32, t64)
        print(f'{tag} {name}: GPU {r:.3e}  float32 on the CPU {r32:.3e}  ratio {r / max(r32, 1e-300):.2f}')
        if not (bool(torch.isfinite(g).all()) and r <= 2.0 * r32):
            missed.append((name, r, r32))
    assert not missed, missed


@pytest.mark.parametrize('kind,stride,shape', list(BLOCK_SEEDS))
def test_one_block_against_float64(rpe, kind, stride, shape):
    from rpe_amd import raft, raft_grad
    blk, x, d = block_case(kind, stride, shape, BLOCK_SEEDS[kind, stride, shape])
    w64, margin = block_reference(blk, x, d, torch.float64)
    w32, _ = block_reference(blk, x, d, torch.float32)
    print(f'block {kind} stride {stride} {shape}: ReLU margin {margin:.3e}')
    assert margin > 1e-5
    mine = _to_product(blk, raft.ResidualBlock(64, blk.conv2.out_channels, kind, stride))
    run = lambda: raft_grad.residual_block_backward(mine, x.to(DEV), d.to(DEV), raft_grad._packed(raft_grad._EncoderPacked, raft_grad.block_params(mine)))
    (dx, grads), (dx2, grads2) = run(), run()
    names = [f'p{i}' for i in range(len(grads))] + ['d_x']
    assert len(grads) == len(raft_grad.block_params(mine)) and all(g.shape == p.shape for g, p in zip(grads, raft_grad.block_params(mine)))
    zeros = names[1:-1:2] if kind == 'instance' else ()                 # the conv biases cancel under the norm: exact zeros
    _compare(f'block {kind} s{stride} {shape}', names, list(grads) + [dx], list(grads2) + [dx2], w64, w32, zeros)


@pytest.mark.parametrize('kind,shape', list(ENCODER_SEEDS))
def test_one_encoder_against_float64(rpe, kind, shape):
    from rpe_amd import raft, raft_grad
    split, raw255 = kind == 'batch', kind == 'instance'                 # cnet as RAFT uses it: (tanh | ReLU) behind the output layer
    enc, images, d = encoder_case(kind, shape, ENCODER_SEEDS[kind, shape])
    w64, margin = encoder_reference(enc, images, d, split, raw255, torch.float64)
    w32, _ = encoder_reference(enc, images, d, split, raw255, torch.float32)
    print(f'encoder {kind} {shape}: ReLU margin {margin:.3e}')
    assert margin > 1e-5
    mine = _to_product(enc, raft.BasicEncoder(output_dim=256, norm_fn=kind))
    params = raft_grad.encoder_params(mine)
    given = images.to(DEV) if shape[0] == 1 else [images[:1].to(DEV), images[1:].to(DEV)]      # a list of batches, as the forward takes
    run = lambda: raft_grad.encoder_backward(mine, given, d.to(DEV), raw255=raw255, split_act=split)
    grads, grads2 = run(), run()
    assert len(grads) == len(params) == (62 if kind == 'batch' else 32) and all(g.shape == p.shape for g, p in zip(grads, params))
    names = [f'p{i}' for i in range(len(grads))]
    zeros = names[1:-2:2] if kind == 'instance' else ()                 # every conv bias in front of a norm: exact zeros (the output layer's has none behind it)
    _compare(f'encoder {kind} {shape}', names, grads, grads2, w64, w32, zeros)


# ------------------------------------------------------------------------------------------------------------------------- the chain
def _chain_truth(model, im1, im2, coords, flows, gup, dtype):
    """d loss / d (every encoder parameter) of loss = sum(flow_up * gup) by autograd in ``dtype`` through the whole model: oracle encoders,
    oracle CorrBlock sampled at the pass's (detached) coordinates, update_block_ref.step per iteration, raft_tail_ref.tail."""
    import raft_tail_ref as tref
    import update_block_ref as ubref
    from oracle.raft import BasicEncoder, CorrBlock, bilinear_sampler
    from rpe_amd import raft_grad
    encs = []
    for kind, src in (('instance', model.fnet), ('batch', model.cnet)):
        e = BasicEncoder(output_dim=256, norm_fn=kind)
        e.load_state_dict({k: v.detach().cpu() for k, v in src.state_dict().items()})
        e = e.eval().to(dtype)
        for p in e.parameters():
            p.requires_grad_(True)
        encs.append(e)
    fnet, cnet = encs
    norm = lambda im: 2 * (im.to(dtype) / 255.0) - 1.0
    f1, f2 = fnet([norm(im1), norm(im2)])
    c = cnet(norm(im1))
    net, inp = torch.tanh(c[:, :128]), torch.relu(c[:, 128:])
    Pu = {k: p.detach().cpu().to(dtype) for k, p in zip(ubref.PARAMS, model.update_params())}
    fh, mk = model.head_params()
    Pt = {k: p.detach().cpu().to(dtype) for k, p in zip(tref.PARAMS, fh + mk)}
    blk = CorrBlock(f1, f2)
    dd = torch.arange(-4, 5, dtype=dtype)
    delta = torch.stack(torch.meshgrid(dd, dd, indexing='ij'), dim=-1).view(1, 9, 9, 2)
    b, _, h8, w8 = net.shape
    for co, fl in zip(coords, flows):
        cen = co.to(dtype).permute(0, 2, 3, 1).reshape(b * h8 * w8, 1, 1, 2)
        win = [bilinear_sampler(lvl, cen / 2 ** i + delta).view(b, h8, w8, -1) for i, lvl in enumerate(blk.corr_pyramid)]
        net = ubref.step(net, inp, torch.cat(win, -1).permute(0, 3, 1, 2), fl.to(dtype), Pu)
    up = tref.tail(net, flows[-1].to(dtype), Pt)[0]
    return torch.autograd.grad((up * gup.to(dtype)).sum(), raft_grad.encoder_params(fnet) + raft_grad.encoder_params(cnet), allow_unused=True)


def test_the_chain_trains_both_encoders(rpe):
    """RAFT.forward(grad_corr=True) -> loss.backward() -> backward_encoders on a 128 x 128 pair (the smallest image whose 16 x 16 map the
    four-level correlation pyramid takes: 64 x 96 gives an 8 x 12 map, which rpe_corr_pyramid_bytes refuses), 2 iterations: every encoder parameter gets
    a finite, non-zero .grad within twice the float32 CPU figure of float64 autograd through the whole model (the leaves are taken behind
    tanh / ReLU, so a wrong side shows here); the pass's outputs and every other gradient keep their bits."""
    from rpe_amd import raft, raft_grad, synth
    model = synth.init_synthetic_weights(raft.RAFT(synth.model_config(128, 128, iters=2))).eval().to(DEV)
    g = _gen(53)
    with torch.no_grad():
        for m in model.cnet.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_((1 + 0.2 * torch.randn(m.weight.shape, generator=g)).to(DEV))
                m.bias.copy_((0.2 * torch.randn(m.bias.shape, generator=g)).to(DEV))
                m.running_mean.copy_((0.2 * torch.randn(m.bias.shape, generator=g)).to(DEV))
                m.running_var.copy_((0.7 + 0.6 * torch.rand(m.bias.shape, generator=g)).to(DEV))
    im1, im2 = (255.0 * torch.rand(1, 3, 128, 128, generator=g)).to(DEV), (255.0 * torch.rand(1, 3, 128, 128, generator=g)).to(DEV)
    gup = torch.randn(1, 2, 128, 128, generator=g).to(DEV)
    fh, mk = model.head_params()
    others = list(fh + mk + model.update_params())
    encp = raft_grad.encoder_params(model.fnet) + raft_grad.encoder_params(model.cnet)
    assert len(encp) == 94
    for p in model.parameters():
        p.requires_grad_(True)

    def run(with_encoders):
        for p in model.parameters():
            p.grad = None
        r = model(im1, im2, ret_lowres=True, grad_corr=True)
        node = r[0][-1].grad_fn
        (r[0][-1] * gup).sum().backward()
        if with_encoders:
            model.backward_encoders(im1, im2, r[6], r[7], r[4], r[5])
        return r, node, [p.grad.clone() for p in others], [None if p.grad is None else p.grad.clone() for p in encp]
    ra, node, oa, ea = run(True)
    rb, _, ob, eb = run(False)
    assert all(e is None for e in eb)
    assert torch.equal(ra[0][-1], rb[0][-1]) and all(torch.equal(a, b) for a, b in zip(ra[1:], rb[1:]))
    assert all(torch.equal(ra[i].grad, rb[i].grad) for i in (1, 4, 5, 6, 7))
    assert len(oa) == 30 and all(torch.equal(a, b) for a, b in zip(oa, ob))
    states = node.passes[0].states
    coords, flows = [co.cpu() for _, co in states], [st[:, 254:].cpu() for st, _ in states]
    w64 = _chain_truth(model, im1.cpu(), im2.cpu(), coords, flows, gup.cpu(), torch.float64)
    w32 = _chain_truth(model, im1.cpu(), im2.cpu(), coords, flows, gup.cpu(), torch.float32)
    names = [f'fnet.p{i}' for i in range(32)] + [f'cnet.p{i}' for i in range(62)]
    fnet_conv_bias = {f'fnet.p{i}' for i in range(1, 30, 2)}            # cancelled by the instance norm: exact zeros, in the truth up to rounding
    missed = []
    for name, got, t64, t32 in zip(names, ea, w64, w32):
        assert got is not None and bool(torch.isfinite(got).all()), name
        if name in fnet_conv_bias:
            assert not bool(got.any()), name
            continue
        assert float(got.abs().max()) > 0, name
        r, r32 = ratio(got, t64), ratio(t32, t64)
        print(f'chain {name}: GPU {r:.3e}  float32 on the CPU {r32:.3e}  ratio {r / max(r32, 1e-300):.2f}')
        if not r <= 2.0 * r32:
            missed.append((name, r, r32))
    assert not missed, missed
    # (the second run cleared every .grad)  the same leaves again: the same bits; once more: ADDED into .grad
    model.backward_encoders(im1, im2, ra[6], ra[7], ra[4], ra[5])
    assert all(torch.equal(p.grad, e) for p, e in zip(encp, ea))
    model.backward_encoders(im1, im2, ra[6], ra[7], ra[4], ra[5])
    assert all(torch.equal(p.grad, e + e) for p, e in zip(encp, ea))
