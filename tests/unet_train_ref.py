"""Test infrastructure: plain torch / numpy restatement of csrc/unet_train.hip ONE STAGE AT A TIME, the per-element bounds, and the
check that holds every buffer of a forward + backward against them (tests/test_gpu_unet_train_edges.py on the GPU, the composition and
mutation tests of tests/test_unet_train_ref_cpu.py here).

``walk`` goes through the chain once.  Its modes:
  'f64'     every stage in float64, nothing rounded: the composition (== forward_ref / autograd in float64);
  'kernel'  every stage from its own float32 inputs with the kernels' arithmetic: the long sums in float64 and rounded to float32 once,
            k_t_bn_apply / k_t_head_bwd_data / k_t_resize in float32 -- the float32 CPU evaluation the checks must accept;
  'f32'     every stage in plain float32 torch ops (torch's own summation order): printed beside the GPU's figures, and NOT expected to
            meet the bounds of the long sums -- that it does not is what the f32-accumulation mutant shows;
  check     (``given`` = the buffers of a run) every stage is evaluated in float64 from the buffers ``given`` holds on its input side,
            and returns the truth and the bound for the buffer on its output side.
Discrete decisions are the kernel's own: ReLU masks and pool routing are read from the same saved float32 maps the kernel reads, the
resize taps are t_tap restated one rounded float32 operation at a time (``taps``).  Nothing has to be kept away from a tie and no element
is left out of a comparison.

Bounds, per element, u = 2^-24, e = 2^-53; none is fitted to what the GPU returns.

Long sums (convolutions, their data / weight / bias gradients, the transposed convolution and its gradients, the head, the norm's
reductions, k_t_resize_bwd).  The kernel adds k products of float32 values (exact in float64) in float64, in some fixed order, by fused
multiply-adds: every partial sum is rounded once at e, so the computed s^ has |s^ - t| <= ((1 + e)^k - 1) A <= (k + 1) e A with
A = sum |a| |b| (k e < 2^-20 here).  It is then rounded to float32: |got - s^| <= u |s^| <= u |t| + u (k + 1) e A.  Together
  |got - t| <= u |t| + (k + 2) e A.                                                                                      (``b64``)
A ReLU behind it is 1-Lipschitz: the same bound holds after it.
k_t_bn_stats.  mean^ = s^ / cnt with the sum as above: |mean^ - mean| <= dm = (cnt + 2) e sum|x| / cnt, stored with one more u.  The
second pass sums (x - mean^)^2, each difference rounded once (relative e, whatever |mean| / std is): sum (x - mean - d)^2 = m2 + cnt d^2,
so var is off by at most (cnt + 4) e var + dm^2, and invstd = 1 / sqrt(var + eps) by the relative u + (cnt + 8) e + dm^2 / (var + eps).
Running statistics: (1 - m) r + m s in float64 (three roundings) of values carrying dm, rounded to float32 once.
k_t_bn_apply (float32): fmaf(rn_mul(rn_sub(x, mean), invstd), gamma, beta) -- the difference and the product round once each, the fused
multiply-add once: |got - t| <= u |t| + ((1 + u)^3 - (1 + u)) |(x - mean) invstd gamma|.
k_t_head_bwd_data (float32): one rounded product, u |t|.
k_t_resize (float32): l0y (l0x a + l1x b) + l1y (l0x c + l1x d) with ``taps``' float32 weights: a term passes at most a product and an
addition per axis, four roundings, fewer where the compiler fuses: ((1 + u)^4 - 1) sum |w_y| |w_x| |v|.
Composites.  k_t_bn_bwd_dx writes dx over the convolution data gradient it read, and k_t_pool_bwd_add adds into the skip's share: the
intermediate z never survives.  The restatement rounds its float64 z to float32; the kernel's z^ is within the long-sum bound b of the
same truth, so |z^ - fl(z)| <= 2 b, and that uncertainty dz goes through the second stage's absolute linear map: sum dz into dbeta,
sum dz |xhat| into dgamma, |gamma invstd| dz into dx (the kernel's dx reads the float32 dgamma / dbeta it wrote to the gradient blob, and
so does the check), and dz itself into the routed sum, whose single float32 addition adds u |t| where something was added.
Sigmoid.  No accuracy of expf is documented, so no bound is derived: the output is held against the float32 CPU evaluation of the same
restatement, 1 / (1 + exp(-v)), by the yardstick rule of tests/test_gpu_unet_train.py (max|err| / max|truth| within FACTOR = 4 of the
float32 figure: another exponential and another order of the same few roundings).  Its backward needs no exponential: g y (1 - y) is two
float32 products of saved values, restated exactly.
Where an absolute sum is zero the bound is zero: the result must be exactly 0.0."""
import numpy as np
import torch
import torch.nn.functional as F

U, E = 2.0 ** -24, 2.0 ** -53
F32, F64 = torch.float32, torch.float64
WIDTHS = (16, 32, 64)
FACTOR = 4.0                        # tests/test_gpu_unet_train.py's
WCHUNK_MIN, WCHUNK_MAX_N = 4096, 32
APPLY_K = (1 + U) ** 3 - (1 + U)
RESIZE_K = (1 + U) ** 4 - 1
MUTANTS = ('tap_shift', 'crop_ceil', 'drop_last_chunk', 'pool_last_max', 'pool_odd_row', 'biased_running_var', 'dx_without_mean',
           'resize_no_clamp', 'f32_accumulation')
# the stage whose check must reject each mutant (names: the buffer a stage writes)
MUTANT_STAGE = {'tap_shift': 'skip.1', 'crop_ceil': 'r.0', 'drop_last_chunk': 'grad.0', 'pool_last_max': 'g_skip.0', 'pool_odd_row': 'g_skip.0',
                'biased_running_var': 'rv.0', 'dx_without_mean': 'g_r1.1', 'resize_no_clamp': 'out', 'f32_accumulation': 'a1.0'}


def wchunks(pixels):
    """ut_wchunks (csrc/unet_train_host.h) restated: (pixels per weight-gradient partial, number of partials)."""
    c = max((pixels + WCHUNK_MAX_N - 1) // WCHUNK_MAX_N, WCHUNK_MIN)
    c = (c + 255) // 256 * 256
    return c, (pixels + c - 1) // c


def b64(t, a, k):
    return U * t.abs() + (k + 2) * E * a


# ------------------------------------------------------------------------------------------------------------------------ forward stages
def crop(sk, uh, uw, ceil=False):
    """The centre crop of a skip map to (uh, uw) from offset floor(d / 2)."""
    dh, dw = sk.shape[-2] - uh, sk.shape[-1] - uw
    oy, ox = (-(-dh // 2), -(-dw // 2)) if ceil else (dh // 2, dw // 2)
    return sk[..., oy:oy + uh, ox:ox + uw]


def conv3(x, w, b, relu, dt=F64):
    """3x3 valid convolution of (the concatenation) x -> (t, A, k)."""
    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    t, a = F.conv2d(x, w, b), F.conv2d(x.abs(), w.abs(), b.abs())
    return (torch.relu(t) if relu else t), a, 9 * x.shape[1] + 1


def bn_stats(x, rm, rv, momentum, eps, train, dt=F64, biased=False):
    """-> dict of (t, bound): mean, invstd, rm, rv (the running statistics after the call)."""
    rm, rv = rm.to(dt), rv.to(dt)
    if not train:
        inv = 1.0 / torch.sqrt(rv + eps)
        z = torch.zeros_like(rm)
        return dict(mean=(rm, z), invstd=(inv, inv * (U + 4 * E)), rm=(rm, z), rv=(rv, z))
    x = x.to(dt)
    cnt = x.shape[0] * x.shape[2] * x.shape[3]
    mean = x.sum((0, 2, 3)) / cnt
    m2 = ((x - mean[None, :, None, None]) ** 2).sum((0, 2, 3))
    var = m2 / cnt
    inv = 1.0 / torch.sqrt(var + eps)
    dm = (cnt + 2) * E * x.abs().sum((0, 2, 3)) / cnt
    m = momentum
    rm1, rv1 = (1 - m) * rm + m * mean, (1 - m) * rv + m * (m2 / (cnt if biased else cnt - 1))
    return dict(mean=(mean, U * mean.abs() + dm), invstd=(inv, inv * (U + (cnt + 8) * E + dm ** 2 / (var + eps))),
                rm=(rm1, U * rm1.abs() + 4 * E * (((1 - m) * rm).abs() + (m * mean).abs()) + m * dm),
                rv=(rv1, U * rv1.abs() + (cnt + 8) * E * rv1.abs() + m * dm ** 2 * cnt / (cnt - 1)))


def bn_apply(x, mean, invstd, gamma, beta, relu, mode):
    v = lambda t: t[None, :, None, None]
    if mode == 'kernel':                # float32 difference and product, then the fused multiply-add
        p = (x - v(mean)) * v(invstd)
        t = (p.double() * v(gamma).double() + v(beta).double()).float()
        return (torch.relu(t) if relu else t), None
    dt = F32 if mode == 'f32' else F64
    p = (x.to(dt) - v(mean).to(dt)) * v(invstd).to(dt) * v(gamma).to(dt)
    t = p + v(beta).to(dt)
    return (torch.relu(t) if relu else t), U * t.abs() + APPLY_K * p.abs()


def pool(x):
    return F.max_pool2d(x, 2)


def upconv(x, w, b, dt=F64):
    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    return F.conv_transpose2d(x, w, b, stride=2), F.conv_transpose2d(x.abs(), w.abs(), b.abs(), stride=2), x.shape[1] + 1


def head(x, w, b, dt=F64):
    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    return F.conv2d(x, w, b), F.conv2d(x.abs(), w.abs(), b.abs()), 17


def taps(n_out, n_in, clamp=True, f32=np.float32):
    """t_tap of every output index, one rounded float32 operation at a time -> (i0, i1, l0, l1).  f32 = np.float64: torch's own taps of a
    float64 F.interpolate (the composition)."""
    scale = f32(n_in) / f32(n_out)
    f = scale * (np.arange(n_out).astype(f32) + f32(0.5)) - f32(0.5)
    f = np.where(f < 0, f32(0), f).astype(f32)
    i0 = f.astype(np.int32)
    i1 = i0 + ((i0 < n_in - 1) if clamp else 1)
    l1 = (f - i0.astype(f32)).astype(f32)
    return i0, i1.astype(np.int32), (f32(1) - l1).astype(f32), l1


def tap_matrices(n_out, n_in, clamp=True, f32=np.float32):
    """(forward (n_out, n_in + 1) float64 with each tap's two weights apart, backward the same with the two weights of a clamped tap added
    in float32 as k_t_resize_bwd does, count of outputs that read each source index).  Column n_in is what an unclamped tap reads: zeros."""
    i0, i1, l0, l1 = taps(n_out, n_in, clamp, f32)
    o = np.arange(n_out)
    wf, wb = np.zeros((n_out, n_in + 1)), np.zeros((n_out, n_in + 1), dtype=f32)
    np.add.at(wf, (o, i0), l0.astype(np.float64)); np.add.at(wf, (o, i1), l1.astype(np.float64))
    np.add.at(wb, (o, i0), l0); np.add.at(wb, (o, i1), l1)
    return torch.from_numpy(wf), torch.from_numpy(wb.astype(np.float64)), torch.from_numpy((wb != 0).sum(0).astype(np.float64))


def resize(hm, out_size, dt=F64, clamp=True, f32=np.float32):
    """Bilinear resize (align_corners=False) of (n, 1, h, w) -> (v, bound)."""
    wy, wx = tap_matrices(out_size[0], hm.shape[-2], clamp, f32)[0], tap_matrices(out_size[1], hm.shape[-1], clamp, f32)[0]
    s = F.pad(hm.to(dt), (0, 1, 0, 1))
    v = torch.einsum('Oh,nchw,Ww->ncOW', wy.to(dt), s, wx.to(dt))
    return v, RESIZE_K * torch.einsum('Oh,nchw,Ww->ncOW', wy.to(dt), s.abs(), wx.to(dt))


def sigmoid(v):
    return 1.0 / (1.0 + torch.exp(-v))


# ----------------------------------------------------------------------------------------------------------------------- backward stages
def resize_bwd(gout, out, hw, dt=F64, rounded=True, f32=np.float32):
    """k_t_resize_bwd: (t, A, k) of the head map's gradient; ``out`` (the forward's output) with the sigmoid, else None.  g y (1 - y) is
    formed in float32, two rounded products of saved values, unless ``rounded`` is off (the float64 composition)."""
    if out is not None and rounded:
        g, y = gout.numpy().astype(np.float32), out.numpy().astype(np.float32)
        g = torch.from_numpy((g * y) * (np.float32(1) - y)).to(dt)
    else:
        g = gout.to(dt) if out is None else gout.to(dt) * out.to(dt) * (1 - out.to(dt))
    (_, by, cy), (_, bx, cx) = tap_matrices(gout.shape[-2], hw[0], True, f32), tap_matrices(gout.shape[-1], hw[1], True, f32)
    by, bx = by[:, :-1].to(dt), bx[:, :-1].to(dt)
    t = torch.einsum('Oh,ncOW,Ww->nchw', by, g, bx)
    return t, torch.einsum('Oh,ncOW,Ww->nchw', by, g.abs(), bx), (cy[:-1, None] * cx[None, :-1]).max().item()


def conv3_bwd_data(dy, w, dst_hw=None, off=(0, 0), dt=F64):
    """Data gradient of the 3x3 valid convolution, placed at ``off`` in a zero map of ``dst_hw`` (the ring outside the crop) -> (t, A, k)."""
    dy, w = dy.to(dt), w.to(dt)
    t, a = F.conv_transpose2d(dy, w), F.conv_transpose2d(dy.abs(), w.abs())
    if dst_hw is not None:
        pad = (off[1], dst_hw[1] - off[1] - t.shape[-1], off[0], dst_hw[0] - off[0] - t.shape[-2])
        t, a = F.pad(t, pad), F.pad(a, pad)
    return t, a, 9 * dy.shape[1]


def conv3_bwd_wb(x, dy, dt=F64, drop_last_chunk=False):
    """Weight and bias gradients -> ((dw, A, k), (db, A, k))."""
    x, dy = x.to(dt), dy.to(dt)
    n, co, ho, wo = dy.shape
    chunk, nchunk = wchunks(n * ho * wo)
    dyw = dy
    if drop_last_chunk:
        dyw = dy.permute(1, 0, 2, 3).reshape(co, -1).clone()
        dyw[:, (nchunk - 1) * chunk:] = 0
        dyw = dyw.reshape(co, n, ho, wo).permute(1, 0, 2, 3)
    tap = lambda g, v: torch.stack([torch.stack([torch.einsum('nohw,nihw->oi', g, v[:, :, ky:ky + ho, kx:kx + wo]) for kx in range(3)], -1)
                                    for ky in range(3)], -2)
    return (tap(dyw, x), tap(dy.abs(), x.abs()), n * ho * wo + nchunk), (dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3)), n * ho * wo)


def bn_bwd(z, dz, x, relu_out, mean, invstd, gamma, train, post_mask, dgamma_dbeta=None, dt=F64, no_mean=False):
    """k_t_bn_bwd_reduce + k_t_bn_bwd_dx on the incoming gradient z (uncertain by dz) -> dict of (t, bound): dgamma, dbeta, dx.
    dgamma_dbeta: the float32 values dx reads (the run's own); None = the ones computed here."""
    v = lambda t: t.to(dt)[None, :, None, None]
    z, x = z.to(dt), x.to(dt)
    cnt = x.shape[0] * x.shape[2] * x.shape[3]
    mask = (relu_out > 0).to(dt) if relu_out is not None else torch.ones_like(z)
    g, dg = z * mask, dz * mask
    xh = (x - v(mean)) * v(invstd)
    s1, s2 = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
    b1 = U * s1.abs() + (cnt + 2) * E * g.abs().sum((0, 2, 3)) + dg.sum((0, 2, 3))
    b2 = U * s2.abs() + (cnt + 3) * E * (g * xh).abs().sum((0, 2, 3)) + (dg * xh.abs()).sum((0, 2, 3))
    dgam, dbet = dgamma_dbeta if dgamma_dbeta is not None else (s2, s1)
    gi = v(gamma) * v(invstd)
    if train:
        mb, mg = v(dbet) / cnt, v(dgam) / cnt
        dx = gi * ((g - (0 if no_mean else mb)) - xh * mg)
        bx = U * dx.abs() + 8 * E * gi.abs() * (g.abs() + mb.abs() + xh.abs() * mg.abs()) + gi.abs() * dg
    else:
        dx = g * gi
        bx = U * dx.abs() + 4 * E * dx.abs() + gi.abs() * dg
    if post_mask:
        keep = (x > 0).to(dt)
        dx, bx = dx * keep, bx * keep
    return dict(dgamma=(s2, b2), dbeta=(s1, b1), dx=(dx, bx))


def pool_route(skip, pooled, last=False, odd_row=False):
    """Where k_t_pool_bwd_add sends each window's gradient: its first maximum in row-major order, the fourth element when none compares
    equal (a NaN window).  -> index map (n, c, h, w) of the pooled pixel a skip pixel receives from, -1 for none."""
    h, w = skip.shape[-2:]
    ho, wo = h // 2, w // 2
    s = [skip[..., dy:2 * ho:2, dx:2 * wo:2] == pooled for dy in (0, 1) for dx in (0, 1)]
    if last:
        first = torch.where(s[3], 3, torch.where(s[2], 2, torch.where(s[1], 1, torch.where(s[0], 0, 3))))
    else:
        first = torch.where(s[0], 0, torch.where(s[1], 1, torch.where(s[2], 2, 3)))
    src = torch.full(skip.shape, -1, dtype=torch.long)
    idx = torch.arange(ho * wo).reshape(ho, wo).expand(first.shape)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        src[..., dy:2 * ho:2, dx:2 * wo:2] = torch.where(first == k, idx, -1)
    if odd_row and h % 2:
        src[..., h - 1, :2 * wo] = src[..., h - 2, :2 * wo]
    return src


def pool_bwd_add(share, dshare, skip, pooled, g_pool, dt=F64, **mut):
    """share (+- dshare) + the routed pooled gradient, one float32 addition where something is routed -> (t, bound)."""
    src = pool_route(skip, pooled, **mut)
    routed = torch.gather(g_pool.to(dt).flatten(-2), -1, src.clamp_min(0).flatten(-2)).reshape(src.shape)
    hit = src >= 0
    t = torch.where(hit, share + routed, share)
    return t, dshare + torch.where(hit, U * t.abs(), torch.zeros_like(t))


def upconv_bwd_data(g, w, dt=F64):
    g, w = g.to(dt), w.to(dt)
    return F.conv2d(g, w, stride=2), F.conv2d(g.abs(), w.abs(), stride=2), 4 * g.shape[1]


def upconv_bwd_w(x, g, dt=F64):
    x, g = x.to(dt), g.to(dt)
    tap = lambda v, q: torch.stack([torch.stack([torch.einsum('nihw,nohw->io', v, q[:, :, ty::2, tx::2]) for tx in (0, 1)], -1) for ty in (0, 1)], -2)
    return tap(x, g), tap(x.abs(), g.abs()), x.shape[0] * x.shape[2] * x.shape[3]


def chan_sum(g, dt=F64):
    g = g.to(dt)
    return g.sum((0, 2, 3)), g.abs().sum((0, 2, 3)), g.shape[0] * g.shape[2] * g.shape[3]


# ------------------------------------------------------------------------------------------------------------------------------ the chain
def walk(inp, mode='f64', given=None, mutant=None):
    """inp: dict x (n, cin, h8, w8), params (36, the order of csrc/unet_train_host.h), rm / rv / nbt (5 each, before the call; nbt entries may
    be None), momentum, eps (5 floats each), train_mask, out_size, sigmoid, gout.  -> {name: (value, bound or None)} for every workspace
    buffer the kernels leave ('a1.0' ..., ops.UNET_TRAIN_WS_NAMES without wpart), 'out', 'grad.0' .. 'grad.35', 'gin', 'rm.k', 'rv.k',
    'nbt.k'.  ``given`` (name -> float32 tensor of a run) switches to the check: every stage then reads its inputs from ``given``."""
    check = given is not None
    assert mutant is None or (mutant in MUTANTS and mode == 'kernel' and not check)
    mode = 'check' if check else mode
    dt = F32 if mode == 'f32' else F64
    keep = (lambda t: t) if mode in ('f64', 'check') else (lambda t: t.to(F32))
    rnd = (lambda t: t) if mode == 'f64' else (lambda t: t.to(F32).to(dt))          # the float32 rounding of an intermediate
    res = {}
    P = inp['params']
    cur = (lambda name: given[name]) if check else (lambda name: res[name][0])

    def put(name, t, bound=None):
        res[name] = (keep(t), bound)

    def long_sum(name, tak, dtl=None):
        t, a, k = tak
        put(name, t, b64(t, a, k))

    def norm(k, xname, yname, gamma, beta, relu):
        train = (inp['train_mask'] >> k) & 1
        st = bn_stats(cur(xname), inp['rm'][k], inp['rv'][k], inp['momentum'][k], inp['eps'][k], train, dt, biased=mutant == 'biased_running_var' and k == 0)
        put(f'mean.{k}', *st['mean']); put(f'invstd.{k}', *st['invstd']); put(f'rm.{k}', *st['rm']); put(f'rv.{k}', *st['rv'])
        res[f'nbt.{k}'] = (None if inp['nbt'][k] is None else int(inp['nbt'][k]) + train, None)
        put(yname, *bn_apply(cur(xname), cur(f'mean.{k}'), cur(f'invstd.{k}'), gamma, beta, relu, 'f64' if check else mode))

    x = inp['x']
    for i in range(3):
        q = P[6 * i:6 * i + 6]
        if mutant == 'f32_accumulation' and i == 0:
            put('a1.0', F.conv2d(x, q[0], q[1]))
        else:
            long_sum(f'a1.{i}', conv3(x, q[0], q[1], 0, dt))
        norm(i, f'a1.{i}', f'r1.{i}', q[2], q[3], 1)
        w2 = q[4].roll(1, -1) if mutant == 'tap_shift' and i == 1 else q[4]
        long_sum(f'skip.{i}', conv3(cur(f'r1.{i}'), w2, q[5], 0, dt))
        if i < 2:
            put(f'pool.{i}', pool(cur(f'skip.{i}')), torch.zeros(()))
            x = cur(f'pool.{i}')
    xname = 'skip.2'
    for j in range(2):
        q = P[18 + 8 * j:26 + 8 * j]
        long_sum(f'up.{j}', upconv(cur(xname), q[0], q[1], dt))
        up = cur(f'up.{j}')
        cat = torch.cat((up, crop(cur(f'skip.{1 - j}'), *up.shape[-2:], ceil=mutant == 'crop_ceil' and j == 0)), 1)
        long_sum(f'r.{j}', conv3(cat, q[2], q[3], 1, dt))
        norm(3 + j, f'r.{j}', f'nrm.{j}', q[4], q[5], 0)
        long_sum(f'dout.{j}', conv3(cur(f'nrm.{j}'), q[6], q[7], 0, dt))
        xname = f'dout.{j}'
    long_sum('hm', head(cur('dout.1'), P[34], P[35], dt))
    clamp = mutant != 'resize_no_clamp'
    ft = np.float64 if mode == 'f64' else np.float32
    v, bv = resize(cur('hm'), inp['out_size'], dt, clamp, ft)
    if inp['sigmoid']:                   # no derived bound: the check holds 'out' against 'out.f32' by the yardstick rule
        put('out', sigmoid(v))
        if check:
            res['out.f32'] = (sigmoid(resize(cur('hm'), inp['out_size'], F32)[0]), None)
    else:
        put('out', v, bv)

    # ---- backward
    gout = inp['gout']
    long_sum('g_hm', resize_bwd(gout, (cur('out') if mode == 'f64' else cur('out').to(F32)) if inp['sigmoid'] else None, cur('hm').shape[-2:], dt, mode != 'f64', ft))
    ghm = cur('g_hm')
    tw = conv3_bwd_wb  # (alias)
    t, a, k = (cur('dout.1').to(dt) * ghm.to(dt)).sum((0, 2, 3)), (cur('dout.1').to(dt) * ghm.to(dt)).abs().sum((0, 2, 3)), ghm.numel()
    put('grad.34', t.reshape(1, 16, 1, 1), b64(t, a, k).reshape(1, 16, 1, 1))
    long_sum('grad.35', chan_sum(ghm, dt))
    t = ghm.to(dt) * P[34].to(dt).reshape(1, 16, 1, 1)
    put('g_dout.1', t, U * t.abs())

    def wb(kw, x, gname, **kwargs):
        (w, b) = tw(x, cur(gname), dt, **kwargs)
        long_sum(f'grad.{kw}', w); long_sum(f'grad.{kw + 1}', b)

    def norm_bwd(k, kg, z, gname, xname, relu_name, gamma, post_mask):
        """The composite conv data gradient z -> (reduce, dx in place) -> the buffer gname; grad.kg = dgamma, grad.kg + 1 = dbeta."""
        zt, za, zk = z
        dz = 2 * b64(zt, za, zk) if mode != 'f64' else torch.zeros_like(zt)
        own = bn_bwd(rnd(zt), dz, cur(xname), cur(relu_name) if relu_name else None, cur(f'mean.{k}'), cur(f'invstd.{k}'), gamma,
                     (inp['train_mask'] >> k) & 1, post_mask, None, dt)
        put(f'grad.{kg}', *own['dgamma']); put(f'grad.{kg + 1}', *own['dbeta'])
        read = (cur(f'grad.{kg}'), cur(f'grad.{kg + 1}')) if mode != 'f64' else None
        if read is not None and not check:
            read = tuple(t.to(F32) for t in read)
        put(gname, *bn_bwd(rnd(zt), dz, cur(xname), cur(relu_name) if relu_name else None, cur(f'mean.{k}'), cur(f'invstd.{k}'), gamma,
                           (inp['train_mask'] >> k) & 1, post_mask, read, dt, no_mean=mutant == 'dx_without_mean' and k == 1)['dx'])

    share = {}
    for j in (1, 0):
        kb, si, c2 = 18 + 8 * j, 1 - j, WIDTHS[2 - j] // 2
        q = P[kb:kb + 8]
        wb(kb + 6, cur(f'nrm.{j}'), f'g_dout.{j}')
        norm_bwd(3 + j, kb + 4, conv3_bwd_data(cur(f'g_dout.{j}'), q[6], dt=dt), f'g_nrm.{j}', f'r.{j}', None, q[4], 1)
        up, sk = cur(f'up.{j}'), cur(f'skip.{si}')
        wb(kb + 2, torch.cat((up, crop(sk, *up.shape[-2:])), 1), f'g_nrm.{j}')
        long_sum(f'g_up.{j}', conv3_bwd_data(cur(f'g_nrm.{j}'), q[2][:, :c2], dt=dt))
        oy, ox = (sk.shape[-2] - up.shape[-2]) // 2, (sk.shape[-1] - up.shape[-1]) // 2
        share[si] = conv3_bwd_data(cur(f'g_nrm.{j}'), q[2][:, c2:], sk.shape[-2:], (oy, ox), dt)
        uin = 'dout.0' if j else 'skip.2'
        long_sum(f'grad.{kb}', upconv_bwd_w(cur(uin), cur(f'g_up.{j}'), dt))
        long_sum(f'grad.{kb + 1}', chan_sum(cur(f'g_up.{j}'), dt))
        long_sum('g_dout.0' if j else 'g_skip.2', upconv_bwd_data(cur(f'g_up.{j}'), q[0], dt))
    for i in (2, 1, 0):
        kb = 6 * i
        q = P[kb:kb + 6]
        wb(kb + 4, cur(f'r1.{i}'), f'g_skip.{i}')
        norm_bwd(i, kb + 2, conv3_bwd_data(cur(f'g_skip.{i}'), q[4], dt=dt), f'g_r1.{i}', f'a1.{i}', f'r1.{i}', q[2], 0)
        if i:
            wb(kb, cur(f'pool.{i - 1}'), f'g_r1.{i}')
            long_sum(f'g_pool.{i - 1}', conv3_bwd_data(cur(f'g_r1.{i}'), q[0], dt=dt))
            st, sa, sk_ = share[i - 1]
            ds = 2 * b64(st, sa, sk_) if mode != 'f64' else torch.zeros_like(st)
            mut = dict(last=mutant == 'pool_last_max' and i == 1, odd_row=mutant == 'pool_odd_row' and i == 1)
            t, b = pool_bwd_add(rnd(st), ds, cur(f'skip.{i - 1}'), cur(f'pool.{i - 1}'), cur(f'g_pool.{i - 1}'), dt, **mut)
            put(f'g_skip.{i - 1}', t, b)
            res[f'share.{i - 1}'] = (rnd(st), ds)               # (not a buffer: what the dropped rows and columns must hold)
        else:
            wb(0, inp['x'], 'g_r1.0', drop_last_chunk=mutant == 'drop_last_chunk')
            long_sum('gin', conv3_bwd_data(cur('g_r1.0'), q[0], dt=dt))
    return res


def measure(got, truth):
    """tests/test_gpu_unet_train.py's: max|got - truth| / max|truth|."""
    d, m = float((got.double() - truth.double()).abs().max()), float(truth.double().abs().max())
    return d / m if m else (0.0 if d == 0.0 else float('inf'))


def check_run(inp, given, tag='', beside=None, verbose=True):
    """Every buffer of a run (``given``: name -> CPU tensor, the names of ``walk``) against the float64 evaluation of the stage that wrote it
    from the run's own buffers, element by element.  -> ({stage: max err / bound}, [failed stages]).  A NaN truth asks for a NaN; a zero
    bound for the exact value.  ``beside``: the buffers of another evaluation (float32 on the CPU), whose figures are printed beside."""
    def figures(g):
        ref = walk(inp, given=g)
        figs, bad = {}, []
        for name, (t, bound) in ref.items():
            if name.startswith('share.') or name == 'out.f32' or t is None:
                continue
            if name.startswith('nbt.'):
                figs[name] = 0.0 if int(g[name]) == t else float('inf')
            elif bound is None:                                   # the sigmoid's output: the yardstick rule
                e, y = measure(g[name], t), measure(ref['out.f32'][0], t)
                figs[name] = e / (FACTOR * y) if y else (0.0 if e == 0 else float('inf'))
                figs[name + ' (max-norm error, float32 CPU yardstick)'] = (e, y)
            else:
                got = g[name].double().reshape(t.shape)
                nan = torch.isnan(t)
                same_nan = bool((torch.isnan(got) == nan).all())
                err = torch.where(nan, torch.zeros_like(t), (got - t).abs())
                bound = torch.where(nan, torch.zeros_like(t), bound.expand(t.shape))
                ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float('inf')).double())
                figs[name] = float(ratio.max()) if same_nan else float('inf')
            if not figs[name] <= 1.0:
                bad.append(name)
        return figs, bad
    figs, bad = figures(given)
    other = figures(beside)[0] if beside is not None else {}
    if verbose:
        for name, f in figs.items():
            if isinstance(f, tuple):
                print(f'{tag} {name}: {f[0]:.3e} {f[1]:.3e}')
            else:
                print(f'{tag} {name:10s} max err / bound {f:9.3f}' + (f'   float32 on the CPU {other[name]:12.3f}' if name in other else ''))
    return figs, bad


def buffers(res):
    """The values of a ``walk`` as the float32 buffers of a run."""
    return {k: (v if not torch.is_tensor(v) else v.to(F32)) for k, (v, _) in res.items() if not k.startswith('share.')}


# ------------------------------------------------------------------------------------------------------------------------------- inputs
def norms_of(net):
    return [st.norm for st in list(net.encoder.enc_blocks) + list(net.decoder.dec_blocks)]


def inputs_of(net, x, gout, sigmoid=False, float32_constants=True, count=False):
    """``walk``'s inputs from a TinyUNet on the CPU (its norms' train / eval state gives the mask).  float32_constants: momentum and eps as
    the library receives them (C floats); off for the comparison with torch's float64 F.batch_norm, which takes the Python doubles."""
    from rpe_amd import unet
    cst = (lambda v: float(np.float32(v))) if float32_constants else float
    ns = norms_of(net)
    return dict(x=x.detach().float(), params=[p.detach().float() for p in unet.train_params(net)],
                rm=[n.running_mean.detach().clone().float() for n in ns], rv=[n.running_var.detach().clone().float() for n in ns],
                nbt=[int(n.num_batches_tracked) if count else None for n in ns], momentum=[cst(n.momentum) for n in ns],
                eps=[cst(n.eps) for n in ns], train_mask=sum(int(n.training) << k for k, n in enumerate(ns)), out_size=tuple(net.out_sz),
                sigmoid=bool(sigmoid), gout=gout.detach().float())


def plant_ties(x, size=14):
    """x with every channel constant over its top-left size x size corner: stage 0's skip map is then bitwise constant over the corner's
    (size - 4)^2 pixels (every pixel there adds the same terms in the same order), and each pool window inside it is a four-way tie."""
    x = x.clone()
    x[..., :size, :size] = x[..., :1, :1]
    return x
