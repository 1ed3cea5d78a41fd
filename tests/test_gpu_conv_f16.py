"""GPU: rpe_conv_f16 (csrc/conv_f16.hip) -- rpe_conv_fused's operation with fp16 operands on the 16-bit matrix cores.

Reference: the FLOAT64 convolution of the fp16-ROUNDED operands with rpe_conv_fused's epilogues (tests/conv_f16_ref.py); kernel and
reference differ by f32 accumulation only, so the bar is the direct f32 kernel's own, test_gpu_conv._tol, on the rounded operands (plus, for
tanh and the gates, the slack test_gpu_conv.py gives the f32 kernels' hardware exp / reciprocal).  Shapes are the smallest at which the
kernel takes each of its paths: one K step / a K tail, 64- and 128-channel tiles with ragged last tiles, maps smaller than, equal to and
not a multiple of the 16 x 8 pixel patch, all four kernel shapes."""
import ctypes

import numpy as np
import pytest
import torch

import conv_f16_ref as ref
from test_gpu_conv import _rand, _tol

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _run(ops, x, wt, bias, mode=0, pad_ch=(3, 4), **kw):
    """conv_fused with a PackedConvF16 on channel slices of larger buffers filled with -7 -> (out, out2, the two buffers, their slices)."""
    b, cin, h, w = x.shape
    cout = wt.shape[0]
    xbuf = torch.full((b, cin + pad_ch[0] + 4, h, w), float('nan'), device=DEV)
    xbuf[:, pad_ch[0]:pad_ch[0] + cin] = x.to(DEV)
    obuf, o2buf = torch.full((b, cout + pad_ch[1] + 1, h, w), -7.0, device=DEV), torch.full((b, cout + 2, h, w), -7.0, device=DEV)
    pc = ops.PackedConvF16(wt.to(DEV), None if bias is None else bias.to(DEV))
    ops.conv_fused(xbuf[:, pad_ch[0]:pad_ch[0] + cin], pc, mode, obuf[:, pad_ch[1]:pad_ch[1] + cout], out2=o2buf[:, 2:], **kw)
    return obuf[:, pad_ch[1]:pad_ch[1] + cout], o2buf[:, 2:], obuf, pc


SHAPES = [(16, 20, 3, 3, 6, 12, 3),        # one K step (half of it zero channels), ragged cout on a 64-channel tile
          (324, 256, 1, 1, 8, 12, 2),      # convc1: a K tail of 4 channels
          (256, 126, 3, 3, 10, 12, 2),     # conv: ragged cout on a 128-channel tile, two patch rows
          (128, 64, 3, 3, 44, 48, 1),      # convf2: a map that is not a whole number of 16 x 8 patches
          (256, 576, 1, 1, 6, 8, 1),       # the mask head's output layer: nine 64-channel tiles
          (128, 256, 3, 3, 4, 8, 1),       # a map smaller than one patch
          (256, 256, 1, 5, 6, 12, 2),      # convz1 | convr1
          (256, 128, 5, 1, 6, 12, 2)]      # convq2


@pytest.mark.parametrize('cin,cout,kh,kw,h,w,b', SHAPES)
def test_matches_f64_of_the_rounded_operands(rpe, cin, cout, kh, kw, h, w, b):
    from rpe_amd import ops
    rng = np.random.default_rng(cin + cout + kh * 7 + kw)
    x, wt, bias = _rand(rng, b, cin, h, w), _rand(rng, cout, cin, kh, kw, s=0.05), _rand(rng, cout, s=0.1)
    want = ref.conv_ref(x, wt, bias)[0]
    out, out2, obuf, _ = _run(ops, x, wt, bias)
    bar = _tol(ref.round_h(x), ref.round_h(wt))
    err = float((out.cpu().double() - want).abs().max())
    print(f'({cin},{cout},{kh}x{kw},{h}x{w},{b}): max error {err:.3e}, bar {bar:.3e}')
    assert err < bar
    assert torch.equal(out, out2)
    assert (obuf[:, :4] == -7.0).all() and (obuf[:, 4 + cout:] == -7.0).all()            # neighbours untouched
    if (cin, cout) == (256, 126):
        # the operands really are fp16: the result is farther than the bar from the f64 convolution of the operands as they are
        far = float((out.cpu().double() - ref.conv_ref(x, wt, bias, rounded=False)[0]).abs().max())
        print(f'    against the unrounded operands: {far:.3e}')
        assert far > bar


def test_rounding_is_to_nearest_even_bit_for_bit(rpe):
    """A 1x1 identity layer returns its input rounded to fp16.  Ties with an even and with an odd kept bit, the f32 neighbours of ties,
    +-65504, the last f32 below 65520, +-0 and the fp16 normal minima come back as x.half().float() exactly.  65520 is the first value
    that becomes Inf: its own channel must hold +-Inf exactly, and -- IEEE's 0 * Inf, SPECIAL VALUES in rpe.h -- the identity's zero
    weights turn the OTHER channels of that pixel into NaN, so those two pixels are checked against that and the rest against
    x.half().float().  No subnormals here."""
    from rpe_amd import ops
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    u = 2.0 ** -10                                                           # fp16 spacing in [1, 2)
    ties = torch.stack([f(1 + u / 2), f(1 + 3 * u / 2), f(1.5 + u / 2), f(1.5 + 3 * u / 2), f(-(1 + u / 2)), f(-(1 + 3 * u / 2)), f(1024 + 0.5), f(1024 + 1.5),
                        f(2.0 ** -14 * (1 + u / 2)), f(2.0 ** -14 * (1 + 3 * u / 2)), f(65504 - 16), f(-(65504 - 16))])
    assert torch.equal(ties.half().float()[:4], torch.tensor([1.0, 1 + 2 * u, 1.5, 1.5 + 2 * u]))     # both parities, as the reference rounds them
    near = torch.cat([torch.nextafter(ties, f(float('inf')).expand_as(ties)), torch.nextafter(ties, f(float('-inf')).expand_as(ties))])
    edge = f([65504.0, -65504.0, 65519.996, -65519.996, 0.0, -0.0, 2.0 ** -14, -(2.0 ** -14), 1.0, -2.5, 3.0e-4, 7.0])
    vals = torch.cat([ties, near, edge])
    assert bool(((vals.abs() >= 2.0 ** -14) | (vals == 0)).all()) and bool(torch.isfinite(vals.half().float()).all())
    n = 16 * 4 * 8
    x = vals.repeat(-(-n // vals.numel()))[:n].reshape(1, 16, 4, 8).clone()
    x[0, 3, 1, 2], x[0, 9, 2, 5] = 65520.0, -65520.0
    eye = torch.eye(16).reshape(16, 16, 1, 1)
    out = torch.empty(1, 16, 4, 8, device=DEV)
    ops.conv_fused(x.to(DEV), ops.PackedConvF16(eye.to(DEV)), ops.CONV_LINEAR, out)
    out, want = out.cpu(), x.half().float()
    assert want[0, 3, 1, 2] == float('inf') and want[0, 9, 2, 5] == float('-inf')
    assert out[0, 3, 1, 2] == float('inf') and out[0, 9, 2, 5] == float('-inf')
    for c, (py, px) in ((3, (1, 2)), (9, (2, 5))):
        others = torch.arange(16) != c
        assert bool(torch.isnan(out[0, others, py, px]).all())
        out[0, :, py, px] = want[0, :, py, px]
    assert torch.equal(out, want)
    assert bool((out != x)[x == x].any())                                     # (the input was not representable: something was rounded)


@pytest.mark.parametrize('mode,slack', [(ref.LINEAR, 0.0), (ref.RELU, 0.0), (ref.TANH, 1e-6)])
def test_plain_modes_with_a_second_output(rpe, mode, slack):
    from rpe_amd import ops
    rng = np.random.default_rng(40 + mode)
    x, wt, bias, add = _rand(rng, 2, 48, 10, 20), _rand(rng, 72, 48, 3, 3, s=0.05), _rand(rng, 72, s=0.1), _rand(rng, 2, 72, 10, 20, s=0.3)
    out, out2, obuf, _ = _run(ops, x, wt, bias, mode, add=add.to(DEV))
    want = ref.conv_ref(x, wt, bias, add=add, mode=mode)[0]
    assert float((out.cpu().double() - want).abs().max()) < _tol(ref.round_h(x), ref.round_h(wt)) + slack
    assert torch.equal(out, out2) and (obuf[:, :4] == -7.0).all() and (obuf[:, 4 + 72:] == -7.0).all()


@pytest.mark.parametrize('kh,kw,h,w', [(1, 5, 10, 20), (5, 1, 10, 20)])
def test_gru_half_step_matches_f64(rpe, kh, kw, h, w):
    """z, r*h and the blended hidden state of one SepConvGRU half with the gates in the epilogue (``add``, ``hidden``, ``zgate``, ``out``
    aliasing ``hidden``), with test_gpu_conv.test_gru_half_step_matches_f64's slack for the f32 kernels' gate arithmetic."""
    from rpe_amd import ops
    c, b = 32, 2
    rng = np.random.default_rng(kh * 10 + kw)
    hx = _rand(rng, b, 2 * c, h, w, s=0.5)
    wzr, bzr, azr = _rand(rng, 2 * c, 2 * c, kh, kw, s=0.03), _rand(rng, 2 * c, s=0.1), _rand(rng, b, 2 * c, h, w, s=0.3)
    wq, bq, aq = _rand(rng, c, 2 * c, kh, kw, s=0.03), _rand(rng, c, s=0.1), _rand(rng, b, c, h, w, s=0.3)
    g_hx, g_rhx, g_z = hx.to(DEV), hx.to(DEV).clone(), torch.empty(b, c, h, w, device=DEV)
    pzr, pq = ops.PackedConvF16(wzr.to(DEV), bzr.to(DEV)), ops.PackedConvF16(wq.to(DEV), bq.to(DEV))
    ops.conv_wino1d(g_hx, pzr, ops.CONV_GATE_ZR, g_z, out2=g_rhx[:, :c], add=azr.to(DEV), hidden=g_hx[:, :c], gate_channels=c)
    z, rh = ref.conv_ref(hx, wzr, bzr, add=azr, mode=ref.GATE_ZR, hidden=hx, gate_channels=c)
    tz = _tol(ref.round_h(hx), ref.round_h(wzr)) * 0.25 + 2e-7
    assert float((g_z.cpu().double() - z).abs().max()) < tz
    assert float((g_rhx[:, :c].cpu().double() - rh).abs().max()) < tz * float(hx.abs().max())
    assert torch.equal(g_rhx[:, c:], g_hx[:, c:])
    rhx_seen, z_seen = g_rhx.cpu(), g_z.cpu()                                 # the q convolution reads the f32 r*h and z the kernel stored
    ops.conv_wino1d(g_rhx, pq, ops.CONV_GATE_H, g_hx[:, :c], add=aq.to(DEV), hidden=g_hx[:, :c], zgate=g_z)   # in place on h
    hnew = ref.conv_ref(rhx_seen, wq, bq, add=aq, mode=ref.GATE_H, hidden=hx, zgate=z_seen)[0]
    assert float((g_hx[:, :c].cpu().double() - hnew).abs().max()) < _tol(ref.round_h(rhx_seen), ref.round_h(wq)) + tz * 2
    assert torch.equal(g_hx[:, c:].cpu(), hx[:, c:])


def test_launcher_list_and_repeat_give_the_same_bits(rpe):
    from rpe_amd import _lib, ops
    rng = np.random.default_rng(7)
    x, wt, bias = _rand(rng, 2, 40, 6, 12).to(DEV), _rand(rng, 24, 40, 3, 3, s=0.05).to(DEV), _rand(rng, 24, s=0.1).to(DEV)
    pc = ops.PackedConvF16(wt, bias)
    fresh = lambda: torch.full((2, 30, 6, 12), -7.0, device=DEV)
    a, b2, c, d, e = fresh(), fresh(), fresh(), fresh(), fresh()
    ops.conv_fused(x, pc, ops.CONV_RELU, a[:, 3:27])
    ops.conv_wino(x, pc, ops.CONV_RELU, b2[:, 3:27])                          # conv_wino runs the kernel that belongs to the packing
    launch = ops.conv_fused(x, pc, ops.CONV_RELU, c[:, 3:27], prepare=True)
    assert launch.op[0] == _lib.OP_CONV_F16 and bool((c == -7.0).all())
    launch()
    ops.OpList().add(ops.conv_fused(x, pc, ops.CONV_RELU, d[:, 3:27], prepare=True)).run((ops.raw_stream(),))
    rec = ops.Recorder()
    with rec:
        ops.conv_fused(x, pc, ops.CONV_RELU, e[:, 3:27])
    assert rec.complete and [k for k, _, _ in rec._items] == [_lib.OP_CONV_F16]
    first = e.clone()
    e.fill_(-7.0)
    rec.run((ops.raw_stream(),))
    for other in (b2, c, d, e, first):
        assert torch.equal(a, other)
    assert bool((a[:, :3] == -7.0).all()) and bool((a[:, 27:] == -7.0).all()) and bool((a[:, 3:27] >= 0).all())
    # a 1x1 layer through Conv1x1: rpe_conv_f16 at every launch size when asked for it
    w1 = _rand(rng, 24, 40, 1, 1, s=0.05).to(DEV)
    o1, o2 = torch.empty(2, 24, 6, 12, device=DEV), torch.empty(2, 24, 6, 12, device=DEV)
    with _lib.CountingLib() as count:
        ops.Conv1x1(w1, bias)(x, ops.CONV_LINEAR, o1, f16=True)
    assert count.names == ['rpe_conv_f16_pack', 'rpe_conv_f16']
    ops.conv1x1(x, ops.PackedConvF16(w1, bias), ops.CONV_LINEAR, o2)
    assert torch.equal(o1, o2)


@pytest.mark.parametrize('layer', ['3x3', 'gate'])
def test_a_row_does_not_depend_on_its_batch(rpe, layer):
    from rpe_amd import ops
    rng = np.random.default_rng(11)
    c, h, w = 32, 10, 20
    x = _rand(rng, 3, 2 * c, h, w, s=0.5).to(DEV)
    if layer == '3x3':
        pc = ops.PackedConvF16(_rand(rng, 72, 2 * c, 3, 3, s=0.05).to(DEV), _rand(rng, 72, s=0.1).to(DEV))
        run = lambda xs: ops.conv_fused(xs, pc, ops.CONV_RELU, torch.empty(xs.shape[0], 72, h, w, device=DEV))
    else:
        pc = ops.PackedConvF16(_rand(rng, c, 2 * c, 1, 5, s=0.03).to(DEV))
        add, z = _rand(rng, 3, c, h, w, s=0.3).to(DEV), torch.rand(3, c, h, w, device=DEV)
        rows = {}

        def run(xs):
            i = rows.get('i')
            sl = slice(None) if i is None else slice(i, i + 1)
            return ops.conv_fused(xs, pc, ops.CONV_GATE_H, torch.empty(xs.shape[0], c, h, w, device=DEV), add=add[sl], hidden=x[sl, :c], zgate=z[sl])
    whole = run(x)
    for i in range(3):
        if layer == 'gate':
            rows['i'] = i
        assert torch.equal(run(x[i:i + 1]), whole[i:i + 1]), i


def test_k_tail_is_staged_as_zero_and_never_read(rpe):
    """cin = 324 as a slice of a 328-channel buffer whose last 4 channels are NaN: the last K step's channels 324 .. 351 are zero weights
    against channels the kernel must not read -- no NaN comes out.  A NaN INSIDE the slice reaches exactly its receptive field."""
    from rpe_amd import ops
    rng = np.random.default_rng(3)
    b, cin, cout, h, w = 1, 324, 40, 10, 20
    buf = torch.full((b, 328, h, w), float('nan'), device=DEV)
    buf[:, :cin] = _rand(rng, b, cin, h, w).to(DEV)
    for k in ((1, 1), (3, 3)):
        pc = ops.PackedConvF16(_rand(rng, cout, cin, *k, s=0.05).to(DEV))
        out = ops.conv_fused(buf[:, :cin], pc, ops.CONV_LINEAR, torch.empty(b, cout, h, w, device=DEV))
        assert not bool(torch.isnan(out).any()), k
        x2 = buf.clone()
        x2[0, 323, 4, 7] = float('nan')
        out = ops.conv_fused(x2[:, :cin], pc, ops.CONV_LINEAR, torch.empty(b, cout, h, w, device=DEV))
        want = torch.zeros(b, cout, h, w, dtype=torch.bool)
        r = k[0] // 2
        want[:, :, 4 - r:4 + r + 1, 7 - r:7 + r + 1] = True
        assert torch.equal(torch.isnan(out).cpu(), want), k


def test_refusals(rpe):
    from rpe_amd import ops
    L = rpe.lib()
    assert L.rpe_conv_f16_packed_bytes(64, 64, 7, 7) == 0
    with pytest.raises(rpe.RpeError):
        ops.PackedConvF16(torch.zeros(8, 8, 7, 7, device=DEV))
    assert not ops.PackedConvF16.supported(torch.zeros(8, 8, 3, 3), 8, 10) and ops.PackedConvF16.supported(torch.zeros(8, 8, 3, 3), 8, 12)
    wt = torch.zeros(8, 8, 3, 3, device=DEV)
    pc = ops.PackedConvF16(wt)
    x, out = torch.zeros(1, 8, 8, 12, device=DEV), torch.empty(1, 8, 8, 12, device=DEV)
    ops.conv_fused(x, pc, ops.CONV_LINEAR, out)
    bad = lambda **kw: pytest.raises(rpe.RpeError, match='rpe_conv_f16 failed with RPE_E_UNSUPPORTED')
    with bad():
        ops.conv_fused(torch.zeros(1, 8, 8, 10, device=DEV), pc, ops.CONV_LINEAR, torch.empty(1, 8, 8, 10, device=DEV))          # w = 10
    with bad():
        ops.conv_fused(torch.zeros(8 * 8 * 12 + 1, device=DEV)[1:].view(1, 8, 8, 12), pc, ops.CONV_LINEAR, out)                      # misaligned slice
    with bad():
        ops.conv_fused(x, pc, ops.CONV_LINEAR, torch.empty(1, 8, 4, 6, device=DEV), stride=2)
    with bad():
        ops.conv_fused(x, pc, ops.CONV_LINEAR, out, scale=torch.ones(8, device=DEV))
    with bad():
        ops.conv_fused(x, pc, ops.CONV_LINEAR, out, residual=torch.zeros(1, 8, 8, 12, device=DEV))
    with bad():
        ops.conv_fused(x, pc, ops.CONV_LINEAR, out, stats=ops.conv_stats_buffer(1, 8, 8, 12, DEV))
    with bad():
        ops.conv_fused(x, pc, ops.CONV_LINEAR, out, pre_norm=torch.zeros(1, 8, 2, device=DEV))
    with pytest.raises(rpe.RpeError, match='valid-extent'):
        ops.conv_fused(x, pc, ops.CONV_LINEAR, out, valid=(8, 12))
