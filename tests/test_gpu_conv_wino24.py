"""GPU: rpe_conv_wino24 -- the 3x3 stride-1 convolutions as Winograd F(2x4,3x3) -- against the float64 convolution at the bars
tests/test_gpu_conv.py keeps for F(2x2,3x3) (its _tol, times 3 for the transforms, times 2.5 for the encoder epilogues), and its
routes against each other bit for bit: 32- and 64-channel tiles, a batch row and a batch-1 call, rpe_run_ops and the direct call."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rand(rng, *shape, s=1.0):
    return torch.from_numpy((rng.normal(size=shape) * s).astype(np.float32))


def _tol(x, w):
    k = w.shape[1] * w.shape[2] * w.shape[3]
    return 3e-6 * np.sqrt(k) * float(x.abs().max()) * float(w.abs().max()) + 1e-6


@pytest.mark.parametrize('cin,cout,h,w,b', [(256, 192, 64, 80, 2), (128, 64, 64, 80, 1), (256, 126, 44, 48, 2), (128, 256, 32, 40, 1),
                                            (8, 20, 6, 12, 3), (64, 64, 128, 160, 1), (64, 96, 20, 36, 9),
                                            (16, 96, 64, 64, 8)])     # 32 patches x 2 tiles x 8 = 512 workgroups: a 64-channel tile + the 32-channel tail launch
def test_wino24_matches_f64(rpe, cin, cout, h, w, b):
    """Bias + ReLU into channel slices with a second output; linear; the prepared launcher: F(2x2)'s bar."""
    from rpe_amd import ops
    rng = np.random.default_rng(cin + cout + 24)
    x, wt, bias = _rand(rng, b, cin, h, w), _rand(rng, cout, cin, 3, 3, s=0.05), _rand(rng, cout, s=0.5)
    assert ops.PackedWino24.supported(wt, h, w)
    pw = ops.PackedWino24(wt.cuda(), bias.cuda())
    ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
    obuf = torch.full((b, cout + 8, h, w), -7.0, device='cuda')
    o2buf = torch.full((b, cout + 4, h, w), -7.0, device='cuda')
    xbuf = torch.zeros(b, cin + 4, h, w, device='cuda')
    xbuf[:, 4:] = x.cuda()
    ops.conv_wino(xbuf[:, 4:], pw, ops.CONV_RELU, obuf[:, 4:4 + cout], out2=o2buf[:, 4:])
    got = obuf[:, 4:4 + cout].cpu().double()
    assert (got - ref.clamp_min(0)).abs().max() < 3 * _tol(x, wt)
    assert torch.equal(obuf[:, 4:4 + cout], o2buf[:, 4:])
    assert (obuf[:, :4] == -7.0).all() and (obuf[:, 4 + cout:] == -7.0).all() and (o2buf[:, :4] == -7.0).all()
    lin = ops.conv_wino(x.cuda(), pw, ops.CONV_LINEAR, torch.empty(b, cout, h, w, device='cuda')).cpu().double()
    assert (lin - ref).abs().max() < 3 * _tol(x, wt)
    out3 = torch.empty(b, cout, h, w, device='cuda')
    ops.conv_wino(x.cuda(), pw, ops.CONV_LINEAR, out3, prepare=True)()
    assert torch.equal(out3.cpu().double(), lin)


def test_wino24_refuses_what_it_cannot_do(rpe):
    from rpe_amd import ops
    with pytest.raises(rpe.RpeError):
        ops.PackedWino24(torch.zeros(8, 6, 3, 3, device='cuda'))             # cin % 4
    pw = ops.PackedWino24(torch.zeros(8, 8, 3, 3, device='cuda'))
    assert not ops.PackedWino24.supported(torch.zeros(8, 8, 3, 3), 8, 10)   # w % 4
    with pytest.raises(rpe.RpeError, match='UNSUPPORTED'):
        ops.conv_wino(torch.zeros(1, 8, 8, 10, device='cuda'), pw, ops.CONV_RELU, torch.empty(1, 8, 8, 10, device='cuda'))


@pytest.mark.parametrize('c,h,w,b', [(64, 64, 80, 3), (96, 44, 48, 2), (128, 32, 40, 2)])
def test_wino24_encoder_epilogues_match_f64(rpe, c, h, w, b):
    """Folded batch norm + ReLU + residual + ReLU; instance-norm moments consumed by rpe_instnorm_finalize / _apply; the loader-side
    relu((x - mean) / std): test_gpu_conv.py's encoder references and bars."""
    from rpe_amd import ops
    rng = np.random.default_rng(c + h + 2)
    x, wt, bias = _rand(rng, b, c, h, w), _rand(rng, c, c, 3, 3, s=0.05), _rand(rng, c, s=0.5)
    res = _rand(rng, b, c, h, w).abs()
    scale, shift = _rand(rng, c).abs() + 0.5, _rand(rng, c, s=0.3)
    pw = ops.PackedWino24(wt.cuda(), None)
    conv = F.conv2d(x.double(), wt.double(), None, padding=1)
    ref = (res.double() + (conv * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]).clamp_min(0)).clamp_min(0)
    got = ops.conv_wino(x.cuda(), pw, ops.CONV_RELU, torch.empty(b, c, h, w, device='cuda'), scale=scale.cuda(), bias=shift.cuda(), residual=res.cuda())
    assert (got.cpu().double() - ref).abs().max() < 3 * _tol(x, wt) * 2.5
    pre = conv + bias.double()[None, :, None, None]
    mean, var = pre.mean((2, 3)), pre.var((2, 3), unbiased=False)
    stats = ops.conv_wino_stats_buffer(b, c, h, w, 'cuda')
    raw = ops.conv_wino(x.cuda(), pw, ops.CONV_LINEAR, torch.empty(b, c, h, w, device='cuda'), bias=bias.cuda(), stats=stats)
    assert (raw.cpu().double() - pre).abs().max() < 3 * _tol(x, wt)
    st = stats.cpu().double()
    assert float(st[..., 0].sum(1).min()) == float(st[..., 0].sum(1).max()) == h * w
    mi = ops.instnorm_finalize(stats, h * w, eps=1e-5).cpu().double()
    assert float((mi[..., 0] - mean).abs().max()) < 1e-5 and float((mi[..., 1] * torch.sqrt(var + 1e-5) - 1).abs().max()) < 2e-5
    ref2 = (res.double() + ((pre - mean[:, :, None, None]) / torch.sqrt(var + 1e-5)[:, :, None, None]).clamp_min(0)).clamp_min(0)
    got2 = ops.instnorm_apply(raw, stats, eps=1e-5, relu=True, residual=res.cuda())
    inv = float((1 / torch.sqrt(var + 1e-5)).max())
    assert (got2.cpu().double() - ref2).abs().max() < (3 * _tol(x, wt) + 2e-6) * inv * 2
    m_i = torch.stack((_rand(rng, b, c, s=0.3), _rand(rng, b, c).abs() + 0.5), dim=-1).contiguous()
    xin = ((x.double() - m_i[..., 0].double()[:, :, None, None]) * m_i[..., 1].double()[:, :, None, None]).clamp_min(0)
    ref3 = F.conv2d(xin, wt.double(), bias.double(), padding=1)
    got3 = ops.conv_wino(x.cuda(), pw, ops.CONV_LINEAR, torch.empty(b, c, h, w, device='cuda'), bias=bias.cuda(), pre_norm=m_i.cuda())
    assert (got3.cpu().double() - ref3).abs().max() < 3 * _tol(xin.float(), wt) + 1e-5
    # moments and pre_norm together (the run-time epilogue shape)
    stats4 = ops.conv_wino_stats_buffer(b, c, h, w, 'cuda')
    got4 = ops.conv_wino(x.cuda(), pw, ops.CONV_LINEAR, torch.empty(b, c, h, w, device='cuda'), bias=bias.cuda(), pre_norm=m_i.cuda(),
                         stats=stats4, scale=torch.ones(c, device='cuda'))
    assert torch.equal(got4.cpu().double(), got3.cpu().double())
    mi4 = ops.instnorm_finalize(stats4, h * w, eps=1e-5).cpu().double()
    assert float((mi4[..., 0] - ref3.mean((2, 3))).abs().max()) < 1e-5


def test_wino24_random_shapes_against_f64(rpe):
    """Random even heights and widths % 4 (partial 16 x 8 patches on every side), channel counts and batch sizes."""
    from rpe_amd import ops
    rng = np.random.default_rng(2424)
    for _ in range(12):
        cin, cout = 4 * int(rng.integers(1, 40)), int(rng.integers(1, 200))
        h, w, b = 2 * int(rng.integers(1, 40)), 4 * int(rng.integers(1, 30)), int(rng.integers(1, 4))
        x, wt, bias = _rand(rng, b, cin, h, w), _rand(rng, cout, cin, 3, 3, s=0.05), _rand(rng, cout, s=0.5)
        pw = ops.PackedWino24(wt.cuda(), bias.cuda())
        got = ops.conv_wino(x.cuda(), pw, ops.CONV_RELU, torch.empty(b, cout, h, w, device='cuda')).cpu().double()
        ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1).clamp_min(0)
        assert (got - ref).abs().max() < 3 * _tol(x, wt), (cin, cout, h, w, b)


@pytest.mark.parametrize('cin,cout', [(256, 192), (128, 64), (256, 126), (128, 256), (64, 96)])
def test_wino24_tile_classes_and_batch_rows_agree_bitwise(rpe, cin, cout):
    """Launches below 512 workgroups run on 32-channel tiles (CB = 1), larger ones on 64-channel tiles (+ a 32-channel tail): a batch of
    16 maps equals the same maps two at a time and one at a time bit for bit, moments included."""
    from rpe_amd import ops
    rng = np.random.default_rng(cin + cout + 7)
    b, h, w = 16, 64, 80
    x, wt, bias = _rand(rng, b, cin, h, w, s=0.5).cuda(), _rand(rng, cout, cin, 3, 3, s=0.05).cuda(), _rand(rng, cout, s=0.1).cuda()
    pw = ops.PackedWino24(wt, bias)
    big = ops.conv_wino(x, pw, ops.CONV_RELU, torch.empty(b, cout, h, w, device='cuda'))
    assert 40 * -(-cout // 64) * b >= 512 > 40 * -(-cout // 64) * 2
    for i in range(0, b, 6):
        small = ops.conv_wino(x[i:i + 2].contiguous(), pw, ops.CONV_RELU, torch.empty(2, cout, h, w, device='cuda'))
        assert torch.equal(big[i:i + 2], small)
        one = ops.conv_wino(x[i:i + 1].contiguous(), pw, ops.CONV_RELU, torch.empty(1, cout, h, w, device='cuda'))
        assert torch.equal(big[i:i + 1], one)
    if cin <= 128:
        sb = ops.conv_wino_stats_buffer(b, cout, h, w, 'cuda')
        rb = ops.conv_wino(x, pw, ops.CONV_LINEAR, torch.empty(b, cout, h, w, device='cuda'), stats=sb)
        s1 = ops.conv_wino_stats_buffer(1, cout, h, w, 'cuda')
        r1 = ops.conv_wino(x[3:4].contiguous(), pw, ops.CONV_LINEAR, torch.empty(1, cout, h, w, device='cuda'), stats=s1)
        assert torch.equal(rb[3:4], r1) and torch.equal(sb.tensor[3:4], s1.tensor)


def test_wino24_launch_list_equals_direct_call(rpe):
    """rpe_run_ops with RPE_OP_CONV_WINO24 runs the same entry point: the same bits as the direct call."""
    from rpe_amd import ops, _lib
    rng = np.random.default_rng(5)
    b, cin, cout, h, w = 2, 128, 192, 32, 40
    x, wt, bias = _rand(rng, b, cin, h, w).cuda(), _rand(rng, cout, cin, 3, 3, s=0.05).cuda(), _rand(rng, cout, s=0.5).cuda()
    pw = ops.PackedWino24(wt, bias)
    direct = ops.conv_wino(x, pw, ops.CONV_RELU, torch.empty(b, cout, h, w, device='cuda'))
    out = torch.full((b, cout, h, w), -1.0, device='cuda')
    launcher = ops.conv_wino(x, pw, ops.CONV_RELU, out, prepare=True)
    assert launcher.op[0] == _lib.OP_CONV_WINO24
    lst = ops.OpList().add(launcher)
    lst.run([ops.raw_stream()])
    torch.cuda.synchronize()
    assert torch.equal(out, direct)


def test_wino24_is_no_further_from_f64_than_wino22(rpe):
    """On the update block's convc2 shape the F(2x4) error stays of the F(2x2) kernel's size (the CPU model: max 2.1e-5 vs 0.9e-5 on
    256-channel sums; here with the bar's margin)."""
    from rpe_amd import ops
    rng = np.random.default_rng(11)
    b, cin, cout, h, w = 2, 256, 192, 64, 80
    x, wt = _rand(rng, b, cin, h, w, s=2.0), _rand(rng, cout, cin, 3, 3, s=0.05)
    ref = F.conv2d(x.double(), wt.double(), None, padding=1)
    e24 = float((ops.conv_wino(x.cuda(), ops.PackedWino24(wt.cuda()), ops.CONV_LINEAR, torch.empty(b, cout, h, w, device='cuda')).cpu().double() - ref).abs().max())
    e22 = float((ops.conv_wino(x.cuda(), ops.PackedWino(wt.cuda()), ops.CONV_LINEAR, torch.empty(b, cout, h, w, device='cuda')).cpu().double() - ref).abs().max())
    assert e24 < 4 * e22 and e24 < 3 * _tol(x, wt), (e24, e22)
