"""GPU: the fused weight heads (csrc/unet.hip: rpe_unet_heads -- both TinyUNets, bilinear resize, sigmoid) at the grids and inputs where
the chain could be wrong without tests/test_gpu_unet.py noticing, against the float64 forward of tests/unet_ref.py (whose own
properties tests/test_unet_ref_cpu.py checks without a GPU).

Tolerance rule (every comparison with the truth here, ``unet_ref.bar``): max|p_hip - p_f64| over a head's weight maps must stay within
4x the same measure of the float32 CPU forward, the yardstick being floored at 2^-23 (one float32 spacing on [0.5, 1)).  Both errors and
their ratio are printed.  The heads' convolution weights carry a gain of 2 so that the logits span 2 to 5 units instead of 0.1.

What the cases are for:
  * 45x47, 46x52, 47x44: 1/8 grids that are not multiples of 4, where the reference raises in torch.cat and the chain crops the skip at
    floor(d / 2) -- 45x47 pools 41x43 maps (last row and column pooled by nothing), 46x52 and 47x44 have odd crop differences with
    dh != dw.  On grids that are multiples of 4 a ceil(d / 2) crop is the same function (test_unet_ref_cpu.py).
  * output sizes other than 8x the grid; a batch large enough to switch the first stage's kernels; guard bytes around the workspace and
    both outputs; NaN, which torch's max pool propagates.
Not covered: the ``aligned == false`` branch of k_u_conv3 (a source whose channel count is not a multiple of 8) cannot be reached through
the C ABI -- every source rpe_unet_heads builds has 8, 16, 32, 64 or 128 channels -- and is left alone."""
import copy
import ctypes
import functools

import pytest
import torch

import unet_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 4096


@functools.lru_cache(maxsize=None)
def _blobs(h8, w8, b):
    """The packed parameter blobs of a case's two heads, on the GPU."""
    from rpe_amd import unet
    return tuple(unet.pack_params(copy.deepcopy(n).cuda()) for n in ref.case(h8, w8, b)['nets'])


def run_hip(c, blobs, out_size, rows=slice(None)):
    from rpe_amd import ops
    hc = c['hc'][rows].cuda()
    return ops.unet_heads(c['inp1'][rows].cuda(), c['inp2'][rows].cuda(), hc[:, :128], hc[:, 128:], blobs[0], blobs[1], out_size)


def check_against_truth(got, truth, yard, what, where=None):
    """Both heads within the bar (over ``where``, a mask, if given); prints hip error, float32 CPU error and their ratio."""
    bad = []
    for hd in range(2):
        g, t, y = got[hd].cpu().double(), truth[hd][1], yard[hd][1]
        assert g.shape == t.shape
        if where is not None:
            g, t, y = g[where[hd]], t[where[hd]], y[where[hd]]
        e, f, bar = float((g - t).abs().max()), float((y.double() - t).abs().max()), ref.bar(t, y)
        print(f'{what} head {hd}: hip {e:.3e}   f32 cpu {f:.3e}   hip / f32 cpu {e / f:.2f}   bar {bar:.3e}')
        if not e <= bar:
            bad.append((hd, e, bar))
    assert not bad, bad


@pytest.mark.parametrize('h8,w8,b', list(ref.PARITY_CASES))
def test_weight_maps_match_float64(rpe, h8, w8, b):
    c = ref.case(h8, w8, b)
    got = run_hip(c, _blobs(h8, w8, b), (8 * h8, 8 * w8))
    assert got[0].shape == got[1].shape == (b, 1, 8 * h8, 8 * w8)
    check_against_truth(got, c['f64'], c['f32'], f'{h8}x{w8} b={b}')


@pytest.mark.parametrize('out_size', [(100, 37), (371, 419), (100, 7)])
def test_resize_away_from_eight_times_the_grid(rpe, out_size):
    """The 46x52 grid ends in a 4x12 head map: (100, 37) and (371, 419) are fractional up-samplings (x25 / x3.08, x92.75 / x34.9),
    (100, 7) down-samples the columns.  Truth: forward_ref (F.interpolate of the head map) at the same size; row 0 of the parity case."""
    c = ref.case(46, 52, 2)
    xs = [x[:1] for x in c['xs']]
    truth, yard = (ref.run_cpu(c['nets'], xs, dt, out_size=out_size) for dt in (torch.float64, torch.float32))
    got = run_hip(c, _blobs(46, 52, 2), out_size, rows=slice(0, 1))
    assert got[0].shape == (1, 1) + out_size
    check_against_truth(got, truth, yard, f'46x52 -> {out_size[0]}x{out_size[1]}')


def test_rows_do_not_depend_on_the_batch_at_a_small_grid(rpe):
    """46x52, batch 32 against rows launched alone (1 row) and in threes.  launch_conv3 runs a layer on 4-channel threads when
    tiles * (cout / 16) * 2b < U_CONV3_MIN_WG = 512 and on 16-channel threads otherwise.  First stage (cout = 16): conv1 writes 44 x 50 =
    2200 pixels = 9 tiles of 256, conv2 42 x 48 = 2016 = 8 tiles; at b = 32 that is 9 * 64 = 576 and 8 * 64 = 512 workgroups -> 16-channel
    threads, at b = 1 and 3 at most 9 * 6 = 54 -> 4-channel threads.  Every later layer has at most 2 tiles x 2 channel groups x 64 = 256
    and stays on 4-channel threads at all three batches.  If U_CONV3_MIN_WG changes, move the batch so that the first stage still switches."""
    from rpe_amd import ops
    h8, w8, b = 46, 52, 32
    blobs = _blobs(h8, w8, 2)
    g = torch.Generator().manual_seed(7)
    i1, i2, hc = (torch.randn(b, ch, h8, w8, generator=g).cuda() for ch in (8, 8, 256))
    full = ops.unet_heads(i1, i2, hc[:, :128], hc[:, 128:], blobs[0], blobs[1], (8 * h8, 8 * w8))
    assert bool(torch.isfinite(full[0]).all()) and float(full[0].max() - full[0].min()) > 0.1
    for sl in (slice(0, 1), slice(7, 10)):
        part = ops.unet_heads(i1[sl].contiguous(), i2[sl].contiguous(), hc[sl, :128], hc[sl, 128:], blobs[0], blobs[1], (8 * h8, 8 * w8))
        assert torch.equal(part[0], full[0][sl]) and torch.equal(part[1], full[1][sl])


def _guarded(nbytes, offset=0):
    """A region of ``nbytes`` bytes, ``offset`` bytes past a 256-byte boundary, with GUARD pattern bytes before and behind it."""
    big = torch.full((GUARD + offset + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    assert big.data_ptr() % 256 == 0
    return big, big[GUARD + offset:GUARD + offset + nbytes]


def _guards_intact(big, nbytes, offset=0):
    lo, hi = big[:GUARD + offset], big[GUARD + offset + nbytes:]
    return hi.numel() == GUARD and bool((lo == 0xA5).all()) and bool((hi == 0xA5).all())


@pytest.mark.parametrize('h8,w8,b,ws_offset', [(45, 47, 2, 0), (46, 52, 3, 0), (45, 47, 2, 4)])
def test_chain_stays_inside_its_workspace_and_outputs(rpe, h8, w8, b, ws_offset):
    """rpe_unet_heads through the raw library handle: the workspace is exactly rpe_unet_workspace_bytes(b, h8, w8) bytes in the middle of
    a larger tensor, both outputs the middles of larger tensors, 4096 pattern bytes on every side -- all of it allocated, so a stray
    write lands in a guard and is seen.  The reported size includes 256 bytes for the library's own round-up of the base: the third
    case hands over a base 4 bytes past a 256-byte boundary.  The workspace starts as NaN bytes: scratch read before it is written
    would show in the outputs, which must be those of ops.unet_heads bit for bit."""
    from rpe_amd import _lib
    L = rpe.lib()
    c = ref.case(h8, w8, b)
    blobs = _blobs(h8, w8, b)
    H, W = 8 * h8, 8 * w8
    want = run_hip(c, blobs, (H, W))
    nws = L.rpe_unet_workspace_bytes(b, h8, w8)
    assert nws > 256
    ws_big, ws = _guarded(nws, ws_offset)
    ws.fill_(0xFF)
    assert ws.data_ptr() % 256 == ws_offset
    outs = [_guarded(b * H * W * 4) for _ in range(2)]
    i1, i2, hc = c['inp1'].cuda(), c['inp2'].cuda(), c['hc'].cuda()
    ctx = hc[:, 128:]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(L.rpe_unet_heads(vp(i1), vp(i2), vp(hc), vp(ctx), hc.stride(0), ctx.stride(0), vp(blobs[0]), vp(blobs[1]), b, h8, w8, H, W,
                                vp(outs[0][1]), vp(outs[1][1]), vp(ws), _lib.stream_ptr()), 'rpe_unet_heads')
    torch.cuda.synchronize()
    assert _guards_intact(ws_big, nws, ws_offset)
    for (big, mid), w in zip(outs, want):
        assert _guards_intact(big, b * H * W * 4)
        assert torch.equal(mid.view(torch.float32).view(b, 1, H, W), w)


@pytest.mark.parametrize('at', ref.NAN_AT, ids=['through-the-pools-only', 'inside-the-crops'])
def test_nan_propagates_as_in_torch(rpe, at):
    """hidden[0, 100, 2, 2] = NaN lies outside both skip crops and reaches the output only through the 2x2 max pools, which propagate NaN
    in torch (and in the reference, whose pose a NaN poisons); hidden[0, 100, 23, 26] travels through the skips as well.  The NaN pixels
    are exactly those of the float32 forward_ref, the finite pixels of that row are within the bar, the other row is untouched."""
    h8, w8, b = ref.NAN_GRID
    c, clean = ref.case(h8, w8, b, nan_at=at), ref.case(h8, w8, b)
    got = run_hip(c, _blobs(h8, w8, b), (8 * h8, 8 * w8))
    got_clean = run_hip(clean, _blobs(h8, w8, b), (8 * h8, 8 * w8))
    masks = [c['f32'][hd][1].isnan() for hd in range(2)]
    for hd in range(2):
        n_hip = int(got[hd].isnan().sum())
        print(f'NaN at hidden{list(at)} head {hd}: {n_hip} NaN pixels, forward_ref {int(masks[hd].sum())} of {masks[hd].numel()}')
        assert bool(masks[hd].any()) and torch.equal(masks[hd], c['f64'][hd][1].isnan())
        assert torch.equal(got[hd].isnan().cpu(), masks[hd])
        assert torch.equal(got[hd][1], got_clean[hd][1]) and not bool(got[hd][1].isnan().any())
    if not all(bool(m[0].all()) for m in masks):
        fin = [~m for m in masks]
        for f in fin:
            f[1:] = False
        check_against_truth(got, c['f64'], c['f32'], f'NaN at hidden{list(at)}, finite pixels', where=fin)


@pytest.mark.parametrize('at', ref.NAN_AT, ids=['through-the-pools-only', 'inside-the-crops'])
def test_nan_propagates_as_in_torch_in_the_training_forward(rpe, at):
    """TinyUNet.forward_train_hip (csrc/unet_train.hip) on the same input concatenated, eval-mode norms, no sigmoid: its NaN pixels are
    those of the float32 CPU forward_ref logits (with frozen norms the restatement of test_gpu_unet_train.py's forward_ref).  Only the
    forward: under NaN every affected gradient is NaN either way."""
    h8, w8, b = ref.NAN_GRID
    c = ref.case(h8, w8, b, nan_at=at)
    for hd in range(2):
        net = copy.deepcopy(c['nets'][hd]).cuda().eval()
        out = net.forward_train_hip((c['xs'][hd].cuda(),)).detach()
        mask = c['f32'][hd][0].isnan()
        print(f'training forward, NaN at hidden{list(at)} head {hd}: {int(out.isnan().sum())} NaN pixels, forward_ref {int(mask.sum())}')
        assert bool(mask.any()) and out.shape == mask.shape
        assert torch.equal(out.isnan().cpu(), mask)


@pytest.mark.parametrize('h8,w8', [(43, 44), (44, 43)])
def test_grids_below_44_are_refused(rpe, h8, w8):
    from rpe_amd import ops
    L = rpe.lib()
    assert L.rpe_unet_workspace_bytes(1, h8, w8) == 0 and L.rpe_unet_workspace_bytes(1, 44, 44) > 0
    blobs = _blobs(44, 44, 2)
    z = lambda ch: torch.zeros(1, ch, h8, w8, device='cuda')
    with pytest.raises(rpe.RpeError, match='too small'):
        ops.unet_heads(z(8), z(8), z(128), z(128), blobs[0], blobs[1], (8 * h8, 8 * w8))
