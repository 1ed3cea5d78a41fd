"""GPU: the fused geometry kernels of csrc/geometry.hip (rpe_depth_backproject_warp, rpe_flow2depth, rpe_warp_taps) at their edges against
the float64 restatement of tests/geometry_ref.py (pinned on the CPU by tests/test_geometry_ref_cpu.py).

The scenes (geometry_ref.edge_scene) have a K and a baseline of their own in every row (one principal point outside the image, one baseline
0), time flow built as target - index so that positions fall on ties, borders and just beside them on both axes, NaN / +-Inf / +-1e9 / +-3e38
flow at corners, row ends and the first and last lane of a block, disparities of +-0, NaN, +-Inf, denormals, depth exactly 1 and one ulp
above, and 1e30 sentinels in image2l and stereo_flow2[:, 1] where no tap falls.  Shapes: one 1/8 cell, one partial block, hw not a multiple
of 256, narrow and tall maps; for the two plain kernels also 1x1, 3x257 and 45x47.

Discrete outputs (depth2, mask2, mask2w, the four tap arrays) are bit-exact.  Float outputs are judged per channel group: the bar of a group
is 4x the error E of the torch float32 oracle against the same float64 truth in the same case (E is measured on the oracle alone); the
margin is for the one extra rounding of the float64-inverted K^-1 and the fused multiply-adds of the ray.  Measured values: NOTES.md,
"Fused geometry: float64 parity"."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import geometry_ref as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FUSED_SHAPES = [(8, 8), (8, 16), (16, 8), (24, 40), (40, 24), (16, 264)]
TAP_SHAPES = FUSED_SHAPES + [(1, 1), (3, 257), (45, 47)]
BADARG = -1
DISCRETE = ('depth2', 'mask2', 'mask2w')
FLOATS = ('pcl1', 'pcl2w', 'inp1', 'inp2', 'pcl2')


@functools.lru_cache(maxsize=None)
def case(n, h, w):
    """(scene, float64 truth, its channel groups, E per group): computed once, shared, never written to."""
    s = ref.edge_scene(n, h, w)
    truth = ref.forward(s)
    gt, go = ref.groups(truth), ref.groups(ref.oracle_f32(s))
    return s, truth, gt, {k: ref.max_err(go[k], gt[k]) for k in ref.GROUPS}


def run(scene, want_pcl2=True):
    from rpe_amd import ops
    return ops.depth_backproject_warp(*[scene[k].to(DEV) for k in ref.ARGS], want_pcl2=want_pcl2)


def bits(t):
    """The tensor's bytes (so that NaN equals NaN and -0 differs from +0)."""
    return t.detach().cpu().contiguous().view(torch.uint8).numpy() if t.dtype != torch.bool else t.detach().cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize('n', (1, 3))
@pytest.mark.parametrize('h,w', FUSED_SHAPES)
def test_fused_pass_against_float64(rpe, n, h, w):
    """Every output of rpe_depth_backproject_warp on the edge scene: discrete outputs bit-exact, every float group within 4 E, pixels whose
    position does not read exactly 0 / False, no sentinel in any output.

    Measured on an MI355X: ratios kernel / E from 0.52 to 2.67 (the largest at inp1.sflow of 1x8x8, three values), E from 1e-9 (inp2.sflow at
    8x8) over 1e-7 (clouds) to 2.5e-5 (images)."""
    s, truth, gt, E = case(n, h, w)
    out = run(s)
    assert np.array_equal(bits(out['depth2']), bits(torch.from_numpy(truth['depth2'])))
    for k in ('mask2', 'mask2w'):
        assert np.array_equal(out[k].cpu().numpy(), truth[k]), k
    dead = torch.from_numpy(ref.no_read(s))
    assert int(dead.sum()) >= 14 * n
    assert float(out['pcl2w'].cpu()[dead[:, None].expand(n, 3, h, w)].abs().max()) == 0.0
    assert not bool(out['mask2w'].cpu()[dead[:, None]].any())
    gk = ref.groups(out)
    bad = []
    for k in ref.GROUPS:
        assert float(np.nanmax(np.where(np.isfinite(gk[k]), np.abs(gk[k]), 0.0))) < 1e20, f'{k}: a sentinel was read'
        e = ref.max_err(gk[k], gt[k])
        print(f'geometry {n}x{h}x{w} {k:11s}: E {E[k]:.3e}   kernel {e:.3e}   ratio {e / E[k] if E[k] else float(e > 0):.2f}')
        if not e <= 4.0 * E[k]:
            bad.append((k, e, E[k]))
    assert not bad, bad


@pytest.mark.parametrize('h,w', FUSED_SHAPES)
def test_dead_centre_pixel_contributes_zero_to_its_cell(rpe, h, w):
    """The cell whose centre pixel (8i+4, 8j+4) has a position that does not read: its inp2 value is a quarter of the sum of the other three
    warped centre pixels (float64 truth, 4 E bar as above; the scene puts a non-finite flow on the last cell's centre)."""
    s, truth, gt, E = case(1, h, w)
    dead = ref.no_read(s)[0]
    i, j = h // 8 - 1, w // 8 - 1
    assert dead[8 * i + 4, 8 * j + 4]
    full = np.concatenate((ref.bilinear(s['stereo_flow2'].double().numpy(), truth['ix'], truth['iy']),
                           ref.bilinear(s['image2l'].double().numpy(), truth['ix'], truth['iy']), truth['pcl2w']), axis=1)
    alive = [(y, x) for y in (8 * i + 3, 8 * i + 4) for x in (8 * j + 3, 8 * j + 4) if not dead[y, x]]
    want = sum(full[0, :, y, x] for (y, x) in alive) / 4.0
    got = run(s)['inp2'][0, :, i, j].cpu().double().numpy()
    for k, sl in (('inp2.sflow', slice(0, 2)), ('inp2.image', slice(2, 5)), ('inp2.cloud', slice(5, 8))):
        fin = np.isfinite(want[sl])
        assert np.array_equal(np.isfinite(got[sl]), fin)
        assert float(np.abs(got[sl][fin] - want[sl][fin]).max(initial=0.0)) <= 4.0 * E[k], k


@pytest.mark.parametrize('h,w', TAP_SHAPES)
def test_warp_taps_everywhere_far_value_included(rpe, h, w):
    """All four tap arrays equal the restatement in every pixel; where a position does not read, the documented far value -1000000."""
    from rpe_amd import ops
    fused = h % 8 == 0 and w % 8 == 0
    s = ref.edge_scene(2 if not fused else 3, h, w, fused=fused)
    t = ref.taps(s['time_flow'])
    got = ops.warp_taps(s['time_flow'].to(DEV))
    far = 0
    for ax in 'xy':
        ok = ref.reads(t['i' + ax])
        far += int((~ok).sum())
        for k in (ax + '0', ax + 'n'):
            a = got[k].cpu().numpy()
            assert a.dtype == np.int32 and np.array_equal(a, t[k].astype(np.int32)), k
            assert bool((a[~ok] == ref.FAR_TAP).all()), k
    assert far >= 1


@pytest.mark.parametrize('h,w', TAP_SHAPES)
def test_flow2depth_disparity_edges(rpe, h, w):
    """rpe_flow2depth bit for bit on +-0, NaN, +-Inf, denormal, huge, depth == 1 and one ulp either side, baseline 0; at the fused shapes it
    is also the fused pass's depth2, and its validity ANDed with the mask the fused pass's mask2."""
    from rpe_amd import ops
    from oracle import warp
    fused = h % 8 == 0 and w % 8 == 0
    s = ref.edge_scene(3, h, w, fused=fused)
    names = {nm for (_, _, _, nm) in s['meta']['disparity']}
    if h * w >= 40:
        assert names == {nm for nm, _ in ref.disparity_edges(1.0)}
    d, v = ops.flow2depth(s['stereo_flow2'].to(DEV), s['baseline'].to(DEV))
    dr, vr = warp.flow2depth(s['stereo_flow2'], s['baseline'])
    assert same_bits(d, dr) and same_bits(v, vr)
    assert not bool(v[2].any()) and bool((d[2] == 1).all())                    # the row with baseline 0
    if fused:
        out = run(s)
        assert same_bits(out['depth2'], d) and same_bits(out['mask2'], v & s['mask2'].to(DEV))
        # a pixel whose nearest source has an invalid disparity under a True mask: warped mask False
        for (r, py, px, y, x, nm) in s['meta']['pointers']:
            if nm != 'depth==1' or float(s['baseline'][r]) == 0.0:
                assert bool(s['mask2'][r, 0, y, x]) and not bool(vr[r, 0, y, x]) and not bool(out['mask2w'][r, 0, py, px]), (r, nm)
            else:
                assert bool(vr[r, 0, y, x]) and bool(out['mask2w'][r, 0, py, px]), (r, nm)
        assert len(s['meta']['pointers']) >= 3


def test_rows_do_not_depend_on_their_batch(rpe):
    """24x40: each row of the n = 3 call, of the call with the rows permuted, and of an n = 1 call on that row's inputs -- the same bits in
    every output."""
    s = case(3, 24, 40)[0]
    perm = [2, 0, 1]
    together, shuffled = run(s), run(ref.permuted(s, perm))
    for r in range(3):
        alone = run(ref.row_of(s, r))
        for k in DISCRETE + FLOATS:
            assert same_bits(alone[k], together[k][r:r + 1]), (r, k)
            assert same_bits(alone[k], shuffled[k][perm.index(r):perm.index(r) + 1]), (r, k)


@pytest.mark.parametrize('h,w', [(8, 8), (24, 40), (16, 264)])
def test_want_pcl2_changes_nothing_else(rpe, h, w):
    s = case(3, h, w)[0]
    a, b = run(s, want_pcl2=True), run(s, want_pcl2=False)
    assert b['pcl2'] is None and a['pcl2'] is not None
    for k in DISCRETE + FLOATS[:-1]:
        assert same_bits(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------------- guard bands
GUARD = 4096
PATTERN = 0xA5


def guarded(nbytes, offset):
    """``nbytes`` bytes starting ``offset`` bytes past a 256-byte boundary, with GUARD bytes of PATTERN before and at least GUARD behind."""
    big = torch.full((256 + GUARD + offset + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    start = (-big.data_ptr()) % 256 + GUARD + offset
    assert (big.data_ptr() + start) % 256 == offset
    return big, start


def intact(big, start, nbytes):
    return bool((big[:start] == PATTERN).all()) and bool((big[start + nbytes:] == PATTERN).all())


def vp(big, start):
    return ctypes.c_void_p(big.data_ptr() + start)


@pytest.mark.parametrize('n,h,w', [(1, 8, 8), (3, 8, 8), (1, 24, 40), (3, 24, 40)])
def test_fused_pass_stays_inside_its_outputs(rpe, n, h, w):
    """rpe_depth_backproject_warp called directly, every output a region of a larger buffer of 0xA5 bytes, float bases 4 bytes and uint8 bases
    1 byte past a 256-byte boundary: no byte outside the regions changes, and the regions hold the bits of ops.depth_backproject_warp."""
    from rpe_amd._lib import lib, ptr, stream_ptr
    s = case(n, h, w)[0]
    want = run(s)
    ins = [s[k].to(DEV).contiguous() for k in ref.ARGS[:-1]] + [s['mask2'].to(DEV).to(torch.uint8).contiguous()]
    hw, hw8 = h * w, (h // 8) * (w // 8)
    sizes = dict(depth2=(4 * n * hw, 4), mask2=(n * hw, 1), pcl1=(12 * n * hw, 4), pcl2w=(12 * n * hw, 4), mask2w=(n * hw, 1),
                 inp1=(32 * n * hw8, 4), inp2=(32 * n * hw8, 4), pcl2=(12 * n * hw, 4))
    buf = {k: guarded(nb, off) for k, (nb, off) in sizes.items()}
    st = lib().rpe_depth_backproject_warp(*[ptr(t) for t in ins], n, h, w, *[vp(*buf[k]) for k in sizes], stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    for k, (nb, _) in sizes.items():
        big, start = buf[k]
        assert intact(big, start, nb), k
        assert np.array_equal(big[start:start + nb].cpu().numpy(), bits(want[k]).reshape(-1).view(np.uint8)), k


def test_plain_kernels_stay_inside_their_outputs(rpe):
    """rpe_flow2depth and rpe_warp_taps at 3x257 (771 pixels: three blocks and three lanes), the same guard bands."""
    from rpe_amd import ops
    from rpe_amd._lib import lib, ptr, stream_ptr
    n, h, w = 2, 3, 257
    s = ref.edge_scene(n, h, w, fused=False)
    sf, b, tf = s['stereo_flow2'].to(DEV), s['baseline'].to(DEV), s['time_flow'].to(DEV)
    d, v = ops.flow2depth(sf, b)
    taps = ops.warp_taps(tf)
    hw = h * w
    bd, bv = guarded(4 * n * hw, 4), guarded(n * hw, 1)
    st = lib().rpe_flow2depth(ptr(sf), ptr(b), n, h, w, vp(*bd), vp(*bv), stream_ptr())
    bt = [guarded(4 * n * hw, 4) for _ in range(4)]
    st2 = lib().rpe_warp_taps(ptr(tf), n, h, w, *[vp(*x) for x in bt], stream_ptr())
    torch.cuda.synchronize()
    assert st == 0 and st2 == 0
    for (big, start), nb, want in [(bd, 4 * n * hw, d), (bv, n * hw, v)] + [(x, 4 * n * hw, taps[k]) for x, k in zip(bt, ('x0', 'y0', 'xn', 'yn'))]:
        assert intact(big, start, nb)
        assert np.array_equal(big[start:start + nb].cpu().numpy(), bits(want).reshape(-1).view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(rpe):
    """RPE_E_BADARG for h or w not a multiple of 8 (fused entry), n, h or w <= 0, and every null required pointer; a null pcl2 is accepted.
    The outputs of a refused call are untouched."""
    from rpe_amd._lib import lib, ptr, stream_ptr
    n, h, w = 1, 8, 16
    s = case(1, 8, 16)[0]
    ins = [s[k].to(DEV).contiguous() for k in ref.ARGS[:-1]] + [s['mask2'].to(DEV).to(torch.uint8).contiguous()]
    hw, hw8 = h * w, 2
    outs = [torch.full((nb,), PATTERN, dtype=torch.uint8, device=DEV) for nb in (4 * hw, hw, 12 * hw, 12 * hw, hw, 32 * hw8, 32 * hw8, 12 * hw)]
    null = ctypes.c_void_p(0)

    def fused(args=None, dims=(n, h, w), o=None):
        a = [ptr(t) for t in ins] if args is None else args
        oo = [ptr(t) for t in outs] if o is None else o
        return lib().rpe_depth_backproject_warp(*a, *dims, *oo, stream_ptr())

    for dims in ((1, 7, 16), (1, 8, 12), (1, 4, 4), (1, 9, 16), (0, 8, 16), (-1, 8, 16), (1, 0, 16), (1, 8, 0), (1, -8, 16), (1, 8, -16)):
        assert fused(dims=dims) == BADARG, dims
    for i in range(9):
        a = [ptr(t) for t in ins]
        a[i] = null
        assert fused(args=a) == BADARG, i
    for i in range(7):                                                         # every output but pcl2
        o = [ptr(t) for t in outs]
        o[i] = null
        assert fused(o=o) == BADARG, i
    torch.cuda.synchronize()
    assert all(bool((t == PATTERN).all()) for t in outs)
    o = [ptr(t) for t in outs]
    o[7] = null
    assert fused(o=o) == 0                                                     # a null pcl2 is accepted
    torch.cuda.synchronize()
    assert bool((outs[7] == PATTERN).all()) and not bool((outs[0] == PATTERN).all())

    sf, b, tf = ins[0], ins[2], ins[1]
    d, v = torch.full((4 * hw,), PATTERN, dtype=torch.uint8, device=DEV), torch.full((hw,), PATTERN, dtype=torch.uint8, device=DEV)
    f2d = lambda a, dims: lib().rpe_flow2depth(a[0], a[1], *dims, a[2], a[3], stream_ptr())    # noqa: E731
    good = [ptr(sf), ptr(b), ptr(d), ptr(v)]
    for dims in ((0, h, w), (1, 0, w), (1, h, 0), (-1, h, w), (1, -1, w), (1, h, -1)):
        assert f2d(good, dims) == BADARG, dims
    for i in range(4):
        a = list(good)
        a[i] = null
        assert f2d(a, (n, h, w)) == BADARG, i
    t4 = [torch.full((4 * hw,), PATTERN, dtype=torch.uint8, device=DEV) for _ in range(4)]
    wt = lambda a, dims: lib().rpe_warp_taps(a[0], *dims, *a[1:], stream_ptr())                # noqa: E731
    good = [ptr(tf)] + [ptr(t) for t in t4]
    for dims in ((0, h, w), (1, 0, w), (1, h, 0), (-1, h, w), (1, -1, w), (1, h, -1)):
        assert wt(good, dims) == BADARG, dims
    for i in range(5):
        a = list(good)
        a[i] = null
        assert wt(a, (n, h, w)) == BADARG, i
    torch.cuda.synchronize()
    assert all(bool((t == PATTERN).all()) for t in [d, v] + t4)
