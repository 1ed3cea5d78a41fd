"""CPU: the float64 restatement of tests/geometry_ref.py against oracle.warp (torch's own grid_sample / interpolate / linalg.inv) on the edge
scenes of tests/test_gpu_geometry_edges.py, the coverage those scenes must have, and the rule for positions that cannot be read -- so that
the truth the GPU tests compare with cannot drift along with the kernels, and none of them can go vacuous."""
import numpy as np
import pytest
import torch

import geometry_ref as ref
from oracle import warp

FUSED_SHAPES = [(8, 8), (8, 16), (16, 8), (24, 40), (40, 24), (16, 264)]
TAP_SHAPES = [(1, 1), (3, 257), (45, 47)]


@pytest.mark.parametrize('n', (1, 3))
@pytest.mark.parametrize('h,w', FUSED_SHAPES)
def test_restatement_agrees_with_torch_on_the_edge_scenes(n, h, w):
    """Discrete outputs equal; every float group within a bound worked out for float32: 64 * 2^-24 of the group's largest finite value
    (a dozen roundings of the ray, the depth product, four weighted taps and the mean, and torch's float32 LU inverse of a skewed K with the
    principal point outside the image, at a few ulp each).  The float32 error of torch is printed per group."""
    s = ref.edge_scene(n, h, w)
    got, want = ref.forward(s), ref.oracle_f32(s)
    assert torch.equal(torch.from_numpy(got['depth2']), want['depth2'])
    for k in ('mask2', 'mask2w'):
        assert np.array_equal(got[k], want[k].numpy()), k
    gg, gw = ref.groups(got), ref.groups(want)
    assert set(gg) == set(ref.GROUPS) == set(gw)
    for k in ref.GROUPS:
        e = ref.max_err(gw[k], gg[k])
        fin = np.isfinite(gg[k])
        scale = float(np.abs(gg[k][fin]).max())
        print(f'{n}x{h}x{w} {k:11s}: torch float32 error {e:.3e}  (largest value {scale:.3e}, ratio {e / scale:.2e})')
        assert e <= 64 * 2.0 ** -24 * scale, k
        assert scale < 1e20, k                                                 # the sentinels are in no output


@pytest.mark.parametrize('n,h,w,fused', [(n, h, w, True) for n in (1, 3) for h, w in FUSED_SHAPES] + [(2, h, w, False) for h, w in TAP_SHAPES])
def test_taps_are_the_oracles_where_it_can_say(n, h, w, fused):
    """oracle.warp.sample_taps casts to int64 whatever the position is; wherever the position reads, floor and nearest taps are its values,
    and everywhere else FAR_TAP."""
    s = ref.edge_scene(n, h, w, fused=fused)
    t = ref.taps(s['time_flow'])
    with np.errstate(all='ignore'):
        o = warp.sample_taps(s['time_flow'])
    for ax in 'xy':
        p = t['i' + ax]
        assert np.array_equal(p, o['i' + ax], equal_nan=True)
        ok = ref.reads(p)
        for k in (ax + '0', ax + 'n'):
            assert np.array_equal(t[k][ok], o[k][ok]), k
            assert bool((t[k][~ok] == ref.FAR_TAP).all()), k
    if (h, w) == (1, 1):
        assert not ref.reads(t['ix']).any() and not ref.reads(t['iy']).any()   # size - 1 = 0: every position is NaN or Inf


NEED = ['tie to even, down', 'tie to even, up', 'in (-1, 0)', 'in (size-1, size)', 'exactly size-1', 'exactly 0', 'below -1', 'at or beyond size',
        'does not read']


@pytest.mark.parametrize('n', (1, 3))
@pytest.mark.parametrize('h,w', FUSED_SHAPES)
def test_edge_scenes_cover_every_class(n, h, w):
    s = ref.edge_scene(n, h, w)
    c = ref.coverage(s)
    print(f'{n}x{h}x{w}: ' + ', '.join(f'{k} {v}' for k, v in c.items()))
    for ax in 'xy':
        for k in NEED:
            assert c[f'{ax}:{k}'] >= 1, (ax, k)
    for k in ('corner: both axes at a border', 'nan position', 'inf position', 'depth exactly 1 (valid)', 'depth one ulp above 1 (invalid)',
              'denormal depth (valid)', 'quotient nan', 'quotient +-inf', 'quotient +-0', 'nearest source: mask2 True, disparity invalid', 'sentinels'):
        assert c[k] >= 1, k
    assert c['rows with baseline 0'] == (1 if n == 3 else 0)
    m = s['meta']
    assert {(v if v == v else 'nan', ch) for (_, _, _, ch, v) in m['nonfinite']} >= {(v if v == v else 'nan', ch) for v in ref.NONFINITE for ch in (0, 1)}
    at = {(y, x) for (r, y, x, _, _) in m['nonfinite'] if r == 0}
    assert {(0, 0), (0, w - 1), (h - 1, w - 1), (1, w - 1)} <= at               # corners and a row end
    if h * w > 256:
        assert {divmod(255, w), divmod(256, w)} <= at                          # last lane of block 0, first lane of block 1
    # every K differs in every entry of its upper triangle, and one principal point is outside the image
    K = s['K'].numpy()
    for i in range(n):
        for j in range(i):
            assert all(K[i][a] != K[j][a] for a in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2)))
    assert any(not (0 <= k[0, 2] < w and 0 <= k[1, 2] < h) for k in K)
    assert len(set(s['baseline'].tolist())) == n


def test_exactly_minus_one_is_outside_the_round_trips_range_at_the_fused_sizes():
    """Why the fused scenes cannot hold a position of exactly -1 (or k + .5 near 0): for g = 2v/(size-1) - 1 in (-2, -1) the sum g + 1 lies on a
    grid of 2^-23, so positions near -1 lie on a grid of about (size - 1) * 2^-24, and -1 is on it only if (size - 1) divides 2^24 or
    2^24 + 1 (2^24 + 1 = 97 * 257 * 673).  Of the sizes the fused entry accepts (multiples of 8) that never holds below 8 * 97; here: every
    float32 within 4096 ulps of -1 as flow + index, at every size of the fused tests.  The tap tests have it at 3 x 257 (size - 1 = 2, 256)."""
    v = np.float32(-1.0) + np.arange(-4096, 4097, dtype=np.float64) * 2.0 ** -24
    v = v.astype(np.float32)
    for size in (8, 16, 24, 40, 264):
        p = ref._pos1(v, size)
        assert not bool((p == -1).any()), size
        assert bool((p < -1).any()) and bool(((p > -1) & (p < -0.999)).any())
    for size in (3, 257):
        assert ref._pos1(np.float32(-1.0), size) == -1 and ref._pos1(np.float32(0.5), size) == 0.5
    c = ref.coverage(ref.edge_scene(2, 3, 257, fused=False))
    for ax in 'xy':
        for k in NEED + ['exactly -1']:
            assert c[f'{ax}:{k}'] >= 1, (ax, k)
    for h, w in ((8, 8), (24, 40), (16, 264)):
        c = ref.coverage(ref.edge_scene(1, h, w))
        assert c['x:exactly -1'] == 0 and c['y:exactly -1'] == 0


@pytest.mark.parametrize('v', [1e9, -1e9, float('inf'), float('-inf')])
@pytest.mark.parametrize('comp', (0, 1))
def test_the_rule_is_what_torch_grid_sample_does(v, comp):
    """+-1e9 and +-Inf flow: torch's CPU grid_sample gives mask False there (nearest) and reads nothing (bilinear), as the rule says, and leaves
    every other pixel alone.  For +-1e9 its bilinear value is the rule's 0.  For +-Inf its bilinear weights are Inf - Inf = NaN and it multiplies
    the masked-out (zero) taps by them, so it returns NaN in every channel -- still no pixel's value; the rule and the kernels give 0 there, which
    is the only place where this restatement departs from torch on purpose (geometry_ref.oracle_f32 hands such pixels to torch as 1e9)."""
    g = torch.Generator().manual_seed(3)
    n, h, w = 1, 6, 9
    flow = torch.randn(n, 2, h, w, generator=g) * 2
    x = torch.rand(n, 3, h, w, generator=g) + 1.0                              # > 0 everywhere: a read would show
    mask = torch.ones(n, 1, h, w, dtype=torch.bool)
    plain_b, _ = warp.remap_from_flow(x, flow)
    spots = [(0, 0), (2, w - 1), (h - 1, 4)]
    for (y, xx) in spots:
        flow[0, comp, y, xx] = v
    ix, iy = ref.positions(flow)
    dead = ~(ref.reads(ix) & ref.reads(iy))
    assert int(dead.sum()) == len(spots) and all(dead[0, y, xx] for (y, xx) in spots)
    tb, _ = warp.remap_from_flow(x, flow)
    tn, valid = warp.remap_from_flow_nearest(mask, flow)
    mine_b = ref.bilinear(x.double().numpy(), ix, iy)
    mine_n = ref.nearest_mask(mask.numpy()[:, 0], ix, iy)
    for (y, xx) in spots:
        if np.isfinite(v):
            assert float(tb[0, :, y, xx].abs().max()) == 0.0
        else:
            assert bool(torch.isnan(tb[0, :, y, xx]).all())
        assert not bool((valid & tn.bool())[0, 0, y, xx])
        assert float(np.abs(mine_b[0, :, y, xx]).max()) == 0.0 and not bool(mine_n[0, y, xx])
    keep = torch.from_numpy(~dead)[:, None].expand_as(tb)
    assert torch.equal(tb[keep], plain_b[keep])
    assert float(np.abs(mine_b - torch.nan_to_num(tb, nan=0.0).double().numpy()).max()) <= 8 * 2.0 ** -24 * 2.0
    assert np.array_equal(mine_n, (valid & tn.bool()).numpy()[:, 0])
    t = ref.taps(flow)
    k0, kn = ('x0', 'xn') if comp == 0 else ('y0', 'yn')
    for (y, xx) in spots:
        assert t[k0][0, y, xx] == ref.FAR_TAP and t[kn][0, y, xx] == ref.FAR_TAP


def test_rule_boundaries_and_nan():
    p = np.array([np.nan, np.inf, -np.inf, 1e6, -1e6, np.nextafter(np.float32(1e6), np.float32(0)), -999999.5, 0.5, 1.5, -0.5, 2.5, 7.49], dtype=np.float32)
    assert ref.reads(p).tolist() == [False] * 5 + [True] * 7
    assert ref.floor_tap(p).tolist() == [ref.FAR_TAP] * 5 + [999999, -1000000, 0, 1, -1, 2, 7]
    assert ref.nearest_tap(p).tolist() == [ref.FAR_TAP] * 5 + [ref.FAR_TAP, ref.FAR_TAP, 0, 2, 0, 2, 7]     # rint(999999.94) = 1e6: does not read


def test_weights_and_mean_on_a_hand_case():
    """One 8x8 cell, K = identity: position (3.25, 4.5) of pixel (3, 3) written out by hand."""
    x = np.arange(64, dtype=np.float64).reshape(1, 1, 8, 8)
    ix, iy = np.full((1, 8, 8), 3.25, np.float32), np.full((1, 8, 8), 4.5, np.float32)
    want = 0.75 * 0.5 * x[0, 0, 4, 3] + 0.25 * 0.5 * x[0, 0, 4, 4] + 0.75 * 0.5 * x[0, 0, 5, 3] + 0.25 * 0.5 * x[0, 0, 5, 4]
    assert ref.bilinear(x, ix, iy)[0, 0, 3, 3] == want
    ix[0, 0, 0], iy[0, 0, 0] = -0.25, 7.5                                      # one tap of four inside: (7, 0), weight .75 * .5
    assert ref.bilinear(x, ix, iy)[0, 0, 0, 0] == 0.375 * x[0, 0, 7, 0]
    assert ref.down8(x)[0, 0, 0, 0] == (27 + 28 + 35 + 36) / 4
    r = ref.rays(np.eye(3)[None], 8, 8)
    assert r[0, :, 2, 5].tolist() == [5.5, 2.5, 1.0]
