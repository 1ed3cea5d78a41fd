"""GPU: the on-the-fly correlation lookup (ops.AltCorr, csrc/corr_alt.hip) against the float64 truth, with the pyramid route as yardstick.

Truth: oracle.raft.CorrBlock on the CPU with the feature maps (and the coordinates) cast to float64; its lookup is restated here without
the final cast to float32.  Yardstick: CorrPyramid.build + lookup on the same inputs.  Condition: max|alt - truth| <= 2 max|pyramid -
truth| per (geometry, coordinate case) -- the factor 2 is for a different but equally long summation order (a c-term dot product with
pooled features, then a 4-tap blend, against 4-pixel poolings of finished dot products) -- and every output whose four taps all lie
outside the level's map is exactly 0.

Geometries.  Both routes refuse a level smaller than 2 x 2 (bilinear_sampler divides by size - 1), so a map is run with as many levels as
the pyramid accepts: (1, 256, 8, 16) and (3, 256, 12, 20) with 3 levels (their fourth would be 1 x 2); (2, 256, 20, 22) -- 10 x 11, 5 x 5,
2 x 2: floored pooling twice, w8 % 8 != 0 -- and (1, 16, 16, 24) -- 16 = the smallest c rpe_corr_build accepts (c % 16 == 0) -- with 4.

Measured on an MI355X (max abs error alt / pyramid, worst coordinate case per geometry): see NOTES.md, "On-the-fly correlation"."""
import numpy as np
import pytest
import torch

from oracle import raft as oraft

pytestmark = pytest.mark.gpu

GEOMS = [(1, 256, 8, 16, 3), (3, 256, 12, 20, 3), (2, 256, 20, 22, 4), (1, 16, 16, 24, 4)]
CASES = ('flow30', 'integer', 'edges', 'far', 'scatter', 'const')


def make_coords(case, seed, b, h8, w8):
    rng = np.random.default_rng(seed)
    grid = oraft.coords_grid(b, h8, w8)
    if case == 'flow30':                                        # grid + uniform +-30 px
        return grid + torch.from_numpy(rng.uniform(-30, 30, size=(b, 2, h8, w8)).astype(np.float32))
    if case == 'integer':                                       # exactly integer coordinates
        return grid + torch.from_numpy(rng.integers(-3, 4, size=(b, 2, h8, w8)).astype(np.float32))
    if case == 'edges':                                         # -0.5, w8 - 1 and h8 - 1 + 0.5
        x = torch.from_numpy(rng.choice(np.array([-0.5, w8 - 1.0], np.float32), size=(b, h8, w8)))
        y = torch.from_numpy(rng.choice(np.array([-0.5, h8 - 1.0, h8 - 1 + 0.5], np.float32), size=(b, h8, w8)))
        return torch.stack((x, y), dim=1)
    if case == 'far':                                           # +-1e4: every tap is outside
        return torch.from_numpy(rng.choice(np.array([-1e4, 1e4], np.float32), size=(b, 2, h8, w8)))
    if case == 'scatter':                                       # neighbours point at different corners of the map: no shared box
        ys, xs = torch.meshgrid(torch.arange(h8), torch.arange(w8), indexing='ij')
        x = torch.where(xs % 2 == 0, 0.3, w8 - 1.3)
        y = torch.where(ys % 2 == 0, 0.6, h8 - 1.6)
        return torch.stack((x, y), dim=0).float()[None].repeat(b, 1, 1, 1).contiguous()
    if case == 'const':                                         # constant flow: one box per tile
        return grid + torch.tensor([1.3, -0.7]).view(1, 2, 1, 1)
    raise ValueError(case)


def truth_lookup(block, coords):
    """CorrBlock.__call__ (oracle/raft.py) in the dtype of its pyramid, without the cast of the result; also returns, per output, whether
    all four taps of its sample lie outside the level's map with a margin no rounding of the position reaches."""
    r = block.radius
    coords = coords.permute(0, 2, 3, 1)
    b, h1, w1, _ = coords.shape
    out, outside = [], []
    for i in range(block.num_levels):
        corr = block.corr_pyramid[i]
        d = torch.linspace(-r, r, 2 * r + 1, dtype=coords.dtype)
        delta = torch.stack(torch.meshgrid(d, d, indexing='ij'), dim=-1)
        lvl = coords.reshape(b * h1 * w1, 1, 1, 2) / 2 ** i + delta.view(1, 2 * r + 1, 2 * r + 1, 2)
        out.append(oraft.bilinear_sampler(corr, lvl).view(b, h1, w1, -1))
        H, W = corr.shape[-2:]
        x, y = lvl[..., 0], lvl[..., 1]
        outside.append(((x < -1.001) | (x > W + 0.001) | (y < -1.001) | (y > H + 0.001)).view(b, h1, w1, -1))
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous(), torch.cat(outside, dim=-1).permute(0, 3, 1, 2).contiguous()


class Scene:
    def __init__(self, geom):
        from rpe_amd import ops
        self.geom = geom
        b, c, h8, w8, levels = geom
        rng = np.random.default_rng(100 * h8 + w8 + c)
        self.f1 = torch.from_numpy(rng.normal(size=(b, c, h8, w8)).astype(np.float32))
        self.f2 = torch.from_numpy(rng.normal(size=(b, c, h8, w8)).astype(np.float32))
        self.block = oraft.CorrBlock(self.f1.double(), self.f2.double(), num_levels=levels, radius=4)
        self.g1, self.g2 = self.f1.cuda(), self.f2.cuda()
        self.pyr = ops.CorrPyramid(b, h8, w8, levels, device='cuda').build(self.g1, self.g2)
        self.alt = ops.AltCorr(b, c, h8, w8, levels, device='cuda').build(self.g1, self.g2)
        self.coords = {case: make_coords(case, 7 + k, b, h8, w8) for k, case in enumerate(CASES)}


_SCENES = {}


@pytest.fixture(scope='module')
def scenes(rpe):
    def get(geom):
        if geom not in _SCENES:
            _SCENES[geom] = Scene(geom)
        return _SCENES[geom]
    yield get
    _SCENES.clear()


@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: 'x'.join(map(str, g)))
def test_alt_lookup_against_float64_truth(scenes, geom):
    s = scenes(geom)
    b, c, h8, w8, levels = geom
    assert s.alt.nbytes == s.alt.buf.numel() > 0
    for case in CASES:
        co = s.coords[case]
        truth, outside = truth_lookup(s.block, co.double())
        got = s.alt.lookup(co.cuda()).cpu()
        ref = s.pyr.lookup(co.cuda()).cpu()
        assert got.shape == ref.shape == truth.shape == (b, levels * 81, h8, w8)
        e_alt, e_pyr = float((got.double() - truth).abs().max()), float((ref.double() - truth).abs().max())
        print(f'corr_alt {geom} {case}: max|alt - truth| = {e_alt:.3e}, max|pyramid - truth| = {e_pyr:.3e}, scale {float(truth.abs().max()):.3f}, '
              f'{int(outside.sum())} outputs wholly outside')
        assert not bool(truth[outside].any())                   # (the mask marks what the truth has as exactly 0)
        assert not bool(got[outside].any()), case               # ... and the route returns exactly 0 there
        assert e_alt <= 2 * e_pyr, (case, e_alt, e_pyr)
        if case in ('far', 'flow30'):
            assert int(outside.sum()) > 0
        if case == 'far':
            assert bool(outside.all())


def test_far_case_is_all_zero(scenes):
    s = scenes(GEOMS[1])
    out = s.alt.lookup(s.coords['far'].cuda())
    assert not bool(out.any())


def test_path_identity_smooth_against_scattered_neighbours(scenes):
    """The same query (coordinate, features) among smooth neighbours -- served by the tile's one box -- and among neighbours that point at
    the corners of the map -- served in a round of its own: bitwise the same 81 * levels values."""
    s = scenes(GEOMS[2])
    b, c, h8, w8, levels = s.geom
    smooth, scat = s.coords['const'].clone(), s.coords['scatter'].clone()
    keep = [(0, 0), (5, 9), (7, 7), (8, 8), (13, 21), (19, 3), (19, 21)]
    for y, x in keep:
        scat[:, :, y, x] = smooth[:, :, y, x]
    a, d = s.alt.lookup(smooth.cuda()), s.alt.lookup(scat.cuda())
    for y, x in keep:
        assert torch.equal(a[:, :, y, x], d[:, :, y, x]), (y, x)
    assert not torch.equal(a, d)
    # and the scattered launch is still right everywhere
    truth, _ = truth_lookup(s.block, scat.double())
    ref = s.pyr.lookup(scat.cuda()).cpu()
    assert float((d.cpu().double() - truth).abs().max()) <= 2 * float((ref.double() - truth).abs().max())


def test_batch_independence(scenes):
    from rpe_amd import ops
    s = scenes(GEOMS[1])
    b, c, h8, w8, levels = s.geom
    for case in ('flow30', 'const', 'scatter'):
        co = s.coords[case].cuda()
        full = s.alt.lookup(co)
        for i in range(b):
            one = ops.AltCorr(1, c, h8, w8, levels, device='cuda').build(s.g1[i:i + 1].contiguous(), s.g2[i:i + 1].contiguous())
            assert torch.equal(one.lookup(co[i:i + 1].contiguous())[0], full[i]), (case, i)


def test_determinism(scenes):
    s = scenes(GEOMS[2])
    for case in ('flow30', 'scatter'):
        co = s.coords[case].cuda()
        assert torch.equal(s.alt.lookup(co), s.alt.lookup(co)), case


def test_prepared_route_through_a_launch_list(scenes):
    from rpe_amd import ops
    s = scenes(GEOMS[2])
    b, c, h8, w8, levels = s.geom
    co = s.coords['flow30'].cuda()
    direct = s.alt.lookup(co)
    out = torch.full_like(direct, float('nan'))
    launcher = s.alt.lookup(co, out=out, prepare=True)
    prog = ops.OpList().add(launcher)
    prog.run((ops.raw_stream(),))
    assert torch.equal(out, direct)
    out.fill_(float('nan'))
    assert launcher() is out and torch.equal(out, direct)


def test_shape_checks(scenes):
    from rpe_amd import ops
    from rpe_amd._lib import RpeError
    s = scenes(GEOMS[0])
    b, c, h8, w8, levels = s.geom
    with pytest.raises(RpeError):
        s.alt.build(s.g1, s.g2[:, :, :-1])
    with pytest.raises(RpeError):
        s.alt.lookup(torch.zeros(b, 2, h8, w8 + 1, device='cuda'))
    with pytest.raises(RpeError):
        s.alt.lookup(s.coords['const'].cuda(), out=torch.empty(b, 5, h8, w8, device='cuda'))
    with pytest.raises(RpeError):
        ops.AltCorr(1, 256, 8, 16, 4, device='cuda')            # the fourth level would be 1 x 2
    with pytest.raises(RpeError):
        ops.AltCorr(1, 24, 16, 16, 4, device='cuda')
