"""GPU: the on-the-fly correlation lookup on fp16 feature maps (ops.AltCorr(fp16=True), csrc/corr_alt.hip) against float64 truth, with the
pyramid route's fp16 build as yardstick.

Truth: oracle.raft.CorrBlock in float64 on f1.half().double() and f2.half().double() -- level 0 rounded as the route rounds it, the
higher levels pooled exactly.  Yardstick: CorrPyramid.build(.., fp16_features=True) + lookup against the same truth, per level:
e_pyr16[l].  Conditions per (geometry, coordinate case):
  level 0:   max|alt16 - truth| <= 2 e_pyr16[0]       (a different but equally long f32 summation order, as tests/test_gpu_corr_alt.py)
  level l:   max|alt16 - truth| <= 2 e_pyr16[l] + B_l,
             B_l = l 2^-11 (1 + 2^-11)^l max_{q,p} sum_k |f1h[q,k]| max(A_l[p,k], 2^-14) / sqrt(c),   A_l = avg_pool^l(|f2.half()|)
             -- each of the l successive roundings of a pooled map costs at most 2^-11 of the value's magnitude (2^-25 absolute in the
             subnormal range); pooling and the bilinear blend are convex, so neither grows the maximum.  Computed in float64.
  every output whose four taps lie outside the level's map is exactly 0.
Geometries: those of tests/test_gpu_corr_alt.py plus (1, 48, 16, 24, 4): three 16-channel steps and a 1 / sqrt(c) that is no power of two
(c = 16: one step).  Coordinates and the truth's lookup are that file's.

Measured on an MI355X (e_alt16 / e_pyr16 per level): see NOTES.md, "On-the-fly correlation"."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import raft as oraft
from test_gpu_corr_alt import CASES, make_coords, truth_lookup

pytestmark = pytest.mark.gpu

GEOMS = [(1, 256, 8, 16, 3), (3, 256, 12, 20, 3), (2, 256, 20, 22, 4), (1, 16, 16, 24, 4), (1, 48, 16, 24, 4)]
NAN = float('nan')


def _pad():
    from conftest import ROOT
    import os
    return int(re.search(r'#define RPE_CORR_ALT_PAD (\d+)', open(os.path.join(ROOT, 'include', 'rpe.h')).read()).group(1))


class Scene:
    def __init__(self, geom):
        from rpe_amd import ops
        self.geom = geom
        b, c, h8, w8, levels = geom
        rng = np.random.default_rng(100 * h8 + w8 + c)
        self.f1 = torch.from_numpy(rng.normal(size=(b, c, h8, w8)).astype(np.float32))
        self.f2 = torch.from_numpy(rng.normal(size=(b, c, h8, w8)).astype(np.float32))
        f1h, f2h = self.f1.half().double(), self.f2.half().double()
        self.block = oraft.CorrBlock(f1h, f2h, num_levels=levels, radius=4)
        self.g1, self.g2 = self.f1.cuda(), self.f2.cuda()
        self.pyr16 = ops.CorrPyramid(b, h8, w8, levels, device='cuda').build(self.g1, self.g2, fp16_features=True)
        self.alt16 = ops.AltCorr(b, c, h8, w8, levels, device='cuda', fp16=True).build(self.g1, self.g2)
        self.coords = {case: make_coords(case, 7 + k, b, h8, w8) for k, case in enumerate(CASES)}
        # B_l (float64): the derived cost of rounding the pooled maps once per level
        q = f1h.abs().reshape(b, c, h8 * w8).transpose(1, 2)                     # (b, nq, c)
        A, self.B = f2h.abs(), [0.0]
        for l in range(1, levels):
            A = F.avg_pool2d(A, 2, stride=2)
            s = torch.matmul(q, A.clamp_min(2.0 ** -14).reshape(b, c, -1))      # (b, nq, np)
            self.B.append(l * 2.0 ** -11 * (1 + 2.0 ** -11) ** l * float(s.max()) / float(np.sqrt(np.float64(c))))
        self._truth = {}

    def truth(self, case):
        if case not in self._truth:
            self._truth[case] = truth_lookup(self.block, self.coords[case].double())
        return self._truth[case]


_SCENES = {}


@pytest.fixture(scope='module')
def scenes(rpe):
    def get(geom):
        if geom not in _SCENES:
            _SCENES[geom] = Scene(geom)
        return _SCENES[geom]
    yield get
    _SCENES.clear()


def _per_level(t, levels):
    return [float(t[:, 81 * l:81 * (l + 1)].abs().max()) for l in range(levels)]


@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: 'x'.join(map(str, g)))
def test_alt16_lookup_against_float64_truth(scenes, geom):
    s = scenes(geom)
    b, c, h8, w8, levels = geom
    assert s.alt16.fp16 and s.alt16.nbytes == s.alt16.buf.numel() > 0
    for case in CASES:
        co = s.coords[case]
        truth, outside = s.truth(case)
        got = s.alt16.lookup(co.cuda()).cpu()
        ref = s.pyr16.lookup(co.cuda()).cpu()
        assert got.shape == ref.shape == truth.shape == (b, levels * 81, h8, w8)
        e_alt, e_pyr = _per_level(got.double() - truth, levels), _per_level(ref.double() - truth, levels)
        print(f'corr_alt16 {geom} {case}: ' + '; '.join(f'level {l}: e_alt16 {e_alt[l]:.3e} e_pyr16 {e_pyr[l]:.3e} B_l {s.B[l]:.3e}' for l in range(levels))
              + f'; scale {float(truth.abs().max()):.3f}, {int(outside.sum())} outputs wholly outside')
        assert not bool(truth[outside].any())                   # (the mask marks what the truth has as exactly 0)
        assert not bool(got[outside].any()), case               # ... and the route returns exactly 0 there
        assert bool(torch.isfinite(got).all())
        assert e_alt[0] <= 2 * e_pyr[0], (case, 0, e_alt[0], e_pyr[0])
        for l in range(1, levels):
            assert e_alt[l] <= 2 * e_pyr[l] + s.B[l], (case, l, e_alt[l], e_pyr[l], s.B[l])
        if case in ('far', 'flow30'):
            assert int(outside.sum()) > 0
        if case == 'far':
            assert bool(outside.all()) and not bool(got.any())


def test_path_identity_smooth_against_scattered_neighbours(scenes):
    """The same query among smooth neighbours (the tile's one box) and among neighbours that point at the corners of the map (a round of
    its own): bitwise the same 81 * levels values."""
    s = scenes(GEOMS[2])
    smooth, scat = s.coords['const'].clone(), s.coords['scatter'].clone()
    keep = [(0, 0), (5, 9), (7, 7), (8, 8), (13, 21), (19, 3), (19, 21)]
    for y, x in keep:
        scat[:, :, y, x] = smooth[:, :, y, x]
    a, d = s.alt16.lookup(smooth.cuda()), s.alt16.lookup(scat.cuda())
    for y, x in keep:
        assert torch.equal(a[:, :, y, x], d[:, :, y, x]), (y, x)
    assert not torch.equal(a, d)


def test_batch_independence(scenes):
    from rpe_amd import ops
    s = scenes(GEOMS[1])
    b, c, h8, w8, levels = s.geom
    for case in ('flow30', 'const', 'scatter'):
        co = s.coords[case].cuda()
        full = s.alt16.lookup(co)
        for i in range(b):
            one = ops.AltCorr(1, c, h8, w8, levels, device='cuda', fp16=True).build(s.g1[i:i + 1].contiguous(), s.g2[i:i + 1].contiguous())
            assert torch.equal(one.lookup(co[i:i + 1].contiguous())[0], full[i]), (case, i)


def test_determinism(scenes):
    s = scenes(GEOMS[2])
    for case in ('flow30', 'scatter'):
        co = s.coords[case].cuda()
        assert torch.equal(s.alt16.lookup(co), s.alt16.lookup(co)), case


def test_prepared_route_through_a_launch_list(scenes):
    from rpe_amd import _lib, ops
    s = scenes(GEOMS[2])
    co = s.coords['flow30'].cuda()
    direct = s.alt16.lookup(co)
    out = torch.full_like(direct, NAN)
    launcher = s.alt16.lookup(co, out=out, prepare=True)
    assert launcher.op[0] == _lib.OP_CORR_ALT_LOOKUP_DT
    prog = ops.OpList().add(launcher)
    prog.run((ops.raw_stream(),))
    assert torch.equal(out, direct)
    out.fill_(NAN)
    prog.run((ops.raw_stream(),))
    assert torch.equal(out, direct)
    out.fill_(NAN)
    assert launcher() is out and torch.equal(out, direct)


@pytest.mark.parametrize('geom', [GEOMS[2], GEOMS[4]], ids=lambda g: 'x'.join(map(str, g)))
def test_padded_maps(scenes, geom):
    """Coords and out as the top-left h8 x w8 of (h8 + 3, w8 + 5) maps prefilled with NaN: inside, the dense lookup's bits; every other
    element of out is still NaN (nothing outside the rectangle is read or written)."""
    s = scenes(geom)
    b, c, h8, w8, levels = geom
    mh, mw = h8 + 3, w8 + 5
    for case in ('flow30', 'scatter'):
        co = s.coords[case].cuda()
        want = s.alt16.lookup(co)
        cpad = torch.full((b, 2, mh, mw), NAN, device='cuda')
        cpad[:, :, :h8, :w8] = co
        out = torch.full((b, levels * 81, mh, mw), NAN, device='cuda')
        assert s.alt16.lookup(cpad, out=out, map_size=(mh, mw)) is out
        assert torch.equal(out[:, :, :h8, :w8], want), case
        rest = torch.ones(mh, mw, dtype=torch.bool, device='cuda')
        rest[:h8, :w8] = False
        assert bool(out[:, :, rest].isnan().all()), case
        # prepared, through a launch list
        from rpe_amd import ops
        out2 = torch.full_like(out, NAN)
        ops.OpList().add(s.alt16.lookup(cpad, out=out2, map_size=(mh, mw), prepare=True)).run((ops.raw_stream(),))
        assert torch.equal(out2[:, :, :h8, :w8], want) and bool(out2[:, :, rest].isnan().all()), case


def test_fp16_false_is_todays_route(scenes):
    """AltCorr(fp16=False) makes the f32 calls it always made and returns their bits; rpe_corr_alt_lookup_dt(RPE_F32) forwards to them."""
    from rpe_amd import _lib, ops
    s = scenes(GEOMS[2])
    b, c, h8, w8, levels = s.geom
    with _lib.CountingLib() as count:
        today = ops.AltCorr(b, c, h8, w8, levels, device='cuda').build(s.g1, s.g2)
        off = ops.AltCorr(b, c, h8, w8, levels, device='cuda', fp16=False).build(s.g1, s.g2)
        co = s.coords['flow30'].cuda()
        a, d = today.lookup(co), off.lookup(co)
    assert count.names == ['rpe_corr_alt_prepare'] * 2 + ['rpe_corr_alt_lookup'] * 2
    assert torch.equal(a, d) and off.fp16 is False
    assert off.nbytes == today.nbytes == rpe_bytes(b, c, h8, w8, levels) == off.buf.numel()
    fwd = torch.full_like(a, NAN)
    ops._launch(_lib.OP_CORR_ALT_LOOKUP_DT, (ops.ptr(off.buf), ops.ptr(co), b, c, h8, w8, levels, 4, h8, w8, _lib.F32, ops.ptr(fwd)), (off, co, fwd), fwd)
    assert torch.equal(fwd, a)
    assert not torch.equal(s.alt16.lookup(co), a)               # (and the fp16 route does round)


def rpe_bytes(b, c, h8, w8, levels):
    from rpe_amd import lib
    return lib().rpe_corr_alt_bytes(b, c, h8, w8, levels)


@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: 'x'.join(map(str, g)))
def test_fp16_scratch_is_half_the_bytes(scenes, geom):
    b, c, h8, w8, levels = geom
    n16, n32 = scenes(geom).alt16.nbytes, rpe_bytes(b, c, h8, w8, levels)
    assert 0 < n16 <= 0.5 * n32 + _pad() * levels, (n16, n32)
    assert n16 >= 2 * (b * c * h8 * w8 * 2)


def test_shape_checks(scenes):
    from rpe_amd import ops
    from rpe_amd._lib import RpeError
    s = scenes(GEOMS[0])
    b, c, h8, w8, levels = s.geom
    with pytest.raises(RpeError):
        s.alt16.build(s.g1, s.g2[:, :, :-1])
    with pytest.raises(RpeError):
        s.alt16.lookup(torch.zeros(b, 2, h8, w8 + 1, device='cuda'))
    with pytest.raises(RpeError):
        s.alt16.lookup(s.coords['const'].cuda(), out=torch.empty(b, 5, h8, w8, device='cuda'))
    with pytest.raises(RpeError):
        s.alt16.lookup(s.coords['const'].cuda(), out=torch.empty(b, levels * 81, h8, w8, device='cuda'), map_size=(h8, w8 - 1))
    with pytest.raises(RpeError):
        ops.AltCorr(1, 256, 8, 16, 4, device='cuda', fp16=True)  # the fourth level would be 1 x 2
    with pytest.raises(RpeError):
        ops.AltCorr(1, 24, 16, 16, 4, device='cuda', fp16=True)
