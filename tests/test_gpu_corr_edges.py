"""GPU: the correlation pyramid's build and window lookup (csrc/corr.hip; ops.CorrPyramid) at their edges, element by element against the
float64 restatement tests/corr_ref.py, whose module docstring derives every bound used here from the kernels' arithmetic:

  build, level l:      K_l u sum |a| |b| / sqrt(c), pooled;  K_l = c + 4 + 3 l  (the c-term f32 chain, the scale's three roundings, three per pool)
  pooling alone:       ((1 + u)^3 - 1) mean |four cells|, level l against the GPU's own level l - 1
  lookup:              ((1 + u)^4 - 1) sum |w_x| |w_y| |v| against the float64 window of the GPU's own pyramid at the float32-restated taps

The taps are restated in float32 (compared exactly with CorrPyramid.taps), so no comparison leaves an element out; tests/test_corr_ref_cpu.py
pins the restatement to the oracle and shows that each check rejects a mutant.

Shapes (b = 2): (16,16) the smallest legal geometry, level 3 is 2 x 2, one patch per band, two query tiles, fmap1 through the permute pass;
(16,32) fmap1 read in place; (17,19) a last band of 1 row, a last patch of 3 columns (fewer than the skew of 7), a last group of 3 queries, 51
groups, levels 8x9, 4x4, 2x2 (a dropped row, then a dropped column); (23,33) a last patch of 1 column, levels 11x16, 5x8, 2x4 (a dropped row
at three levels in a row), a different row padding per level; (41,37) for the band walk only."""
import pytest
import torch

import corr_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MAPS = [(16, 16), (16, 32), (17, 19), (23, 33)]


def _maps(b, c, h8, w8, seed=0):
    g = torch.Generator().manual_seed(100000 * seed + 1000 * h8 + 10 * w8 + c)
    return torch.randn(b, c, h8, w8, generator=g), torch.randn(b, c, h8, w8, generator=g)


def _build(ops, f1, f2, fill=None, **kw):
    b, _, h8, w8 = f1.shape
    pyr = ops.CorrPyramid(b, h8, w8, device=DEV)
    if fill is not None:
        pyr.buf.fill_(fill)
    return pyr.build(f1.to(DEV), f2.to(DEV), **kw)


def _guarded_out(b, h8, w8):
    n, pad = b * 324 * h8 * w8, 4096
    buf = torch.full((n + 2 * pad,), 7.25, device=DEV)
    return buf, buf[pad:pad + n].view(b, 324, h8, w8), pad


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


# -------------------------------------------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize('h8,w8,c', [(16, 16, 256), (16, 32, 256), (17, 19, 16), (17, 19, 48), (17, 19, 256), (23, 33, 32)])
def test_build_against_float64_per_element(rpe, h8, w8, c):
    """c = 16 is one 16-channel step of the K loop, 48 an odd number of steps through its ring of buffers, 256 the full depth."""
    from rpe_amd import ops
    f1, f2 = _maps(2, c, h8, w8)
    pyr = _build(ops, f1, f2)
    got = ref.dense_levels(pyr)
    tag = f'{h8}x{w8} c={c}'
    ref.check_pyramid(got, f1, f2, tag, beside=ref.pyramid(f1, f2))
    ref.check_pooling(got, tag)
    # two runs give the same bits; row 0 of the b = 2 build is the b = 1 build
    again, one = _build(ops, f1, f2), _build(ops, f1[:1], f2[:1])
    for l in range(4):
        full = pyr.export_level(l)
        assert torch.equal(again.export_level(l), full) and torch.equal(one.export_level(l), full[:h8 * w8]), l


@pytest.mark.parametrize('h8,w8', [(17, 19), (16, 16)])
def test_fp16_feature_build_against_float64_per_element(rpe, h8, w8):
    """fp16_features=True: the truth is the float64 correlation of the half-rounded maps; their products are exact in f32, so the build's
    bound keeps its form."""
    from rpe_amd import ops
    f1, f2 = _maps(2, 256, h8, w8, seed=1)
    h1, h2 = f1.half().float(), f2.half().float()
    got = ref.dense_levels(_build(ops, f1, f2, fp16_features=True))
    tag = f'{h8}x{w8} fp16 features'
    ref.check_pyramid(got, h1, h2, tag, beside=ref.pyramid(h1, h2))
    ref.check_pooling(got, tag)


# ----------------------------------------------------------------------------------------------------------------------- the carry walk
def _geometry(b, h8, w8):
    """(band workgroups of a build launch, bytes of the four levels): make_geom of csrc/corr.hip.  A row of 8-query groups is gx = ceil(w8 / 8),
    the queries in group order are padded to mp = 128 ceil(8 gx h8 / 128), the bands are nbands = ceil(h8 / 8); level l holds, per pair and
    group, h_l rows of wp_l = 4 ceil((w_l + sk_l) / 4) slots of 8 floats, sk_l = max(7 >> l, 1)."""
    gx = (w8 + 7) // 8
    mp = (gx * h8 * 8 + 127) // 128 * 128
    nbands, npx = (h8 + 7) // 8, (w8 + 15) // 16
    pyr_bytes = sum(b * gx * h8 * hl * ((wl + max(7 >> l, 1) + 3) // 4 * 4) * 32 for l, (hl, wl) in enumerate(ref.level_sizes(h8, w8)))
    scratch = b * 256 * (mp + nbands * npx * 128) * 4
    return nbands * (mp // 128) * b, pyr_bytes, scratch


@pytest.mark.parametrize('h8,w8,b', [(17, 19, 342), (41, 37, 53)])
def test_band_walk_with_carry_at_ragged_shapes(rpe, h8, w8, b):
    """rpe_corr_build takes k_corr_build<true> -- a workgroup walks a band's patches, level 0 through the LDS carry -- when
    nbands (mp / 128) b >= 4096, else one workgroup per patch.  (17,19): nbands = 3, mp = 128 ceil(408 / 128) = 512, 3 * 4 * 342 = 4104;
    (41,37): nbands = 6, mp = 128 ceil(1640 / 128) = 1664, 6 * 13 * 53 = 4134; with b = 2 both are far below.  Asserted from the same formula.
    Neither shape has whole bands, whole patches (3 and 5 columns are left, fewer than the skew) or whole groups.  The first, the middle and
    the last pair of the big build equal b = 2 builds of the same pairs bit for bit, level by level and through a border-heavy lookup, and
    keep the float64 bound; on (17,19) the big build is repeated into a pyramid region filled with 0xFF bytes (every float a NaN)."""
    from rpe_amd import ops
    c = 32
    wgs, pyr_bytes, scratch = _geometry(b, h8, w8)
    assert wgs >= 4096 > _geometry(2, h8, w8)[0], wgs
    assert wgs == {(17, 19): 4104, (41, 37): 4134}[(h8, w8)]
    f1, f2 = _maps(b, c, h8, w8, seed=2)
    rows = [0, b // 2, b - 1]
    nq = h8 * w8
    big = ops.CorrPyramid(b, h8, w8, device=DEV)
    assert big.buf.numel() == pyr_bytes + scratch + 256                      # the layout arithmetic above is the library's
    d1, d2 = f1.to(DEV), f2.to(DEV)
    big.build(d1, d2)
    co3, _, _ = ref.edge_coords(3, h8, w8, 7)
    cb = torch.zeros(b, 2, h8, w8, device=DEV)
    cb[rows] = co3.to(DEV)
    levels_big = []
    for l in range(4):
        d = big.export_level(l)
        levels_big.append(d.reshape(b, nq, *d.shape[1:])[rows].clone())
        del d
    out_big = big.lookup(cb)[rows].clone()
    assert bool(torch.isfinite(out_big).all())
    for pair in ((0, 1), (1, 2)):
        sel = [rows[pair[0]], rows[pair[1]]]
        small = _build(ops, f1[sel], f2[sel])
        for l in range(4):
            ls = small.export_level(l)
            assert torch.equal(ls.reshape(2, nq, *ls.shape[1:]), levels_big[l][list(pair)]), (pair, l)
        assert torch.equal(small.lookup(co3[list(pair)].to(DEV)), out_big[list(pair)]), pair
    got = [x.cpu().double() for x in levels_big]
    tag = f'{h8}x{w8} b={b} band walk'
    ref.check_pyramid(got, f1[rows], f2[rows], tag, beside=ref.pyramid(f1[rows], f2[rows]))
    ref.check_pooling(got, tag)
    ref.check_lookup(out_big, got, co3, tag)
    if (h8, w8) == (17, 19):
        big.buf[:pyr_bytes].fill_(0xFF)
        big.build(d1, d2)
        again = big.lookup(cb)[rows]
        assert bool(torch.isfinite(again).all()) and torch.equal(again, out_big)
        for l in range(4):
            d = big.export_level(l)
            assert torch.equal(d.reshape(b, nq, *d.shape[1:])[rows], levels_big[l]), l
            del d
    del big, out_big, levels_big, d1, d2, cb
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- every slot is written
@pytest.mark.parametrize('fp16', [False, True])
@pytest.mark.parametrize('h8,w8', MAPS)
def test_build_writes_every_slot_the_lookup_reads(rpe, h8, w8, fp16):
    """The layout's zero slots (x' < sk, the columns past w_l, the row padding up to wp_l) are grid_sample's zero padding, and export_level
    never reads them.  Built into a buffer of 0xFF bytes -- every float a NaN -- the pyramid gives a finite lookup at the border coordinates,
    the same bits as a build into zeros; so does a second, different pair built over the first."""
    from rpe_amd import ops
    kw = dict(fp16_features=True) if fp16 else {}
    (a1, a2), (b1, b2) = _maps(2, 32, h8, w8, seed=3), _maps(2, 32, h8, w8, seed=4)
    co = ref.edge_coords(2, h8, w8, 9)[0].to(DEV)
    want_a = _build(ops, a1, a2, fill=0, **kw).lookup(co)
    want_b = _build(ops, b1, b2, fill=0, **kw).lookup(co)
    assert not torch.equal(want_a, want_b)
    pyr = _build(ops, a1, a2, fill=0xFF, **kw)
    got_a = pyr.lookup(co)
    assert bool(torch.isfinite(got_a).all()) and torch.equal(got_a, want_a)
    got_b = pyr.build(b1.to(DEV), b2.to(DEV), **kw).lookup(co)
    assert bool(torch.isfinite(got_b).all()) and torch.equal(got_b, want_b)


# ------------------------------------------------------------------------------------------------------------------------------- lookup
def _check_taps(pyr, co):
    b, nq = co.shape[0], co.shape[2] * co.shape[3]
    x0, y0 = pyr.taps(co.to(DEV))
    x0, y0 = x0.cpu(), y0.cpu()
    for l, (X, Y) in enumerate(ref.taps(co)):
        for got, T in ((x0, X), (y0, Y)):
            assert torch.equal(got[:, l], torch.from_numpy(T[0]).reshape(9, b, nq).permute(1, 0, 2)), l


@pytest.mark.parametrize('h8,w8', MAPS)
def test_lookup_against_float64_of_the_gpu_pyramid(rpe, h8, w8):
    """Random targets over the map plus a margin of 6 and corr_ref.edge_plants: integers at every level, half-integers, -0.0, -1e-7, the last
    row and column, centres from the last tap column inside to nothing inside on each axis and on both (only a corner inside), NaN, inf, 1e12
    and -3000.  Every output within the lookup's bound -- exactly zero where nothing is inside --, the taps equal to the restatement, the
    output written into a view between untouched canaries, twice the same bits, and row 0 equal to the b = 1 call."""
    from rpe_amd import ops
    f1, f2 = _maps(2, 32, h8, w8, seed=5)
    pyr = _build(ops, f1, f2)
    levels = ref.dense_levels(pyr)
    co, at, nonfinite = ref.edge_coords(2, h8, w8, 11 + h8)
    _check_taps(pyr, co)
    buf, out, pad = _guarded_out(2, h8, w8)
    assert pyr.lookup(co.to(DEV), out=out) is out
    assert bool((buf[:pad] == 7.25).all()) and bool((buf[-pad:] == 7.25).all())
    ref.check_lookup(out, levels, co, f'{h8}x{w8}')
    assert float(out[0].reshape(324, -1)[:, at[-nonfinite:]].abs().max()) == 0.0
    assert torch.equal(pyr.lookup(co.to(DEV)), out)
    one = _build(ops, f1[:1], f2[:1]).lookup(co[:1].to(DEV))
    assert torch.equal(one[0], out[0])


def _rough_groups(co, h8, w8):
    """Plants whole groups (8 queries that are neighbours in x) of batch row 1 and returns {name: (group index, rounds expected at level 0)}.
    At level 0 lane k's window starts at skewed column sx = floor(x - 4) + 7 - k and row floor(y - 4); a round serves the lanes within one row
    of the topmost pending one whose sx is at most 5 right of the leftmost of those (11 columns in a 16-slot box, 11 rows in a 12-row box)."""
    gx, k = (w8 + 7) // 8, torch.arange(8.0)
    x, y = co[1, 0], co[1, 1]
    groups = {}

    def put(name, row, g, xs, ys, rounds):
        n = min(8, w8 - 8 * g)
        x[row, 8 * g:8 * g + n], y[row, 8 * g:8 * g + n] = xs[:n], ys[:n]
        groups[name] = (row * gx + g, rounds)
    fit, nofit = torch.tensor([0.0, 5, 0, 5, 2, 3, 1, 4]), torch.tensor([0.0, 6, 0, 5, 2, 3, 1, 4])
    put('eight distant places', 1, 0, torch.where(k % 2 == 0, 2.5, w8 - 3.5), 0.5 + 2 * k, 8)
    put('two clusters', 2, 1, torch.where(k < 4, 3.5 + k, w8 - 8.5 + k), torch.where(k < 4, 2.5, 11.5), 2)
    put('x spread fits the 16 slots', 3, 0, 2.5 + k + fit, torch.full((8,), 6.5), 1)
    put('x spread of one more', 4, 1, 2.5 + k + nofit, torch.full((8,), 6.5), 2)
    put('y spread fits the 12 rows', 5, 0, 3.5 + k, 4.5 + (fit > 2).float(), 1)
    put('y spread of one more', 6, 1, 3.5 + k, 4.5 + (fit > 2).float() + (k == 2).float() * 2, 2)
    if w8 % 8:
        put('ragged last group', 7, gx - 1, torch.tensor([2.5, 12.5, 3.5, 0, 0, 0, 0, 0]), torch.full((8,), 5.5), 2)
    return groups


@pytest.mark.parametrize('h8,w8', [(16, 32), (17, 19)])
def test_rough_flow_inside_a_group(rpe, h8, w8):
    """Windows of one group that do not fit one 12 x 16 staging box are served by further rounds with the box re-anchored: the planted groups
    take the rounds the rule gives them (CorrPyramid.rounds), and every output keeps the lookup's bound.  Where rows are whole groups the
    fused lookup + convc1 stays bit-identical to lookup followed by conv1x1 at these coordinates."""
    from rpe_amd import ops
    f1, f2 = _maps(2, 32, h8, w8, seed=6)
    pyr = _build(ops, f1, f2)
    co = ref.edge_coords(2, h8, w8, 13)[0]
    groups = _rough_groups(co, h8, w8)
    cod = co.to(DEV)
    rounds = pyr.rounds(cod)[0].cpu()
    for name, (g, want) in groups.items():
        got = int(rounds[1, 0, g])
        print(f'{h8}x{w8} {name}: {got} round(s) at level 0')
        assert got == 1 if want == 1 else got > 1, (name, got)
        assert got == want, (name, got, want)
    _check_taps(pyr, co)
    out = pyr.lookup(cod)
    ref.check_lookup(out, ref.dense_levels(pyr), co, f'{h8}x{w8} rough flow')
    if w8 % 8 == 0:
        g = torch.Generator().manual_seed(h8)
        wt, bias = (torch.randn(256, 324, 1, 1, generator=g) * 0.05).to(DEV), (torch.randn(256, generator=g) * 0.5).to(DEV)
        packed = ops.PackedLookupConv(wt, bias)
        for relu in (True, False):
            want = ops.conv1x1(out, ops.PackedConv1x1(wt, bias), ops.CONV_RELU if relu else ops.CONV_LINEAR, torch.empty(2, 256, h8, w8, device=DEV))
            got = pyr.lookup_conv1x1(cod, packed, torch.empty(2, 256, h8, w8, device=DEV), relu=relu)
            assert bool(torch.isfinite(want).all()) and _same(got, want), relu
