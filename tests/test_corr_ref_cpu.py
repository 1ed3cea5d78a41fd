"""CPU: tests/corr_ref.py -- the float64 restatement of the correlation's forward -- pinned to oracle.raft.CorrBlock, and the checks of
tests/test_gpu_corr_edges.py shown to bite: each mutant of a float32 CPU evaluation standing in for the GPU is rejected by exactly the check
function the GPU test calls, and the unmutated float32 evaluation passes it."""
import math

import numpy as np
import pytest
import torch

import corr_grad_ref as gref
import corr_ref as ref
from oracle.raft import CorrBlock, bilinear_sampler

SHAPES = [(16, 16), (17, 19), (23, 33)]


def _maps(h8, w8, c=16, b=2, seed=0):
    g = torch.Generator().manual_seed(1000 * h8 + w8 + c + seed)
    return torch.randn(b, c, h8, w8, generator=g), torch.randn(b, c, h8, w8, generator=g)


def _oracle_lookup(blk, coords):
    """CorrBlock.__call__ in the dtype of its pyramid: the same lines without the final cast to float32."""
    r = blk.radius
    b, _, h1, w1 = coords.shape
    dt = blk.corr_pyramid[0].dtype
    co = coords.to(dt).permute(0, 2, 3, 1)
    d = torch.linspace(-r, r, 2 * r + 1, dtype=dt)
    delta = torch.stack(torch.meshgrid(d, d, indexing='ij'), dim=-1).view(1, 2 * r + 1, 2 * r + 1, 2)
    out = [bilinear_sampler(lvl, co.reshape(b * h1 * w1, 1, 1, 2) / 2 ** i + delta).view(b, h1, w1, -1) for i, lvl in enumerate(blk.corr_pyramid)]
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('h8,w8', SHAPES)
@pytest.mark.parametrize('c', [16, 48])
def test_pyramid_matches_the_oracle_in_float64(h8, w8, c):
    f1, f2 = _maps(h8, w8, c)
    blk = CorrBlock(f1.double(), f2.double())
    fix = float(torch.sqrt(torch.tensor(c).float())) / math.sqrt(c)           # the oracle divides by float32(sqrt(c)): a known ratio
    got = ref.pyramid(f1.double(), f2.double())
    assert [tuple(g.shape[2:]) for g in got] == gref.level_sizes(h8, w8)
    cat = gref.f2cat(f2.double())
    off = 0
    for l, (g, want) in enumerate(zip(got, blk.corr_pyramid)):
        want = want.reshape(g.shape) * fix
        assert float((g - want).abs().max()) <= 1e-12 * float(want.abs().max()), l
        # pooling is linear: level l is also fmap1 against the pooled fmap2
        n = g.shape[2] * g.shape[3]
        alt = torch.einsum('bcq,bcp->bqp', f1.double().reshape(2, c, -1), cat[:, :, off:off + n]) / math.sqrt(c)
        assert float((g.reshape(2, h8 * w8, n) - alt).abs().max()) <= 1e-12 * float(want.abs().max()), l
        off += n
    ab = ref.pyramid_abs(f1, f2)
    assert all(bool((a >= g.abs() - 1e-12).all()) for a, g in zip(ab, got))


@pytest.mark.parametrize('h8,w8', SHAPES)
def test_lookup_matches_the_oracle_in_float64(h8, w8):
    f1, f2 = _maps(h8, w8)
    blk = CorrBlock(f1.double(), f2.double())
    co = ref.pin_coords(2, h8, w8, 3 * h8 + w8)
    want = _oracle_lookup(blk, co)
    levels = [lvl.reshape(2, h8 * w8, *lvl.shape[2:]) for lvl in blk.corr_pyramid]
    got = ref.lookup(levels, co, ref.taps(co, 4, np.float64))                  # upstream's sampler, float64 taps
    scale = float(want.abs().max())
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-9 * scale
    flat = want[0].reshape(324, -1)
    assert float(flat[:, [22, 29]].abs().max()) == 0.0 and float(got[0].reshape(324, -1)[:, [22, 29]].abs().max()) == 0.0      # wholly outside
    assert float(flat[:, 36].abs().max()) > 0.0 and int((flat[:81, 36] != 0).sum()) == 1                                       # a corner inside
    # the separable weights of corr_grad_ref give the same windows
    x, y = co[:, 0].reshape(-1).double(), co[:, 1].reshape(-1).double()
    for l, lvl in enumerate(levels):
        Ax, Ay = gref.axis_weights(x / 2 ** l, lvl.shape[3]), gref.axis_weights(y / 2 ** l, lvl.shape[2])
        sep = torch.einsum('qjy,qyx,qix->qij', Ay, lvl.reshape(-1, *lvl.shape[2:]), Ax).reshape(2, h8 * w8, 81).permute(0, 2, 1)
        assert float((sep - got[:, 81 * l:81 * l + 81].reshape(2, 81, -1)).abs().max()) <= 1e-9 * scale, l
    # the float32 taps are the same function up to the rounding of the positions: a weight moves by at most position_error, a product of
    # two weights in [0, 1] by at most px + py + px py, and a window value is four such products times at most max |v|
    got32 = ref.lookup(levels, co)
    worst = max(float(gref.position_error(torch.cat((x, y)) / 2 ** l, max(lvl.shape[2:])).max()) for l, lvl in enumerate(levels))
    assert float((got32 - got).abs().max()) <= 4 * (2 * worst + worst * worst) * float(levels[0].abs().max())
    assert float((got32 - got).abs().max()) > 0.0


def test_float32_taps_take_the_round_trip_not_the_exact_floor():
    """What restating the taps is for: -1e-7 has floor -1, but 2 v / (size - 1) - 1 rounds to -1 and comes back as position 0; 3000 pixels
    outside, NaN, inf and 1e12 give taps that contribute nothing."""
    idx, w0, w1 = ref.tap_floor_f32(np.float32([-1e-7, -0.0, 18.0, np.nan, np.inf, 1e12, -3000.0]), 19, 0)
    assert idx[4].tolist()[:3] == [0, 0, 18] and w0[4].tolist()[:3] == [1.0, 1.0, 1.0] and w1[4].tolist()[:3] == [0.0, 0.0, 0.0]
    assert bool((idx[:, 3:6] == ref.FAR).all()) and not w0[:, 3:6].any() and not w1[:, 3:6].any()
    assert bool(((idx[:, 6] > -3010) & (idx[:, 6] < -2990)).all())
    i64, _, _ = ref.tap_floor(np.float64([-1e-7]), 19, 0, np.float64)
    assert i64[4, 0] == -1


# ------------------------------------------------------------------------------------------------------------------------------ mutants
H8, W8, C = 16, 16, 16


@pytest.fixture(scope='module')
def stand_in():
    """The float32 CPU evaluation standing in for the GPU on the smallest shape: pyramid, coordinates, its own lookup."""
    f1, f2 = _maps(H8, W8, C)
    levels = ref.pyramid(f1, f2)
    assert levels[0].dtype == torch.float32
    co, at, nonfinite = ref.edge_coords(2, H8, W8, 5)
    return f1, f2, levels, co, at, nonfinite


def _lookup32(levels, co, **kw):
    return ref.lookup(levels, co, dtype=torch.float32, **kw)


def test_the_float32_evaluation_passes_every_check(stand_in):
    f1, f2, levels, co, at, nonfinite = stand_in
    ref.check_pyramid(levels, f1, f2, 'stand-in', who='float32 on the CPU')
    ref.check_pooling(levels, 'float32 CPU')
    out = _lookup32(levels, co)
    assert ref.check_lookup(out, levels, co, 'float32 CPU') > 0.0
    assert float(out[0].reshape(324, -1)[:, at[-nonfinite:]].abs().max()) == 0.0
    # fp16 features: the truth is the correlation of the rounded maps
    h1, h2 = f1.half().float(), f2.half().float()
    ref.check_pyramid(ref.pyramid(h1, h2), h1, h2, 'stand-in, half-rounded maps', who='float32 on the CPU')


def test_mutant_two_neighbouring_cells_swapped(stand_in):
    f1, f2, levels, *_ = stand_in
    bad = [l.clone() for l in levels]
    bad[0][1, 77, 9, [5, 6]] = levels[0][1, 77, 9, [6, 5]]                       # (columns of two different 2x2 blocks)
    with pytest.raises(AssertionError):
        ref.check_pyramid(bad, f1, f2)
    with pytest.raises(AssertionError):
        ref.check_pooling(bad)                                                   # level 1 is no longer the mean of this level 0


def test_mutant_level_2_pooled_from_shifted_rows(stand_in):
    f1, f2, levels, *_ = stand_in
    bad = [l.clone() for l in levels]
    bad[2] = torch.nn.functional.avg_pool2d(torch.roll(levels[1], -1, 2), 2, stride=2)
    with pytest.raises(AssertionError):
        ref.check_pyramid(bad, f1, f2)
    with pytest.raises(AssertionError):
        ref.check_pooling(bad)


def test_mutant_a_padding_read_returns_one(stand_in):
    _, _, levels, co, at, _ = stand_in
    q = at[3]                                                                    # the plant (2.5, 8.5): its taps 0 and 1 read columns -2 .. 0
    assert tuple(co[0, :, q // W8, q % W8].tolist()) == (2.5, 8.5)
    def hook(l, P):
        if l == 0:
            assert float(P[q, 9, 0]) == 0.0
            P[q, 9, 0] = 1.0                                                     # row 8, the column left of the map
    out = _lookup32(levels, co, pad_hook=hook)
    good = _lookup32(levels, co)
    assert int((out != good).sum()) > 0 and int((out != good).sum()) <= 2 * 2
    with pytest.raises(AssertionError):
        ref.check_lookup(out, levels, co)


def test_mutant_one_tap_deviates(stand_in):
    _, _, levels, co, at, _ = stand_in
    tl = ref.taps(co)
    q = 16 * 7 + 9                                                               # an unplanted query of row 0
    assert q not in at and tl[1][0][0][3, q] != ref.FAR
    tl[1][0][0][3, q] += 1                                                       # level 1, x axis, tap 3: dev flipped
    out = _lookup32(levels, co, tap_list=tl)
    assert 0 < int((out != _lookup32(levels, co)).sum()) <= 9
    with pytest.raises(AssertionError):
        ref.check_lookup(out, levels, co)


def test_mutant_window_transposed(stand_in):
    _, _, levels, co, *_ = stand_in
    out = _lookup32(levels, co)
    out = out.reshape(2, 4, 9, 9, H8, W8).transpose(2, 3).reshape(2, 324, H8, W8)
    with pytest.raises(AssertionError):
        ref.check_lookup(out, levels, co)
