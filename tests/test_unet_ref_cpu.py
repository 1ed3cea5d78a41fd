"""CPU: the truth the fused weight heads are held to (tests/unet_ref.py) -- it is the oracle's TinyUNet where the oracle runs, and the
cases of tests/test_gpu_unet_edges.py can tell a right chain from a wrong one: their logits are spread out, a ceil(d / 2) skip crop is far
outside the bar on the odd grids (and indistinguishable on the even ones: why the odd grids are there), and a NaN that reaches the output
only through the 2x2 max pools is visible in the truth and absent under a pool that drops NaN."""
import copy

import pytest
import torch
import torch.nn.functional as F

import unet_ref as ref

EVEN = [(44, 44, 2), (64, 80, 1)]                      # multiples of 4: the reference's crop fits
ODD = [(45, 47, 2), (46, 52, 2), (47, 44, 1)]


def drop_pool(t):
    """2x2 max pool that ignores NaN (what fmaxf does to a window with a finite value in it)."""
    return F.max_pool2d(torch.nan_to_num(t, nan=float('-inf'), posinf=float('inf'), neginf=float('-inf')), 2)


def fmaxf_pool(t):
    """fmaxf(fmaxf(a, b), fmaxf(c, d)) itself: NaN only where all four are."""
    h, w = t.shape[-2] // 2 * 2, t.shape[-1] // 2 * 2
    fm = lambda x, y: torch.where(x.isnan(), y, torch.where(y.isnan(), x, torch.maximum(x, y)))
    return fm(fm(t[..., 0:h:2, 0:w:2], t[..., 0:h:2, 1:w:2]), fm(t[..., 1:h:2, 0:w:2], t[..., 1:h:2, 1:w:2]))


def test_cases_are_the_ones_the_gpu_tests_name():
    assert sorted(ref.PARITY_CASES) == sorted(EVEN + ODD)


@pytest.mark.parametrize('h8,w8,b', EVEN)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_forward_ref_is_the_oracle_where_the_oracle_runs(h8, w8, b, dtype):
    c = ref.case(h8, w8, b)
    got = c['f64' if dtype == torch.float64 else 'f32']
    for hd in range(2):
        with torch.no_grad():
            want = copy.deepcopy(c['onets'][hd]).to(dtype)(c['xs'][hd].to(dtype))
        assert want.dtype == dtype and torch.equal(got[hd][0], want)
        assert torch.equal(got[hd][1], torch.sigmoid(want))


@pytest.mark.parametrize('h8,w8,b', ODD)
def test_oracle_raises_off_multiples_of_four(h8, w8, b):
    c = ref.case(h8, w8, b)
    for hd in range(2):
        with pytest.raises(RuntimeError), torch.no_grad():
            c['onets'][hd](c['xs'][hd])


@pytest.mark.parametrize('h8,w8,b', list(ref.PARITY_CASES))
def test_logits_are_spread_out_and_unsaturated(h8, w8, b):
    """Conditions on the inputs, not tolerances: maps near-constant at 0.5 (the default initialisation) or saturated hide errors."""
    for hd, (logits, _) in enumerate(ref.case(h8, w8, b)['f64']):
        lo, hi = float(logits.min()), float(logits.max())
        print(f'{h8}x{w8} b={b} head {hd}: float64 logits {lo:.2f} .. {hi:.2f}')
        assert hi - lo >= 2.0 and max(-lo, hi) < 8.0


@pytest.mark.parametrize('h8,w8,b', [(45, 47, 2), (46, 52, 2), (44, 44, 2)])
def test_a_ceil_crop_is_caught_on_the_odd_grids_only(h8, w8, b):
    c = ref.case(h8, w8, b)
    ceil = ref.run_cpu(c['nets'], c['xs'], torch.float64, crop='ceil')
    for hd in range(2):
        truth = c['f64'][hd][1]
        d, bar = float((ceil[hd][1] - truth).abs().max()), ref.bar(truth, c['f32'][hd][1])
        print(f'{h8}x{w8} head {hd}: ceil crop moves p by {d:.3e}, bar {bar:.3e}')
        if (h8, w8) == (44, 44):
            assert d == 0.0
        else:
            assert d > 1000.0 * bar


def test_fmaxf_emulations_are_the_max_pool_on_finite_maps():
    t = torch.randn(2, 3, 41, 43, generator=torch.Generator().manual_seed(0))
    assert torch.equal(drop_pool(t), F.max_pool2d(t, 2)) and torch.equal(fmaxf_pool(t), F.max_pool2d(t, 2))


def test_nan_through_the_pools_only_shows_in_the_truth_and_not_under_a_dropping_pool():
    """hidden[0, 100, 2, 2] lies outside both skip crops: its NaN reaches the output through the pools alone."""
    c = ref.case(*ref.NAN_GRID, nan_at=ref.NAN_AT[0])
    for hd in range(2):
        m64, m32 = c['f64'][hd][1].isnan(), c['f32'][hd][1].isnan()
        assert torch.equal(m64, m32)
        assert bool(m32[0].any()) and not bool(m32[0].all()) and not bool(m32[1].any())
    for pool in (drop_pool, fmaxf_pool):
        for _, p in ref.run_cpu(c['nets'], c['xs'], torch.float32, pool=pool):
            assert not bool(p.isnan().any())


def test_nan_inside_the_crops_poisons_its_whole_row():
    c = ref.case(*ref.NAN_GRID, nan_at=ref.NAN_AT[1])
    for hd in range(2):
        m64, m32 = c['f64'][hd][1].isnan(), c['f32'][hd][1].isnan()
        assert torch.equal(m64, m32) and bool(m32[0].all()) and not bool(m32[1].any())


def test_bar_has_a_floor_of_one_float32_spacing():
    z = torch.zeros(3, dtype=torch.float64)
    assert ref.bar(z, z.float()) == 4 * 2.0 ** -23
    assert ref.bar(z, torch.tensor([0.0, 1e-3, 0.0])) == pytest.approx(4e-3, rel=1e-6)
