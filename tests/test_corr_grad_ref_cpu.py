"""CPU: tests/corr_grad_ref.py -- the restatement of the correlation's three adjoints (G accumulation, concatenated GEMMs, pool adjoints) --
against float64 autograd through oracle.raft.CorrBlock (build, pooling and lookup, coordinates detached).  The map is (21, 23): levels
21 x 23, 10 x 11, 5 x 5 and 2 x 2, so three of the four pooling steps drop a row or a column; c = 8, b = 2, and two lookups at different
coordinates accumulate into one G.  Agreement to 1e-12 of max |truth| pins the layout of G, the window order and the pooling rule."""
import torch

import corr_grad_ref as ref

H8, W8, C, B = 21, 23, 8, 2


def _case():
    g = torch.Generator().manual_seed(5)
    f1, f2 = torch.randn(B, C, H8, W8, generator=g), torch.randn(B, C, H8, W8, generator=g)
    coords, ds = [], []
    for _ in range(2):
        x = torch.rand(B, 1, H8, W8, generator=g) * (W8 + 11) - 6          # the map plus a margin of 6 pixels
        y = torch.rand(B, 1, H8, W8, generator=g) * (H8 + 11) - 6
        coords.append(torch.cat((x, y), 1))
        ds.append(torch.randn(B, 4 * 81, H8, W8, generator=g))
    return f1, f2, coords, ds


def test_restatement_matches_float64_autograd_through_the_oracle():
    f1, f2, coords, ds = _case()
    assert ref.level_sizes(H8, W8) == [(21, 23), (10, 11), (5, 5), (2, 2)] and ref.volume_cells(H8, W8) == 483 + 110 + 25 + 4
    t1, t2, tG = ref.oracle_grads(f1, f2, coords, ds)
    G = None
    for co, d in zip(coords, ds):
        G = ref.lookup_adjoint(co.double(), d.double(), G)
    d1, d2, _ = ref.build_adjoint(G, f1, f2)
    for name, got, want in (('G', G, tG), ('d_fmap1', d1, t1), ('d_fmap2', d2, t2)):
        err = float((got - want).abs().max() / want.abs().max())
        print(f'{name}: {err:.3e} of max |truth|')
        assert got.shape == want.shape and err < 1e-12, (name, err)


def test_two_lookups_accumulate_and_dropped_rows_get_nothing():
    f1, f2, coords, ds = _case()
    a = ref.lookup_adjoint(coords[0].double(), ds[0].double())
    both = ref.lookup_adjoint(coords[1].double(), ds[1].double(), a.clone())
    assert float((both - a - ref.lookup_adjoint(coords[1].double(), ds[1].double())).abs().max()) < 1e-12
    # a gradient on the pooled levels only reaches nothing in level 0's dropped row (21 is odd) and column (23 is odd)
    dcat = torch.zeros(B, C, ref.volume_cells(H8, W8), dtype=torch.float64)
    dcat[:, :, H8 * W8:] = 1.0
    d2 = ref.pool_adjoints(dcat, H8, W8)
    assert float(d2[:, :, 20].abs().max()) == 0.0 and float(d2[:, :, :, 22].abs().max()) == 0.0 and float(d2[:, :, :20, :22].abs().min()) > 0.0
