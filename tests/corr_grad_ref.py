"""Test infrastructure: plain-torch restatement of the three adjoints of csrc/corr_backward.hip -- the accumulation of the gradient volume G
(the window lookup's adjoint), the two concatenated GEMMs and the pool adjoints (the pyramid build's adjoint) -- in any dtype, with the
absolute-value sums the GPU tests' error bounds are made of.  Pinned to autograd through oracle.raft.CorrBlock by
tests/test_corr_grad_ref_cpu.py.

G (b, h8 w8, S), S = sum_l h_l w_l with (h_l, w_l) = (h8 >> l, w8 >> l): row p = the four levels' maps of query p one after the other, each
row-major.  Window channel l 81 + i 9 + j samples level l at (x / 2^l + i - 4, y / 2^l + j - 4): upstream's transposed order."""
import torch
import torch.nn.functional as F

R, WIN = 4, 9
U = 2.0 ** -24                     # unit roundoff of float32


def level_sizes(h8, w8, levels=4):
    return [(h8 >> l, w8 >> l) for l in range(levels)]


def volume_cells(h8, w8, levels=4):
    return sum(h * w for h, w in level_sizes(h8, w8, levels))


def tap_positions(c, dtype=None):
    """(n, 9): c + (i - 4) for i = 0 .. 8."""
    c = c if dtype is None else c.to(dtype)
    return c[:, None] + torch.arange(-R, R + 1, dtype=c.dtype)[None, :]


def axis_weights(c, size):
    """A (n, 9, size): A[q, i, p] = the bilinear weight of tap i of query q on pixel p of an axis of ``size`` pixels; pixels outside the axis
    are dropped (grid_sample's zero padding)."""
    pos = tap_positions(c)
    f = torch.floor(pos)
    w1 = pos - f
    A = torch.zeros(*pos.shape, size, dtype=c.dtype)
    for idx, w in ((f, 1 - w1), (f + 1, w1)):
        ok = (idx >= 0) & (idx < size)
        A.scatter_add_(2, idx.clamp(0, size - 1).long()[..., None], (w * ok)[..., None])
    return A


def position_error(c, size):
    """(n, 9): a bound on |float32 tap position - exact tap position| for the forward's arithmetic (csrc/sampling.h rt_pos after one rounded
    addition): with v = c + (i - 4), s = size - 1 and u = 2^-24, the rounded steps are v (u |v|), 2 v / s (u |v| in position units), - 1
    (u (|v| + s / 2)), + 1 (u |v|) and * s (u |v|), first order u (5 |v| + s / 2); u (6 |v| + size) covers the second order."""
    return U * (6 * tap_positions(c.double()).abs() + size)


def axis_weight_errors(c, size):
    """D (n, 9, size), float64: a bound on |float32 weight - exact weight| of tap i on pixel p.  Both weights are exact functions of the float32
    position (pos - floor, floor + 1 - pos: differences of neighbours), so each moves by at most the position's error; the pixels are the
    two of the exact position, or the three a position within its error of an integer can touch."""
    pos = tap_positions(c.double())
    d = position_error(c, size)
    lo, hi = torch.floor(pos - d), torch.floor(pos + d) + 1
    D = torch.zeros(*pos.shape, size, dtype=torch.float64)
    for k in range(3):
        idx = lo + k
        ok = (idx <= hi) & (idx >= 0) & (idx < size)
        D.scatter_add_(2, idx.clamp(0, size - 1).long()[..., None], (d * ok)[..., None])
    return D


def _window(d_corr, l):
    b, _, h8, w8 = d_corr.shape
    return d_corr[:, l * WIN * WIN:(l + 1) * WIN * WIN].reshape(b, WIN, WIN, h8 * w8).permute(0, 3, 1, 2).reshape(b * h8 * w8, WIN, WIN)


def lookup_adjoint(coords, d_corr, G=None, levels=4):
    """G += the adjoint of one window lookup at coords (b,2,h8,w8) from d_corr (b, levels 81, h8, w8); dtype = d_corr's."""
    b, _, h8, w8 = coords.shape
    nq, dt = h8 * w8, d_corr.dtype
    if G is None:
        G = torch.zeros(b, nq, volume_cells(h8, w8, levels), dtype=dt)
    x, y = coords[:, 0].reshape(-1).to(dt), coords[:, 1].reshape(-1).to(dt)
    off = 0
    for l, (hl, wl) in enumerate(level_sizes(h8, w8, levels)):
        Ax, Ay = axis_weights(x / 2 ** l, wl), axis_weights(y / 2 ** l, hl)
        G[:, :, off:off + hl * wl] += torch.einsum('qjy,qij,qix->qyx', Ay, _window(d_corr, l), Ax).reshape(b, nq, hl * wl)
        off += hl * wl
    return G


def lookup_adjoint_bounds(coords, d_corr, levels=4):
    """(sum |w| |d|, fraction error) per cell of G for ONE lookup, float64: the sum of the absolute terms with exact weights, and the bound
    on what the forward's float32 tap positions change, sum |d| (Dx |wy| + |wx| Dy + Dx Dy)."""
    b, _, h8, w8 = coords.shape
    nq = h8 * w8
    x, y = coords[:, 0].reshape(-1).double(), coords[:, 1].reshape(-1).double()
    S, E = [], []
    for l, (hl, wl) in enumerate(level_sizes(h8, w8, levels)):
        Ax, Ay = axis_weights(x / 2 ** l, wl), axis_weights(y / 2 ** l, hl)
        Dx, Dy = axis_weight_errors(x / 2 ** l, wl), axis_weight_errors(y / 2 ** l, hl)
        d = _window(d_corr.double(), l).abs()
        es = lambda ay, ax: torch.einsum('qjy,qij,qix->qyx', ay, d, ax).reshape(b, nq, hl * wl)
        S.append(es(Ay, Ax))
        E.append(es(Ay, Dx) + es(Dy, Ax) + es(Dy, Dx))
    return torch.cat(S, 2), torch.cat(E, 2)


def f2cat(fmap2, levels=4):
    """(b, c, S): fmap2 followed by its successively 2x2-pooled copies (floor), each row-major."""
    b, c = fmap2.shape[:2]
    out, t = [], fmap2
    for l in range(levels):
        if l:
            t = F.avg_pool2d(t, 2, stride=2)
        out.append(t.reshape(b, c, -1))
    return torch.cat(out, 2)


def pool_adjoints(dcat, h8, w8, levels=4):
    """d_fmap2 (b,c,h8,w8) from dF2cat (b,c,S): the levels applied from the last down to 0, a quarter of each value to the four cells its pool
    covered and nothing to a dropped row or column."""
    b, c = dcat.shape[:2]
    sizes = level_sizes(h8, w8, levels)
    offs = [sum(h * w for h, w in sizes[:l]) for l in range(levels + 1)]
    t = None
    for l in reversed(range(levels)):
        hl, wl = sizes[l]
        cur = dcat[:, :, offs[l]:offs[l + 1]].reshape(b, c, hl, wl).clone()
        if t is not None:
            up = 0.25 * t.repeat_interleave(2, 2).repeat_interleave(2, 3)
            cur[:, :, :up.shape[2], :up.shape[3]] += up
        t = cur
    return t


def build_adjoint(G, fmap1, fmap2, levels=4):
    """(d_fmap1, d_fmap2, dF2cat) of the pyramid build from G (b, h8 w8, S); dtype = G's."""
    b, c, h8, w8 = fmap1.shape
    dt = G.dtype
    s = c ** -0.5
    Fc = f2cat(fmap2.to(dt), levels)
    d1 = s * torch.einsum('bcs,bqs->bcq', Fc, G).reshape(b, c, h8, w8)
    dcat = s * torch.einsum('bcq,bqs->bcs', fmap1.to(dt).reshape(b, c, -1), G)
    return d1, pool_adjoints(dcat, h8, w8, levels), dcat


def build_adjoint_abs(G, fmap1, fmap2, levels=4):
    """The same three with every product replaced by its absolute value, float64: sum |a| |b| of each result's plain sum of products."""
    return build_adjoint(G.double().abs(), fmap1.double().abs(), fmap2.double().abs(), levels)


def oracle_grads(fmap1, fmap2, coords_list, d_list, dtype=torch.float64):
    """(d_fmap1, d_fmap2, G per level as autograd sees it) of sum_k <CorrBlock(fmap1, fmap2)(coords_k), d_k> by autograd through
    oracle.raft.CorrBlock, coordinates detached.  The oracle divides by float32(sqrt(c)), the restatement by the exact root: the results are
    rescaled by that known ratio."""
    import math
    from oracle.raft import CorrBlock
    f1, f2 = fmap1.to(dtype).requires_grad_(True), fmap2.to(dtype).requires_grad_(True)
    blk = CorrBlock(f1, f2)
    # G: the lookups alone, on leaf copies of the levels (a level's gradient inside the whole graph would include what the pooled levels hand down)
    alone = CorrBlock.__new__(CorrBlock)
    alone.num_levels, alone.radius = blk.num_levels, blk.radius
    alone.corr_pyramid = [lvl.detach().requires_grad_(True) for lvl in blk.corr_pyramid]
    for k, one in enumerate((blk, alone)):
        loss = 0
        for co, d in zip(coords_list, d_list):
            w = one(co.to(dtype).detach())                              # (the oracle returns float32: the cast's adjoint is the identity)
            loss = loss + (w.to(dtype) * d.to(dtype)).sum()
        loss.backward()
    c = fmap1.shape[1]
    fix = float(torch.sqrt(torch.tensor(c).float())) / math.sqrt(c)
    b, _, h8, w8 = fmap1.shape
    G = torch.cat([lvl.grad.reshape(b, h8 * w8, -1) for lvl in alone.corr_pyramid], 2)
    return f1.grad * fix, f2.grad * fix, G
