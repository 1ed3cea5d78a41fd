"""Test infrastructure: plain torch / numpy restatement of the FORWARD of csrc/corr.hip -- the pyramid build (level 0 = fmap1^T fmap2 / sqrt(c),
level l = the 2x2 mean of level l - 1 with floor) and the radius-4 window lookup --, the absolute-value sums the GPU tests' bounds are made of,
the checks themselves (tests/test_gpu_corr_edges.py and the mutation tests of tests/test_corr_ref_cpu.py call the same functions) and the
coordinate sets.  Sizes, weights-by-axis and unit roundoff come from tests/corr_grad_ref.py.

The discrete decisions are the kernel's own.  ``tap_floor`` restates csrc/sampling.h rt_pos and csrc/corr_taps.h make_taps one rounded
operation at a time in a numpy dtype: in float32 it yields the floor index and both weights of every tap bit for bit as the kernel forms
them (CorrPyramid.taps returns the kernel's indices: compared exactly on the GPU), in float64 it is upstream's sampler in float64 (pinned to
oracle.raft.CorrBlock to 1e-9).  ``lookup`` evaluates a window from such taps, by default the float32 ones cast to float64, so no coordinate
has to be kept away from an integer: what is left between it and the GPU is the bilinear arithmetic alone.

Bounds, u = 2^-24, all per element, none fitted to what the GPU returns.

Build, level 0.  k_corr_build adds the c products of an element in one f32 chain of fused multiply-adds (v_mfma_f32_32x32x2_f32; the fp16
build adds exact products of half values in f32): a term passes at most c roundings.  The result is multiplied by
scale = 1.0f / sqrtf((float)c): the root, the quotient and the product round once each, 3 more (none for c = 16 or 256, counted anyway).
(1 + u)^(c + 3) - 1 <= (c + 4) u for every c <= 256, so |level 0 - truth| <= K0 u sum |a| |b| / sqrt(c) with K0 = c + 4.
Build, level l.  build_epilogue pools (((s0 + s1) + s2) + s3) * 0.25f: three rounded additions, the product by a power of two is exact.  The
error of a pooled cell is the mean of its four cells' errors plus at most ((1 + u)^3 - 1) times the mean of their absolute values, which is
itself at most (1 + K u) times the pooled absolute sum: K_l = c + 4 + 3 l, |level l - truth| <= K_l u pyramid_abs_l.
Pooling alone.  Level l of a pyramid against the float64 mean of ITS OWN level l - 1: ((1 + u)^3 - 1) mean |four cells|.

Lookup.  consume_pass forms a window row as A[i] a0 + A[i + 1] a1 (+ A[i + 2] a2, where one of the three weights is an exact zero whose
product is an exact zero and whose addition changes nothing) and the output as hm2 w0 + hm1 w1 (+ hc w2, likewise): a term w_x w_y v passes
one rounded product and one rounded addition per axis, or fewer where the compiler fuses them -- four roundings, with weights that are exactly
``tap_floor``'s float32 ones.  |lookup - truth| <= ((1 + u)^4 - 1) sum |w_x| |w_y| |v|.  Where that sum is zero (a window wholly outside its
map, a non-finite or far coordinate) the bound is zero: the output must be exactly 0.0."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from corr_grad_ref import R, U, WIN, level_sizes

POOL_K = (1 + U) ** 3 - 1
LOOKUP_K = (1 + U) ** 4 - 1
FAR = -1000000                      # the index of a tap that contributes nothing (safe_floor)


# ------------------------------------------------------------------------------------------------------------------------------ pyramid
def pyramid(f1, f2, levels=4):
    """[(b, h8 w8, h_l, w_l)] in the dtype of f1: all-pairs correlation / sqrt(c), then F.avg_pool2d level after level (floor: an odd last
    row or column is dropped)."""
    b, c, h8, w8 = f1.shape
    corr = torch.einsum('bcq,bcp->bqp', f1.reshape(b, c, -1), f2.reshape(b, c, -1)) / math.sqrt(c)
    out = [corr.reshape(b, h8 * w8, h8, w8)]
    for _ in range(1, levels):
        out.append(F.avg_pool2d(out[-1], 2, stride=2))
    return out


def pyramid_abs(f1, f2, levels=4):
    """The same with every product replaced by its absolute value: sum |a| |b| / sqrt(c), pooled the same way; float64."""
    return pyramid(f1.double().abs(), f2.double().abs(), levels)


def build_k(c, level):
    return c + 4 + 3 * level


def dense_levels(pyr, rows=None):
    """The levels of an ops.CorrPyramid as [(b, nq, h_l, w_l)] float64 CPU tensors; ``rows``: these batch rows only."""
    out = []
    for l in range(pyr.levels):
        d = pyr.export_level(l)
        d = d.reshape(pyr.b, pyr.h8 * pyr.w8, *d.shape[1:])
        out.append((d if rows is None else d[rows]).cpu().double())
        del d
    return out


def check_pyramid(got, f1, f2, tag='', beside=None, who='GPU'):
    """Every level of ``got`` ([(b, nq, h_l, w_l)]) within K_l u pyramid_abs_l of the float64 pyramid of (f1, f2), element by element.
    Prints max err / bound per level, beside the figure of ``beside`` (a float32 CPU evaluation) where given; returns the figures."""
    c = f1.shape[1]
    truth, ab = pyramid(f1.double(), f2.double(), len(got)), pyramid_abs(f1, f2, len(got))
    figures = []
    for l, (g, t, a) in enumerate(zip(got, truth, ab)):
        assert tuple(g.shape) == tuple(t.shape), (tag, l, tuple(g.shape), tuple(t.shape))
        bound = build_k(c, l) * U * a
        ratio = lambda x: float(((x.double() - t).abs() / bound.clamp_min(1e-300)).max())
        r, rs = ratio(g), (ratio(beside[l]) if beside is not None else float('nan'))
        print(f'{tag} build level {l} {tuple(t.shape[2:])} K = {build_k(c, l)}: max err / bound {who} {r:.3f}' + (f'  float32 on the CPU {rs:.3f}' if beside is not None else ''))
        figures.append((r, rs))
        assert bool(((g.double() - t).abs() <= bound).all()), (tag, 'level', l, r)
    return figures


def check_pooling(got, tag=''):
    """Level l of ``got`` against the float64 2x2 mean of ITS OWN level l - 1: within the pooling's three roundings of the mean of the four
    absolute values, element by element."""
    figures = []
    for l in range(1, len(got)):
        src = got[l - 1].double()
        t, a = F.avg_pool2d(src, 2, stride=2), F.avg_pool2d(src.abs(), 2, stride=2)
        assert tuple(got[l].shape) == tuple(t.shape), (tag, l)
        err, bound = (got[l].double() - t).abs(), POOL_K * a
        r = float((err / bound.clamp_min(1e-300)).max())
        print(f'{tag} pooling {l - 1} -> {l}: max err / bound {r:.3f}')
        figures.append(r)
        assert bool((err <= bound).all()), (tag, 'pooling to level', l, r)
    return figures


# --------------------------------------------------------------------------------------------------------------------------------- taps
def tap_floor(c, size, level, dtype=np.float32):
    """(idx int32, w0, w1), each (9, *c.shape): tap i of an axis of ``size`` pixels at level ``level`` reads pixel idx[i] with weight w0[i] and
    pixel idx[i] + 1 with weight w1[i].  csrc/sampling.h rt_pos after csrc/corr_taps.h's rounded centroid + delta, every operation rounded
    in ``dtype``; a position that is not finite or not inside (-1e6, 1e6), and every tap of an axis on which floor(pos_i) - i spreads by more
    than one or reaches below -500000, gives idx = FAR and two zero weights (make_taps' ``bad``)."""
    dt = np.dtype(dtype).type
    c = np.asarray(c, dtype=dtype)
    one, two, sm1 = dt(1), dt(2), dt(size - 1)
    with np.errstate(all='ignore'):
        cl = c / dt(2 ** level)                                           # coords / 2^l: exact
        d = np.arange(-R, R + 1).astype(dtype).reshape(WIN, *[1] * c.ndim)
        v = cl[None] + d
        g = two * v / sm1 - one
        pos = ((g + one) / two) * sm1
        ok = (pos > dt(-1.0e6)) & (pos < dt(1.0e6))
        pf = np.where(ok, np.floor(pos), dt(-1.0e6))
        idx = pf.astype(np.int64)
        f = idx - np.arange(WIN).reshape(d.shape)
        lo = f.min(0, keepdims=True)
        bad = (f - lo > 1) | (lo < -500000)
        w1, w0 = pos - pf, (pf + one) - pos
    zero = dt(0)
    return np.where(bad, FAR, idx).astype(np.int32), np.where(bad, zero, w0).astype(dtype), np.where(bad, zero, w1).astype(dtype)


def tap_floor_f32(c, size, level):
    return tap_floor(c, size, level, np.float32)


def taps(coords, levels=4, dtype=np.float32):
    """[(X, Y)] per level for coords (b, 2, h8, w8): X = tap_floor of the b h8 w8 x coordinates on the level's width, Y likewise."""
    b, _, h8, w8 = coords.shape
    co = coords.detach().cpu().numpy().astype(dtype).reshape(b, 2, -1)
    x, y = co[:, 0].reshape(-1), co[:, 1].reshape(-1)
    return [(tap_floor(x, wl, l, dtype), tap_floor(y, hl, l, dtype)) for l, (hl, wl) in enumerate(level_sizes(h8, w8, levels))]


# ------------------------------------------------------------------------------------------------------------------------------- lookup
def lookup(levels_dense, coords, tap_list=None, dtype=torch.float64, absolute=False, pad_hook=None):
    """(b, levels 81, h8, w8) in ``dtype``: window channel l 81 + i 9 + j = level l at tap i along x and tap j along y (upstream's order),
    wy0 (wx0 v00 + wx1 v01) + wy1 (wx0 v10 + wx1 v11) with zeros outside the level.  ``tap_list``: taps() of the coordinates (default: the
    float32 restatement); ``absolute``: |w| |v| in place of w v; ``pad_hook(l, padded)`` may alter the zero-padded copy of level l
    (b nq, h_l + 2, w_l + 2; every pixel outside the level reads its one-cell ring) -- for mutants."""
    b, _, h8, w8 = coords.shape
    n = b * h8 * w8
    tap_list = taps(coords, len(levels_dense)) if tap_list is None else tap_list
    rows = torch.arange(n)[:, None, None]
    out = []
    for l, (lvl, (X, Y)) in enumerate(zip(levels_dense, tap_list)):
        hl, wl = lvl.shape[-2:]
        P = F.pad(lvl.reshape(n, hl, wl).to(dtype), (1, 1, 1, 1))
        if absolute:
            P = P.abs()
        if pad_hook is not None:
            pad_hook(l, P)
        def axis(T, size):
            idx, w0, w1 = (torch.from_numpy(np.ascontiguousarray(t)) for t in T)          # (9, n)
            i0, i1 = idx.long().clamp(-1, size) + 1, (idx.long() + 1).clamp(-1, size) + 1
            w0, w1 = w0.to(dtype), w1.to(dtype)
            return i0.t(), i1.t(), (w0.abs() if absolute else w0).t(), (w1.abs() if absolute else w1).t()
        x0, x1, wx0, wx1 = (t[:, :, None] for t in axis(X, wl))                            # (n, 9 i, 1)
        y0, y1, wy0, wy1 = (t[:, None, :] for t in axis(Y, hl))                            # (n, 1, 9 j)
        top = wx0 * P[rows, y0, x0] + wx1 * P[rows, y0, x1]
        bot = wx0 * P[rows, y1, x0] + wx1 * P[rows, y1, x1]
        out.append((wy0 * top + wy1 * bot).reshape(b, h8 * w8, WIN * WIN))
    return torch.cat(out, 2).permute(0, 2, 1).reshape(b, len(levels_dense) * WIN * WIN, h8, w8).contiguous()


def lookup_abs(levels_dense, coords, tap_list=None):
    return lookup(levels_dense, coords, tap_list, torch.float64, absolute=True)


def check_lookup(got, levels_dense, coords, tag=''):
    """``got`` (b, 324, h8, w8) within ((1 + u)^4 - 1) sum |w| |v| of the float64 window of ``levels_dense`` at the float32-restated taps,
    element by element and with nothing left out; a zero bound demands an exact zero.  Prints and returns max err / bound."""
    tl = taps(coords, len(levels_dense))
    truth, ab = lookup(levels_dense, coords, tl), lookup_abs(levels_dense, coords, tl)
    assert tuple(got.shape) == tuple(truth.shape), (tag, tuple(got.shape))
    err, bound = (got.cpu().double() - truth).abs(), LOOKUP_K * ab
    inside = bound > 0
    r = float((err[inside] / bound[inside]).max()) if bool(inside.any()) else 0.0
    print(f'{tag} lookup: max err / bound {r:.3f}; {int((~inside).sum())} of {inside.numel()} outputs read nothing inside their level')
    assert bool((err <= bound).all()), (tag, 'lookup', r, int((~(err <= bound)).sum()))
    return r


# -------------------------------------------------------------------------------------------------------------------------- coordinates
def pin_coords(b, h8, w8, seed):
    """float32 (b, 2, h8, w8): targets uniform over the map plus a margin of 6 (windows partly outside) with every fraction in [0.02, 0.98],
    and in row 0 the planted queries of tests/test_gpu_corr_backward.py's _coords: half positions, windows wholly outside every level, a
    window of which only a corner is inside.  Away from the plants c / 2^l is at least 1e-3 from an integer at every level: asserted."""
    g = torch.Generator().manual_seed(seed)
    def axis(size):
        whole = torch.floor(torch.rand(b, h8 * w8, generator=g) * (size + 11) - 6)
        return whole + 0.02 + 0.96 * torch.rand(b, h8 * w8, generator=g)
    x, y = axis(w8), axis(h8)
    plants = [(3.5, 5.5), (w8 - 1.5, h8 - 1.5), (-0.5, 2.5), (-50.5, -50.5), (w8 + 60.5, h8 + 60.5), (w8 - 1 + 4.5, h8 - 1 + 4.5), (-3.5, -3.5)]
    for q, (px, py) in enumerate(plants):
        x[0, 7 * q + 1], y[0, 7 * q + 1] = px, py
    co = torch.stack((x, y), 1).reshape(b, 2, h8, w8).float()
    for l in range(4):
        v = co.double().reshape(b, 2, -1) / 2 ** l
        frac = v - torch.floor(v)
        assert bool(((frac >= 1e-3) & (frac <= 1 - 1e-3)).all()), l
    f0 = co.double() - torch.floor(co.double())
    assert bool(((f0 >= 0.02 - 1e-6) & (f0 <= 0.98 + 1e-6)).all())
    return co


NONFINITE = [(float('nan'), 3.0), (3.0, float('inf')), (float('-inf'), 3.0), (1.0e12, 2.0), (2.0, -3000.0), (float('nan'), float('nan'))]


def edge_plants(h8, w8):
    """The planted (x, y) of edge_coords, NONFINITE last."""
    W, H, e = w8 - 1.0, h8 - 1.0, np.float32(-1e-7).item()
    p = [(8.0, 8.0), (0.0, 0.0), (8.0 * ((w8 - 1) // 8), 8.0 * ((h8 - 1) // 8)),            # integers at every level
         (2.5, 8.5), (8.5, 3.5),                                                            # half-integers
         (-0.0, 3.0), (3.0, -0.0), (-0.0, -0.0), (e, 5.0), (5.0, e), (e, e),
         (W, H), (W, 2.25), (3.25, H)]
    for d in (4.0, 4.5, 5.0):                                                               # last tap column inside ... nothing inside
        p += [(-d, 6.25), (6.25, -d), (-d, -d), (W + d, 6.25), (6.25, H + d), (W + d, H + d), (-d, H + d), (W + d, -d)]
    return p + NONFINITE


def edge_coords(b, h8, w8, seed):
    """(coords float32 (b, 2, h8, w8), flat query indices of the plants in batch row 0, number of NONFINITE plants at their end): random over
    the map plus a margin of 6 at arbitrary fractions, a quarter of them rounded to quarter positions, and edge_plants at queries 5 p + 2 of
    row 0 -- asserted on the generated tensor bit for bit."""
    g = torch.Generator().manual_seed(seed)
    nq = h8 * w8
    x = torch.rand(b, nq, generator=g) * (w8 + 11) - 6
    y = torch.rand(b, nq, generator=g) * (h8 + 11) - 6
    quarter = torch.rand(b, nq, generator=g) < 0.25
    x, y = torch.where(quarter, torch.round(x * 4) / 4, x), torch.where(quarter, torch.round(y * 4) / 4, y)
    plants = edge_plants(h8, w8)
    at = [5 * p + 2 for p in range(len(plants))]
    assert at[-1] < nq
    co = torch.stack((x, y), 1).float()
    co[0, :, at] = torch.tensor(plants, dtype=torch.float64).t().float()
    co = co.reshape(b, 2, h8, w8).contiguous()
    back = co[0].reshape(2, nq)[:, at].t().numpy()
    assert np.array_equal(back.view(np.int32), np.array(plants, dtype=np.float32).view(np.int32))             # -0.0 and NaN included
    assert bool(np.signbit(back[5, 0])) and back[5, 0] == 0.0 and back[8, 0] < 0.0 and float(np.floor(back[8, 0])) == -1.0
    return co, at, len(NONFINITE)
