"""Float64 restatement (numpy / torch on the CPU, no kernels) of csrc/geometry.hip: disparity -> depth and validity, back-projection of both
frames, the bilinear warp of the second cloud, image and stereo flow by the time flow, the nearest warp of the mask, and the two 8-channel
1/8 stacks.  tests/test_geometry_ref_cpu.py pins it against oracle.warp (torch's own grid_sample / interpolate / linalg.inv);
tests/test_gpu_geometry_edges.py holds the kernels to it.

What is decided in float32, because the float32 arithmetic IS the definition:
  * the sampling positions: oracle.warp.source_coords, the round trip 2 * (flow + index) / (size - 1) - 1 -> ((g + 1) / 2) * (size - 1) one
    rounded operation at a time.  floor() and rint() of them choose the pixels that are read;
  * depth2 and its validity: oracle.warp.flow2depth (one IEEE division, 0 < d <= 1, invalid depths become 1).

THE RULE for positions that cannot be read: a position p "reads" iff  -1e6 < p < 1e6  (so NaN, +-Inf and anything at or beyond +-1e6 do
not).  If either coordinate of a pixel's position does not read, the bilinear warp of that pixel is 0 in every plane and the nearest warp
gives mask False.  floor_tap / nearest_tap report FAR_TAP (-1000000) for such a coordinate; for the nearest tap the rule is applied to
rint(p), the value that is converted.  No NaN or Inf is ever cast to an integer: the cast is taken of a copy in which they are 0.

Everything after those decisions is float64: K^-1 by numpy.linalg.inv per row, rays through (x + .5, y + .5), clouds, bilinear weights from
the float32 positions widened to float64 ((x0 + 1 - p) and (p - x0) are exact), a tap outside the image ABSENT from the sum (never a
product with a clamped value; an in-image tap with weight 0 is a product, so 0 * Inf is NaN as in torch), the x0.125 stacks as the mean of
the 2x2 centre pixels (8i + 3..4, 8j + 3..4) of each 8x8 cell.

Also here: the edge scenes of the GPU tests (edge_scene), coverage(scene) -- how many pixels fall in each edge class, counted from this
module's own positions -- the channel groups each output is judged in (groups) and the comparison (compare)."""
import numpy as np
import torch

from oracle import warp

FAR = np.float32(1.0e6)
FAR_TAP = -1000000
SENTINEL = 1e30
NAN, INF = float('nan'), float('inf')
F32 = np.float32


# ----------------------------------------------------------------------------------------------------- positions and taps (float32)
def positions(flow):
    """(ix, iy) float32 (n,h,w): oracle.warp.source_coords.  A 1-pixel axis divides by size - 1 = 0: NaN or Inf, which do not read."""
    with np.errstate(all='ignore'):
        return warp.source_coords(torch.as_tensor(flow).float())


def reads(p):
    """THE RULE: -1e6 < p < 1e6 (False for NaN)."""
    with np.errstate(invalid='ignore'):
        return (p > -FAR) & (p < FAR)


def _to_int(p, ok):
    return np.where(ok, np.where(ok, p, F32(0)).astype(np.int64), FAR_TAP)


def floor_tap(p):
    """floor(p) as an integer, FAR_TAP where p does not read."""
    return _to_int(np.floor(p), reads(p))


def nearest_tap(p):
    """rint(p) (ties to even) as an integer, FAR_TAP where rint(p) does not read."""
    r = np.rint(p)
    return _to_int(r, reads(r))


def taps(flow):
    ix, iy = positions(flow)
    return dict(ix=ix, iy=iy, x0=floor_tap(ix), y0=floor_tap(iy), xn=nearest_tap(ix), yn=nearest_tap(iy))


# --------------------------------------------------------------------------------------------------------------- warps (float64)
def _gather(planes, yy, xx, inb):
    """planes (n,c,h,w) at integer (yy, xx) (n,h,w) where inb, else an exact 0 that takes no part in any product."""
    n, c, h, w = planes.shape
    bi = np.arange(n)[:, None, None]
    v = planes[bi, :, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]           # (n,h,w,c)
    return np.moveaxis(v, -1, 1), inb[:, None]


def bilinear(planes, ix, iy):
    """Zero-padded bilinear sample of float64 planes (n,c,h,w) at float32 positions (n,h,w)."""
    planes = np.asarray(planes, np.float64)
    n, c, h, w = planes.shape
    ok = reads(ix) & reads(iy)
    x0, y0 = floor_tap(ix), floor_tap(iy)
    px, py = np.where(ok, ix, F32(0)).astype(np.float64), np.where(ok, iy, F32(0)).astype(np.float64)
    fx, fy = np.where(ok, x0, 0).astype(np.float64), np.where(ok, y0, 0).astype(np.float64)
    wx = (fx + 1.0 - px, px - fx)
    wy = (fy + 1.0 - py, py - fy)
    out = np.zeros_like(planes)
    with np.errstate(invalid='ignore'):
        for dy in (0, 1):
            for dx in (0, 1):
                xx, yy = x0 + dx, y0 + dy
                inb = ok & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                v, m = _gather(planes, yy, xx, inb)
                out = out + np.where(m, v * (wx[dx] * wy[dy])[:, None], 0.0)
    return out


def touched(flow, h, w, only=None):
    """Boolean (n,h,w): source pixels that are an in-image tap (weight 0 included) of the bilinear warp of some output pixel; ``only``
    (h,w) bool restricts the output pixels."""
    t = taps(flow)
    n = t['x0'].shape[0]
    hit = np.zeros((n, h, w), dtype=bool)
    sel = np.ones((h, w), dtype=bool) if only is None else only
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = t['x0'] + dx, t['y0'] + dy
            inb = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h) & sel[None]
            for r in range(n):
                hit[r, yy[r][inb[r]], xx[r][inb[r]]] = True
    return hit


def nearest_mask(mask, ix, iy):
    """mask (n,h,w) bool at the nearest pixel of each position; False where nothing is read."""
    n, h, w = mask.shape
    xn, yn = nearest_tap(ix), nearest_tap(iy)
    inb = (xn >= 0) & (xn < w) & (yn >= 0) & (yn < h)
    bi = np.arange(n)[:, None, None]
    return inb & mask[bi, np.clip(yn, 0, h - 1), np.clip(xn, 0, w - 1)]


def centre_pixels(h, w):
    """(h,w) bool: the 2x2 centre pixels of every 8x8 cell -- the only pixels the x0.125 stacks look at."""
    c = np.zeros((h, w), dtype=bool)
    for dy in (3, 4):
        for dx in (3, 4):
            c[dy::8, dx::8] = True
    return c


def down8(x):
    """Mean of the 2x2 centre pixels of each 8x8 cell (bilinear x0.125, align_corners=False, samples exactly 8i + 3.5)."""
    return 0.25 * (x[:, :, 3::8, 3::8] + x[:, :, 3::8, 4::8] + x[:, :, 4::8, 3::8] + x[:, :, 4::8, 4::8])


# ------------------------------------------------------------------------------------------------------------ the whole operation
ARGS = ('stereo_flow2', 'time_flow', 'baseline', 'K', 'depth1', 'image1l', 'image2l', 'stereo_flow1', 'mask2')


def rays(K, h, w):
    """(n,3,h,w) float64: K^-1 [x + .5, y + .5, 1], K^-1 by numpy.linalg.inv on float64, per row."""
    Ki = np.stack([np.linalg.inv(k) for k in np.asarray(K, np.float64)])
    px = (np.arange(w, dtype=np.float64) + 0.5)[None, None, None, :]
    py = (np.arange(h, dtype=np.float64) + 0.5)[None, None, :, None]
    return Ki[:, :, 0, None, None] * px + Ki[:, :, 1, None, None] * py + Ki[:, :, 2, None, None]


def forward(scene):
    """The outputs of rpe_depth_backproject_warp for scene (dict of torch tensors named as ARGS).  depth2 float32 and the masks / taps are
    exact by contract; pcl1, pcl2, pcl2w, inp1, inp2 are float64.  inp1 / inp2 are None unless h and w are multiples of 8."""
    sf2, tf, b, K, d1, i1, i2, sf1, m2 = (scene[k] for k in ARGS)
    n, _, h, w = sf2.shape
    depth2, valid = warp.flow2depth(sf2.float(), b.float())
    mask2 = (m2.bool() & valid).numpy()[:, 0]
    t = taps(tf)
    ix, iy = t['ix'], t['iy']
    ray = rays(K, h, w)
    pcl1 = d1.double().numpy() * ray
    pcl2 = depth2.double().numpy() * ray
    pcl2w = bilinear(pcl2, ix, iy)
    out = dict(depth2=depth2.numpy(), mask2=mask2[:, None], mask2w=nearest_mask(mask2, ix, iy)[:, None], pcl1=pcl1, pcl2=pcl2, pcl2w=pcl2w,
               inp1=None, inp2=None, **{k: t[k] for k in ('x0', 'y0', 'xn', 'yn', 'ix', 'iy')})
    if h % 8 == 0 and w % 8 == 0:
        f64 = lambda a: a.double().numpy()                                    # noqa: E731
        out['inp1'] = down8(np.concatenate((f64(sf1), f64(i1), pcl1), axis=1))
        out['inp2'] = down8(np.concatenate((bilinear(f64(sf2), ix, iy), bilinear(f64(i2), ix, iy), pcl2w), axis=1))
    return out


def oracle_f32(scene):
    """The same outputs from oracle.warp: the torch float32 calls the reference project makes.  The flow of a pixel whose position does not
    read is handed to torch as 1e9: at a NaN or +-Inf position torch's CPU bilinear grid_sample multiplies its masked-out taps by NaN weights
    and returns NaN, where the rule (and the kernels) read nothing and give 0; at a finite position beyond +-1e6 torch gives 0 too, and its
    nearest mode gives False for all of them (tests/test_geometry_ref_cpu.py)."""
    sf2, tf, b, K, d1, i1, i2, sf1, m2 = (scene[k] for k in ARGS)
    dead = torch.from_numpy(no_read(scene))[:, None].expand_as(tf)
    tf = torch.where(dead, torch.full_like(tf, 1e9), tf)
    depth2, valid = warp.flow2depth(sf2, b)
    m2v = m2.bool() & valid
    pcl1, pcl2 = warp.backproject(d1, K), warp.backproject(depth2, K)
    pcl2w, mask2w, inp1, inp2 = warp.weight_inputs(pcl1, pcl2, i1, i2, m2v, tf, sf1, sf2)
    return dict(depth2=depth2, mask2=m2v, mask2w=mask2w, pcl1=pcl1, pcl2=pcl2, pcl2w=pcl2w, inp1=inp1, inp2=inp2)


GROUPS = ('inp1.sflow', 'inp1.image', 'inp1.cloud', 'inp2.sflow', 'inp2.image', 'inp2.cloud', 'pcl1', 'pcl2', 'pcl2w')


def groups(out):
    """The float outputs split into the channel groups that are each judged at their own scale (numpy float64)."""
    a = lambda v: None if v is None else (v.detach().cpu().double().numpy() if torch.is_tensor(v) else np.asarray(v, np.float64))   # noqa: E731
    g = {}
    for k in ('inp1', 'inp2'):
        v = a(out[k])
        if v is not None:
            g[k + '.sflow'], g[k + '.image'], g[k + '.cloud'] = v[:, 0:2], v[:, 2:5], v[:, 5:8]
    for k in ('pcl1', 'pcl2', 'pcl2w'):
        if out.get(k) is not None:
            g[k] = a(out[k])
    return g


def max_err(got, want):
    """Max abs error over the elements ``want`` has finite, after asserting that NaN sits exactly where ``want`` has it and +-Inf likewise
    with the same sign."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN positions differ'
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(np.sign(got[inf]), np.sign(want[inf])), 'Inf positions differ'
    fin = np.isfinite(want)
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


# ------------------------------------------------------------------------------------------------------------------- edge scenes
def _pos1(v, size):
    """The float32 round trip for one axis (v = flow + index, already rounded)."""
    with np.errstate(all='ignore'):
        sm1, one, two = F32(size - 1), F32(1), F32(2)
        g = two * F32(v) / sm1 - one
        return ((g + one) / two) * sm1


def _flow_for(target, idx, size):
    """A float32 flow for pixel index idx whose position is exactly ``target`` if some flow within 8 ulps of target - idx gives that, else
    target - idx itself (the round trip is not the identity: on most sizes positions k + .5 near 0 and -1 are not in its range)."""
    cands = [F32(target)]
    lo = hi = F32(target)
    for _ in range(8):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        cands += [lo, hi]
    for c in cands:
        f = F32(c - F32(idx))
        if _pos1(F32(f + F32(idx)), size) == F32(target):
            return f
    return F32(F32(target) - F32(idx))


def _flow_beside(edge, idx, size, below):
    """A flow whose position is as close as found to ``edge`` on the stated side (strictly)."""
    for e in range(24, 3, -1):
        d = F32(2.0 ** -e)
        f = F32(F32(edge - d if below else edge + d) - F32(idx))
        p = _pos1(F32(f + F32(idx)), size)
        if (p < edge) if below else (p > edge):
            return f
    raise AssertionError('no position beside the edge')


def axis_targets(size):
    """The listed targets of one axis: (name, value or ('below' | 'above', edge))."""
    s = float(size)
    return [('-1.5', -1.5), ('-1', -1.0), ('-0.5', -0.5), ('<0', ('below', 0.0)), ('0', 0.0), ('0.5', 0.5), ('1.5', 1.5), ('2.5', 2.5),
            ('s-2', s - 2), ('s-1.5', s - 1.5), ('s-1', s - 1), ('>s-1', ('above', s - 1)), ('s-0.5', s - 0.5), ('s', s), ('s+0.5', s + 0.5)]


def target_flow(t, idx, size):
    if isinstance(t, tuple):
        return _flow_beside(F32(t[1]), idx, size, t[0] == 'below')
    return _flow_for(t, idx, size)


NONFINITE = [NAN, INF, -INF, 1e9, -1e9, 3e38, -3e38]
ROW_K = [(1.1, 1.3, 0.5, 0.5, 0.02, 0.37, -1.21),           # fx/w, fy/w, cx/w, cy/h, skew/w, and offsets of cx, cy in pixels
         (0.9, 0.8, -0.4, 1.3, -0.05, 0.0, 0.0),            # the principal point outside the image
         (2.1, 1.7, 0.31, 0.77, 0.11, -0.13, 0.29)]
ROW_BASELINE = [5.25, 0.8125, 0.0]


def _rows(n):
    return [1] if n == 1 else list(range(n))


def intrinsics(n, h, w):
    K = np.zeros((n, 3, 3), dtype=np.float32)
    for r, k in enumerate(_rows(n)):
        fx, fy, cx, cy, sk, ox, oy = ROW_K[k % 3]
        K[r] = [[fx * w, sk * w, cx * w + ox], [0.0, fy * w, cy * h + oy], [0.0, 0.0, 1.0]]
    return torch.from_numpy(K)


def disparity_edges(b):
    """(name, disparity) for a row of baseline b.  '-huge' is the one value that must not be a tap of any 1/8 stack (its float32 error would
    drown the group it falls in)."""
    b = F32(b)
    return [('+0', F32(0.0)), ('-0', F32(-0.0)), ('nan', F32(NAN)), ('+inf', F32(INF)), ('-inf', F32(-INF)), ('+denormal', F32(1e-40)),
            ('-denormal', F32(-1e-40)), ('-huge', F32(-3e38)), ('depth==1', -b), ('depth>1', np.nextafter(-b, F32(0))),
            ('depth<1', np.nextafter(-b, F32(-INF)))]


def edge_scene(n, h, w, fused=True):
    """The scene of the edge tests for an (n, h, w) call (deterministic).  Returns the dict of input tensors (ARGS) plus 'meta': the pixels
    every deliberate value was put at.  With fused=False only time_flow, stereo_flow2 and baseline are meaningful (any h, w)."""
    rng = np.random.default_rng(100000 * n + 1000 * h + w)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
    hw = h * w
    base = np.array([ROW_BASELINE[k % 3] for k in _rows(n)], dtype=np.float32)
    tf = rng.normal(0, 2.5, size=(n, 2, h, w)).astype(np.float32)
    sf2 = rng.normal(0, 1.0, size=(n, 2, h, w)).astype(np.float32)
    sf2[:, 0] = -rng.uniform(2.0, 40.0, size=(n, h, w))                       # depth b / 40 ... b / 2: rows 0 part invalid (> 1), row 1 all valid
    sf2[:, 0][rng.uniform(size=(n, h, w)) < 0.1] *= -1                        # positive disparities: negative depth, invalid
    m2 = rng.uniform(size=(n, 1, h, w)) > 0.2
    centre = centre_pixels(h, w) if fused else np.zeros((h, w), dtype=bool)
    meta = dict(nonfinite=[], targets=[], disparity=[], pointers=[], sentinels=[])

    for r in range(n):
        free = np.ones(hw, dtype=bool)

        def take(p):
            assert free[p], p
            free[p] = False
            return divmod(p, w)

        def take_any(prefer_centre):
            cand = np.flatnonzero(free & (centre.reshape(-1) == prefer_centre))
            if cand.size == 0:
                cand = np.flatnonzero(free)
            return take(int(cand[(7 * len(meta['targets']) + 3 * r) % cand.size]))

        # non-finite and far flow: corners, row ends, the last lane of block 0 and the first of block 1, a centre pixel, then anywhere
        spots = [0, w - 1, hw - 1, hw - w, 2 * w - 1 if h > 1 else None, 255 if hw > 256 else None, 256 if hw > 256 else None]
        if fused:
            spots.insert(3, (8 * (h // 8 - 1) + 4) * w + 8 * (w // 8 - 1) + 4)
        spots = [p for i, p in enumerate(spots) if p is not None and p < hw and p not in spots[:i]]
        combos = [(v, c) for v in NONFINITE for c in (0, 1)]
        combos = combos[(5 * r) % 14:] + combos[:(5 * r) % 14]
        if hw < 40:
            combos = combos[:max(1, hw // 3)]
        for i, (v, c) in enumerate(combos):
            if i < len(spots) and free[spots[i]]:
                y, x = take(spots[i])
            else:
                y, x = take_any(False)
            tf[r, c, y, x] = v
            meta['nonfinite'].append((r, y, x, c, v))

        # targeted positions: every target of each axis with a plain partner on the other axis, then corners where both axes are at a border
        def plain(idx, size):
            return F32(min(max(idx + 0.25, 0.25), max(size - 1.25, 0.25)) - idx)

        tx, ty = axis_targets(w), axis_targets(h)
        name = dict(tx)
        namey = dict(ty)
        pairs = [(('<0', '<0')), ('s-0.5', 's-0.5'), ('-1', 's-1'), ('>s-1', '<0'), ('s-1', 's-1'), ('0', '0'), ('s-1.5', 's-0.5'), ('-0.5', '>s-1'),
                 ('s', '0.5')]
        todo = [('x', k, None) for k, _ in tx] + [('y', None, k) for k, _ in ty]
        todo = [('xy', a, b_) for a, b_ in pairs] + todo[(4 * r) % 30:] + todo[:(4 * r) % 30]
        for kind, kx, ky in todo:
            if not free.any():
                break
            y, x = take_any(True)
            tf[r, 0, y, x] = target_flow(name[kx], x, w) if kx is not None else plain(x, w)
            tf[r, 1, y, x] = target_flow(namey[ky], y, h) if ky is not None else plain(y, h)
            meta['targets'].append((r, y, x, kx, ky))

        # disparity edges (their own tensor: they may share a pixel with a deliberate flow); '-huge' and the sentinels go where no centre
        # pixel's taps fall
        untouched = np.flatnonzero(~touched(tf[r:r + 1], h, w, only=centre if fused else None)[0].reshape(-1))
        if not fused:
            untouched = np.arange(hw)
        edges = disparity_edges(base[r])
        dsp = [0, w - 1, hw - 1, 255, 256, hw - w] + list(range(w + 1, hw, max(1, hw // 17)))
        dsp = [p for i, p in enumerate(dsp) if p < hw and p not in dsp[:i]]
        used = set()
        for i, (nm, v) in enumerate(edges):
            if nm == '-huge':
                cand = [int(p) for p in untouched if int(p) not in used and int(p) not in dsp[:len(edges)]]
            else:
                cand = [p for p in dsp if p not in used]
            if not cand:
                continue
            p = cand[0]
            used.add(p)
            y, x = divmod(p, w)
            sf2[r, 0, y, x] = v
            m2[r, 0, y, x] = True
            meta['disparity'].append((r, y, x, nm))
        # pixels whose nearest source is one of those (mask2 True there, so a False is the validity's doing)
        for (rr, y, x, nm) in [d for d in meta['disparity'] if d[0] == r and d[3] in ('nan', '+0', 'depth>1', 'depth==1')]:
            cand = np.flatnonzero(free & ~centre.reshape(-1))
            if cand.size == 0:
                break
            py, px = take(int(cand[cand.size // 2]))
            tf[r, 0, py, px] = F32(F32(x + 0.25 if x < w - 1 else x - 0.25) - px)
            tf[r, 1, py, px] = F32(F32(y - 0.25 if y > 0 else y + 0.25) - py)
            meta['pointers'].append((r, py, px, y, x, nm))

    scene = dict(stereo_flow2=t32(sf2), time_flow=t32(tf), baseline=t32(base), meta=meta)
    if not fused:
        return scene
    i2 = rng.uniform(0, 255, size=(n, 3, h, w)).astype(np.float32)
    # wrong-read sentinel: 1e30 where no tap of any centre pixel falls (the full-resolution warp reads only the disparity plane)
    hit = touched(tf, h, w, only=centre)
    for r in range(n):
        taken = {(y, x) for (rr, y, x, _) in meta['disparity'] if rr == r}
        cand = [divmod(int(p), w) for p in np.flatnonzero(~hit[r].reshape(-1))]
        cand = [c for c in cand if c not in taken]
        for (y, x) in cand[::max(1, len(cand) // 5)][:5]:
            i2[r, :, y, x] = SENTINEL
            sf2[r, 1, y, x] = SENTINEL
            meta['sentinels'].append((r, y, x))
    scene.update(stereo_flow2=t32(sf2), K=intrinsics(n, h, w), depth1=t32(rng.uniform(0.1, 1.0, size=(n, 1, h, w))),
                 image1l=t32(rng.uniform(0, 255, size=(n, 3, h, w))), image2l=t32(i2), stereo_flow1=t32(rng.normal(0, 5.0, size=(n, 2, h, w))),
                 mask2=torch.from_numpy(m2))
    return scene


def row_of(scene, r):
    """Row r of a scene as a scene of its own (contiguous copies)."""
    return {k: (v[r:r + 1].clone() if torch.is_tensor(v) else v) for k, v in scene.items()}


def permuted(scene, perm):
    idx = torch.as_tensor(perm)
    return {k: (v[idx].clone() if torch.is_tensor(v) else v) for k, v in scene.items()}


def no_read(scene):
    """(n,h,w) bool: pixels whose position does not read (the rule above)."""
    ix, iy = positions(scene['time_flow'])
    return ~(reads(ix) & reads(iy))


def coverage(scene):
    """How many pixels of the scene fall in each edge class, from this module's own positions (and oracle.warp.flow2depth)."""
    tf = scene['time_flow']
    n, _, h, w = tf.shape
    ix, iy = positions(tf)
    c = {}
    with np.errstate(invalid='ignore'):
        for ax, p, size in (('x', ix, w), ('y', iy, h)):
            ok = reads(p)
            frac = p - np.floor(p)
            tie = ok & (frac == F32(0.5)) & (p > -2) & (p < size + 1)
            low = np.where(tie, np.floor(np.where(tie, p, 0)), 0).astype(np.int64)
            c[ax + ':tie to even, down'] = int((tie & (low % 2 == 0)).sum())
            c[ax + ':tie to even, up'] = int((tie & (low % 2 != 0)).sum())
            c[ax + ':in (-1, 0)'] = int((ok & (p > -1) & (p < 0)).sum())
            c[ax + ':in (size-1, size)'] = int((ok & (p > size - 1) & (p < size)).sum())
            c[ax + ':exactly -1'] = int((p == -1).sum())
            c[ax + ':exactly size-1'] = int((p == size - 1).sum())
            c[ax + ':exactly 0'] = int((p == 0).sum())
            c[ax + ':below -1'] = int((ok & (p < -1)).sum())
            c[ax + ':at or beyond size'] = int((ok & (p >= size)).sum())
            c[ax + ':does not read'] = int((~ok).sum())
        bx = reads(ix) & (((ix > -1) & (ix <= 0)) | ((ix >= w - 1) & (ix < w)))
        by = reads(iy) & (((iy > -1) & (iy <= 0)) | ((iy >= h - 1) & (iy < h)))
        c['corner: both axes at a border'] = int((bx & by).sum())
        c['nan position'] = int((np.isnan(ix) | np.isnan(iy)).sum())
        c['inf position'] = int((np.isinf(ix) | np.isinf(iy)).sum())
    sf2, b = scene['stereo_flow2'], scene['baseline']
    with np.errstate(all='ignore'):
        q = (b[:, None, None] / -sf2[:, 0]).numpy()
    depth2, valid = warp.flow2depth(sf2, b)
    valid = valid.numpy()[:, 0]
    c['depth exactly 1 (valid)'] = int(((q == 1) & valid).sum())
    c['depth one ulp above 1 (invalid)'] = int((q == np.nextafter(F32(1), F32(2))).sum())
    c['denormal depth (valid)'] = int(((q > 0) & (q < np.finfo(np.float32).tiny) & valid).sum())
    c['quotient nan'] = int(np.isnan(q).sum())
    c['quotient +-inf'] = int(np.isinf(q).sum())
    c['quotient +-0'] = int((q == 0).sum())
    c['rows with baseline 0'] = int((b == 0).sum())
    if 'mask2' in scene:
        m2 = scene['mask2'].numpy()[:, 0]
        xn, yn = nearest_tap(ix), nearest_tap(iy)
        inb = (xn >= 0) & (xn < w) & (yn >= 0) & (yn < h)
        bi = np.arange(n)[:, None, None]
        src = lambda a: a[bi, np.clip(yn, 0, h - 1), np.clip(xn, 0, w - 1)]     # noqa: E731
        c['nearest source: mask2 True, disparity invalid'] = int((inb & src(m2) & ~src(valid)).sum())
        c['sentinels'] = len(scene['meta']['sentinels'])
    return c
