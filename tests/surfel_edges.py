"""Exact scenes for the surfel-map edge tests (tests/test_gpu_surfel_edges.py, and their CPU preconditions in
tests/test_surfel_map_cpu.py): inputs on which every DECISION of fuse / render -- in or out of the image, the rounded pixel, the depth
test, the prune, the render winner -- is the same in float32 and float64 by construction, so a kernel can be held to the float64
decisions exactly, with no surfel set aside.

  K      power-of-two focal lengths, dyadic principal point (fx = fy = 16, cx = w / 2, cy = h / 2); Kinv is the exact dyadic inverse
  poses  identity, a dyadic translation, a half turn about z (q = (0, 0, 1, 0)): lietorch's p + w uv + v x uv is exact for all three
  points depths and camera-space z are powers of two, x and y dyadic: u and v land on the listed values without a rounding

``check_exact`` asserts that the float32 and float64 restatements (tests/surfel_ref.py) decide alike: a precondition on the inputs."""
import math

import numpy as np
import torch

import surfel_ref as sr

F32, F64 = torch.float32, torch.float64
EPS = 2.0 ** -10                       # the "just outside / just inside" offset of a coordinate
POSES = {'identity': (0., 0., 0., 0., 0., 0., 1.), 'shift': (.5, -.25, 0., 0., 0., 0., 1.), 'turn': (0., 0., 0., 0., 0., 1., 0.)}
RENDER_POSES = dict(POSES, shift=(.5, -.25, 2., 0., 0., 0., 1.))        # the render has no depth test: its shift also moves z


def kmat(h, w, mirror=False):
    """mirror (True or 'u'): fx = -16 and cx = -0.0, the one K under which u can be -0.0 (every term of the row is a negative zero);
    mirror 'v': the same for v (fy = -16, cy = -0.0)."""
    if mirror == 'v':
        return torch.tensor([[16., 0., w / 2], [0., -16., -0.], [0., 0., 1.]])
    if mirror:
        return torch.tensor([[-16., 0., -0.], [0., 16., h / 2], [0., 0., 1.]])
    return torch.tensor([[16., 0., w / 2], [0., 16., h / 2], [0., 0., 1.]])


def kinv(K):
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    return torch.tensor([[1 / fx, 0., -cx / fx + 0.], [0., 1 / fy, -cy / fy + 0.], [0., 0., 1.]])


def pose(name, table=POSES):
    return torch.tensor(table[name])


def cam_points(K, uvz):
    """Camera-space points that project to the given (u, v) at depth z: ((u - cx) z / fx, (v - cy) z / fy, z), in float64."""
    K = K.double()
    uvz = torch.tensor(uvz, dtype=F64).reshape(-1, 3)
    z = uvz[:, 2]
    return torch.stack(((uvz[:, 0] - K[0, 2]) * z / K[0, 0], (uvz[:, 1] - K[1, 2]) * z / K[1, 1], z))


def to_f32_exact(x):
    """float64 -> float32, asserting that nothing is rounded (the scenes are dyadic by construction)."""
    y = x.to(F32)
    assert torch.equal(torch.nan_to_num(y.double(), nan=7.), torch.nan_to_num(x, nan=7.)), 'a scene value is not a float32'
    return y


def world(T, cam):
    """Points (3,N) float64 that T^-1 takes to cam (fuse: opts = pose . cam; render under T: opts = T^-1 . cam -- pass the inverse)."""
    return to_f32_exact(sr.act(T.double(), cam, F64))


def same(a, b):
    """Equal values, NaN where NaN (the sign of a zero and a NaN's payload are not decisions)."""
    a, b = a.double(), b.double()
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ---------------------------------------------------------------------------------------------------------------- value yardstick
RATIOS = {}                            # section -> the worst kernel error / float32-restatement error seen (for the printed summary)


def rel_err(x, truth):
    """max |x - truth| / max |truth| over the entries where truth is finite; the others must agree as values (inf, NaN)."""
    x, truth = x.double().reshape(-1), truth.double().reshape(-1)
    assert x.shape == truth.shape, (x.shape, truth.shape)
    fin = torch.isfinite(truth)
    assert same(x[~fin], truth[~fin]), 'non-finite entries differ'
    if not bool(fin.any()):
        return 0.0
    scale = float(truth[fin].abs().max()) or 1.0
    return float((x[fin] - truth[fin]).abs().max()) / scale


def check_values(what, kernel, ref32, ref64, section='values'):
    """The value bound of the edge suite: the kernel's error against the float64 truth is at most twice the float32 restatement's
    (same formula in float32, another contraction); where the restatement is exact the kernel must be too."""
    ek, ey = rel_err(kernel, ref64), rel_err(ref32, ref64)
    print(f'{what}: kernel {ek:.3e}  float32 restatement {ey:.3e}  (max |x - f64| / max |f64|)')
    if ey > 0:
        RATIOS[section] = max(RATIOS.get(section, 0.0), ek / ey)
    assert ek <= 2 * ey, f'{what}: kernel error {ek:.3e} > 2 x {ey:.3e}'


# ---------------------------------------------------------------------------------------------------------------- fuse
TICK = 5


def fuse_scene(pose_name='identity', h=8, w=12):
    """One surfel per edge case of fuse's association (name -> expected association), d_thresh 8, tick 5; the frame is depth 4
    everywhere except the pixels of the depth cases.  Returns a dict of float32 tensors and the expectations."""
    assert (h, w) == (8, 12)
    K = kmat(h, w)
    P = pose(pose_name)
    one_below = float(np.nextafter(np.float32(1), np.float32(0)))
    #       name          u            v            z   conf       t_created  associated
    rows = [('u0',        0.,          .5,          4., .25,       TICK,      True),      # u == 0: in, column rint(-.5) = 0
            ('v0',        6.5,         0.,          4., .25,       TICK,      True),
            ('vtie1',     7.5,         1.,          4., .25,       TICK,      True),      # rint(.5) = 0: row 0
            ('u_neg',     -EPS,        1.5,         4., .25,       TICK,      False),
            ('u_hi_in',   w - 1 - EPS, 1.5,         4., .25,       TICK,      True),      # column 10
            ('u_w1',      w - 1.,      2.5,         4., .25,       TICK,      False),     # the test is u < w - 1
            ('utie1',     1.,          2.5,         4., .25,       TICK,      True),      # rint(.5) = 0
            ('utie3',     3.,          2.5,         4., .25,       TICK,      True),      # rint(2.5) = 2
            ('vtie2',     8.5,         2.,          4., .25,       TICK,      True),      # rint(1.5) = 2
            ('vtie3',     9.5,         3.,          4., .25,       TICK,      True),      # rint(2.5) = 2
            ('utie2',     2.,          3.5,         4., .25,       TICK,      True),      # rint(1.5) = 2
            ('utie5',     5.,          3.5,         4., .25,       TICK,      True),      # rint(4.5) = 4
            ('v_neg',     3.5,         -EPS,        4., .25,       TICK,      False),
            ('v_h1',      5.5,         h - 1.,      4., .25,       TICK,      False),
            ('v_hi_in',   4.5,         h - 1 - EPS, 4., .25,       TICK,      True),      # row 6
            ('d_eq',      .5,          4.5,         8., .25,       TICK,      False),     # |16 - 8| == d_thresh
            ('d_ulp',     1.5,         4.5,         8., .25,       TICK,      True),      # |2^-21 - 8| = nextafter(8, 0)
            ('d_nan',     2.5,         4.5,         4., .25,       TICK,      False),
            ('d_inf',     3.5,         4.5,         4., .25,       TICK,      False),
            ('masked',    .5,          5.5,         4., .25,       TICK,      False),
            ('m1',        2.5,         5.5,         4., .25,       TICK,      True),      # three surfels on pixel (5, 2)
            ('m2',        2.25,        5.5,         4., .375,      TICK,      True),
            ('m3',        2.75,        5.75,        4., .5,        TICK,      True),
            ('clamp',     4.5,         5.5,         4., .9,        TICK,      True),      # .9 + 1/7 > 1 -> exactly 1
            ('nanconf',   5.5,         5.5,         4., math.nan,  TICK,      True),
            ('stable',    -5.,         1.5,         4., 1.,        0,         False),     # old, conf 1: kept
            ('almost',    -5.,         1.5,         4., one_below, 0,         False),     # old, one ulp below 1: dropped
            ('old_assoc', 6.5,         6.5,         4., .25,       0,         True),      # updated, then pruned all the same
            ('by1',       8.5,         5.5,         4., .25,       TICK - 1,  True),
            ('by2',       9.5,         6.5,         4., .625,      TICK,      True)]
    names = [r[0] for r in rows]
    cam = cam_points(K, [r[1:4] for r in rows])
    # behind / at the camera centre and a NaN point: given in camera space
    extra = [('behind_neg', (.25, .25, -4.), False), ('behind_pos', (4., 4., -4.), False), ('centre', (0., 0., 0.), True),
             ('nanpt', (math.nan, 0., 4.), False)]
    cam = torch.cat((cam, torch.tensor([e[1] for e in extra], dtype=F64).T), dim=1)
    names += [e[0] for e in extra]
    expect = torch.tensor([r[6] for r in rows] + [e[2] for e in extra])
    n = cam.shape[1]
    depth = torch.full((h, w), 4.)
    depth[4, 0], depth[4, 1], depth[4, 2], depth[4, 3] = 16., 2.0 ** -21, math.nan, math.inf
    mask = torch.ones(h, w, dtype=torch.bool)
    mask[5, 0] = False
    img = (1 + torch.arange(h * w)[None] + h * w * torch.arange(3)[:, None]).float().reshape(3, h, w)      # a pixel's colour names it
    conf = torch.tensor([r[4] for r in rows] + [.25] * len(extra), dtype=F32)[None]
    t_created = torch.tensor([r[5] for r in rows] + [TICK] * len(extra), dtype=F32)[None]
    rgb = (1000 + 8 * torch.arange(n)[None] + torch.arange(3)[:, None]).float()                           # and a surfel's names it
    return dict(K=K, kinv=kinv(K), pose=P, opts=world(P, cam), rgb=rgb, conf=conf, t_created=t_created, depth=depth, img=img, mask=mask,
                tick=TICK, d_thresh=8.0, names=names, expect=expect, h=h, w=w)


def negzero_scene():
    """u == -0.0, which is in the image (-0 >= 0): reachable only under the mirrored K, where every term of K's first row is -0."""
    h, w = 8, 12
    K = kmat(h, w, mirror=True)
    cam = torch.tensor([[0., -.5, 4.], [0., .5, 4.]], dtype=F64).T              # 0 * y is -0 for the first, +0 for the second
    s = fuse_scene()
    s.update(K=K, kinv=kinv(K), opts=to_f32_exact(cam), rgb=s['rgb'][:, :2], conf=s['conf'][:, :2], t_created=s['t_created'][:, :2],
             depth=torch.full((h, w), 4.), mask=torch.ones(h, w, dtype=torch.bool), names=['negzero', 'poszero'], expect=torch.tensor([True, True]))
    return s


def small_scene(h, w, n=0, mask=True):
    """A frame of h x w at depth 4 with n bystander surfels at (0, 0, 4): the empty-input cases (n = 0, all-false mask, h = w = 1, w = 1)."""
    K = kmat(h, w)
    img = (1 + torch.arange(3 * h * w)).float().reshape(3, h, w)
    return dict(K=K, kinv=kinv(K), pose=pose('identity'), opts=torch.tensor([[0.], [0.], [4.]]).repeat(1, n), rgb=torch.full((3, n), 9.),
                conf=torch.full((1, n), .25), t_created=torch.full((1, n), float(TICK)), depth=torch.full((h, w), 4.), img=img,
                mask=torch.full((h, w), bool(mask)), tick=TICK, d_thresh=8.0, h=h, w=w)


def ref_map(s, average, t_max, conf_thr, dtype):
    m = sr.RefMap.__new__(sr.RefMap)
    m.K, m.kinv, m.dtype = s['K'].to(dtype), s['kinv'], dtype
    m.conf_thr, m.t_max, m.d_thresh, m.average = conf_thr, t_max, s['d_thresh'], average
    m.shape = (s['h'], s['w'])
    m.opts, m.rgb, m.conf, m.t_created = (s[k].to(dtype).clone() for k in ('opts', 'rgb', 'conf', 't_created'))
    m.tick = s['tick']
    return m


def fuse_truth(s, average, t_max, conf_thr, dtype):
    """One fuse of the restatement: the decisions (flags: associated surfels; new: appended pixels; keep: the prune over old + new)
    and the map afterwards."""
    m = ref_map(s, average, t_max, conf_thr, dtype)
    m.fuse(s['img'], s['depth'], s['mask'], s['pose'])
    return dict(flags=m.last_flags, new=m.last_new, keep=m.last_keep, opts=m.opts, rgb=m.rgb, conf=m.conf, t_created=m.t_created,
                n=m.opts.shape[1])


def check_exact_fuse(s, average, t_max, conf_thr):
    """Precondition: float32 and float64 take the same decisions on the scene.  Returns (float32, float64) results."""
    a, b = (fuse_truth(s, average, t_max, conf_thr, d) for d in (F32, F64))
    for k in ('flags', 'new', 'keep'):
        assert torch.equal(a[k], b[k]), f'{k}: the float32 and float64 restatements decide differently'
    assert a['n'] == b['n'] and torch.equal(a['t_created'].double(), b['t_created'])
    return a, b


FUSE_CASES = [(False, 2, 7), (True, 2, 7), (True, 0, 7), (False, 1, 7), (True, 1, 1), (False, 0, 1)]        # (average_pts, t_max, conf_thr)


# ---------------------------------------------------------------------------------------------------------------- render
def render_scene(h, w, pose_name='identity', nan_plane=False, seed=0):
    """Background: one low-conf surfel at every pixel centre with seeded generic colours (the neighbours a NaN fill reads); on top,
    the coordinate edges, the key-order groups and NaN colours.  Channel 1 is every surfel's index (finite, exact): it names the
    winner of a pixel.  nan_plane: channel 2 of every surfel is NaN (a plane that is all NaN)."""
    g = torch.Generator().manual_seed(seed + 31 * h + w)
    K = kmat(h, w)
    T = pose(pose_name, RENDER_POSES)
    uvz, conf, nanrgb = [], [], []

    def add(u, v, c, z=4., nan=False):
        uvz.append((u, v, z)); conf.append(c); nanrgb.append(nan)
        return len(conf) - 1

    for y in range(h):
        for x in range(w):
            add(x + .5, y + .5, .125, z=8.)
    near_one = 1 - 2.0 ** -20                                     # (1 - 2^-24 would not leave x = (u - cx) z / fx a float32)
    expect = {}                                                   # pixel -> index of the winner it must show (hand-derived)
    # coordinates: u == 0, just outside, u == w (out), just inside the last column, just below 1 (column 0 by truncation); same for v
    expect[1 * w + 0] = add(0., 1.5, .5)
    add(-EPS, 1.5, .75)
    add(float(w), 1.5, .75)
    expect[1 * w + w - 1] = add(w - EPS, 1.5, .5)
    expect[2 * w + 0] = add(near_one, 2.5, .5)
    expect[0 * w + 1] = add(1.5, 0., .5)
    add(1.5, -EPS, .75)
    add(1.5, float(h), .75)
    expect[(h - 1) * w + 1] = add(1.5, h - EPS, .5)
    expect[0 * w + 2] = add(2.5, near_one, .5)
    if h >= 8 and w >= 12:
        # key order, several surfels on one pixel (row 3 .. 5, columns 3 ..)
        add(3.5, 3.5, .5); expect[3 * w + 3] = add(3.25, 3.75, .5)                                   # equal conf: the largest index
        add(5.5, 3.5, math.inf); expect[3 * w + 5] = add(5.5, 3.5, math.nan); add(5.5, 3.5, math.inf)       # +inf < NaN
        add(6.5, 3.5, math.nan); expect[3 * w + 6] = add(6.5, 3.5, math.nan)                         # two NaNs: the index
        expect[3 * w + 7] = add(7.5, 3.5, 1., nan=True)                                              # NaN colours: interior, ...
        expect[3 * w + 8] = add(8.5, 3.5, 1., nan=True); expect[4 * w + 8] = add(8.5, 4.5, 1., nan=True)               # ... neighbours
        expect[4 * w + 7] = add(7.5, 4.5, 1., nan=True)
        expect[0] = add(.5, .5, 1., nan=True)                                                        # ... a corner
        expect[5 * w + w - 1] = add(w - .5, 5.5, 1., nan=True)                                       # ... an edge
    else:
        expect[(h // 2) * w + w // 2] = add(w // 2 + .5, h // 2 + .5, 1., nan=True)
        add(.5, .5, .5); expect[0] = add(.25, .75, .5)
    n = len(conf)
    cam = cam_points(K, uvz)
    opts = world(sr.inv(T.double()), cam)
    conf = torch.tensor(conf, dtype=F32)[None]
    rgb = torch.rand(3, n, generator=g) * 255
    rgb[1] = torch.arange(n).float()
    rgb[0, torch.tensor(nanrgb)] = math.nan
    if nan_plane:
        rgb[2] = math.nan
    return dict(K=K, T=T, opts=opts, rgb=rgb, conf=conf, h=h, w=w, expect=expect)


def zero_conf_scene(h=8, w=12):
    """Pixels whose only surfels have conf 0, +-0 ties, a negative conf below a zero, and -inf alone on a pixel: no background."""
    K = kmat(h, w)
    uvz = [(1.5, 1.5, 4.), (2.5, 1.5, 4.), (2.5, 1.5, 4.), (3.5, 1.5, 4.), (3.5, 1.5, 4.), (4.5, 1.5, 4.), (4.5, 1.5, 4.), (5.5, 1.5, 4.)]
    conf = [0., 0., -0., -0., 0., 0., -.5, -math.inf]
    winners = {1 * w + 1: 0, 1 * w + 2: 2, 1 * w + 3: 4, 1 * w + 4: 5, 1 * w + 5: 7}
    n = len(conf)
    rgb = torch.stack((10. + torch.arange(n), torch.arange(n).float(), 20. + torch.arange(n)))
    return dict(K=K, T=pose('identity'), opts=to_f32_exact(cam_points(K, uvz)), rgb=rgb, conf=torch.tensor(conf)[None], h=h, w=w, expect=winners)


def render_negzero_scene(axis, h=8, w=12):
    """u == -0.0 (axis 'u') or v == -0.0 (axis 'v') in the render: in the image, column / row 0 by truncation.  Under the mirrored K
    the row of K gives (-16 * +0) + (0 * negative) + (-0 * z) = -0 for surfel 1 and +0 for surfel 2 (0 * positive); surfel 0 is a
    low-conf bystander on surfel 1's pixel, so the -0.0 surfel must win it.  Points in camera space, T the identity."""
    K = kmat(h, w, mirror=axis)
    if axis == 'u':
        cam = [(-.125, -.375, 4.), (0., -.5, 4.), (0., .5, 4.)]          # (u, v) = (.5, 2.5), (-0, 2), (+0, 6)
        expect = {2 * w + 0: 1, 6 * w + 0: 2}
    else:
        cam = [(-.375, -.125, 4.), (-.5, 0., 4.), (.5, 0., 4.)]          # (u, v) = (4.5, .5), (4, -0), (8, +0)
        expect = {0 * w + 4: 1, 0 * w + 8: 2}
    rgb = torch.tensor([[31., 32., 33.], [0., 1., 2.], [41., 42., 43.]])
    return dict(K=K, T=pose('identity'), opts=torch.tensor(cam).T.contiguous(), rgb=rgb, conf=torch.tensor([[.125, .5, .5]]), h=h, w=w,
                expect=expect)


def edge_render_scenes():
    """(name, scene) of every section-5 render scene: the shapes under the identity, with and without a NaN plane, the zero-conf
    scene and the two negative-zero scenes."""
    out = [(f'{h}x{w}{"-nan_plane" if nanp else ""}', render_scene(h, w, 'identity', nanp)) for h, w in RENDER_SHAPES for nanp in (False, True)]
    return out + [('zero_conf', zero_conf_scene()), ('negzero_u', render_negzero_scene('u')), ('negzero_v', render_negzero_scene('v'))]


def render_truth(s, depth_transformed, dtype):
    img, depth, confidence, mask, winner, _ = sr.render(s['opts'], s['rgb'], s['conf'], s['K'], s['T'], (s['h'], s['w']), depth_transformed, dtype)
    return dict(img=img, depth=depth, confidence=confidence, mask=mask, winner=winner)


def check_exact_render(s, depth_transformed):
    a, b = (render_truth(s, depth_transformed, d) for d in (F32, F64))
    assert torch.equal(a['winner'], b['winner']) and torch.equal(a['mask'], b['mask']), 'float32 and float64 pick different winners'
    assert same(a['confidence'], b['confidence'])
    for pix, i in s['expect'].items():
        assert int(b['winner'][pix]) == i, f'pixel {pix}: the truth shows surfel {int(b["winner"][pix])}, the scene was built for {i}'
    return a, b


RENDER_SHAPES = [(3, 3), (3, 5), (5, 3), (8, 12)]


# ---------------------------------------------------------------------------------------------------------------- prune
def prune_keep(conf, t_created, tick, t_max):
    """remove_surfels_by_confidence_and_time's mask on float32 rows (the arithmetic is exact: small integers and comparisons)."""
    return (conf >= 1.0) | ((tick - t_created) < t_max)


def prune_rows(n, pattern, tick=20, t_max=6, seed=0):
    """(8, n) int32 rows of a map to prune and the kept mask: rows 0-5 are seeded random bits; conf and t_created are set so that
    exactly the pattern's items are kept, alternately by confidence and by age."""
    g = torch.Generator().manual_seed(seed * 7919 + n)
    i = torch.arange(n)
    if pattern == 'all':
        keep = torch.ones(n, dtype=torch.bool)
    elif pattern == 'none':
        keep = torch.zeros(n, dtype=torch.bool)
    elif pattern == 'first':
        keep = i == 0
    elif pattern == 'last':
        keep = i == n - 1
    elif pattern == 'tiles':                                      # every other whole tile of 1024 keeps nothing
        keep = (i // 1024) % 2 == 1
    else:
        keep = torch.rand(n, generator=g) < .3
    rows = torch.randint(-2 ** 31, 2 ** 31 - 1, (8, n), generator=g, dtype=torch.int64).to(torch.int32)
    by_conf = keep & (i % 2 == 0)
    conf = torch.where(by_conf, torch.tensor(1.), torch.tensor(.5))
    t = torch.where(keep & ~by_conf, torch.tensor(float(tick - t_max + 1)), torch.tensor(float(tick - t_max)))
    rows[6], rows[7] = conf.view(torch.int32), t.view(torch.int32)
    assert torch.equal(prune_keep(conf, t, tick, t_max), keep)
    return rows, keep


PRUNE_SIZES = [0, 1, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 1024 * 1024 - 1, 1024 * 1024, 1024 * 1024 + 1, 1024 * 1025 + 3]
PRUNE_PATTERNS = ['all', 'none', 'first', 'last', 'tiles', 'random']


def prune_edge_rows(tick=20, t_max=6):
    """The predicate's edges in one small map: (conf, t_created, kept)."""
    nan, inf = math.nan, math.inf
    below = float(np.nextafter(np.float32(1), np.float32(0)))
    cases = [(.5, tick - t_max, False), (.5, tick - t_max + 1, True), (1., 0., True), (below, 0., False), (inf, 0., True),
             (nan, tick, True), (nan, 0., False), (.5, nan, False), (1., nan, True), (-inf, tick, True), (2., -inf, True), (.5, inf, True)]
    rows = torch.arange(8 * len(cases), dtype=torch.int32).reshape(8, -1) + 1000
    rows[6] = torch.tensor([c[0] for c in cases]).view(torch.int32)
    rows[7] = torch.tensor([float(c[1]) for c in cases]).view(torch.int32)
    return rows, torch.tensor([c[2] for c in cases])
