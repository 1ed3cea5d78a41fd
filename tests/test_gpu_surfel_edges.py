"""GPU: the surfel-map kernels (csrc/surfel.hip) at their edges against float64.

Truth is the float64 run of the plain-torch restatement (tests/surfel_ref.py); its float32 run is the yardstick.  On the exact scenes
of tests/surfel_edges.py every decision -- the kept set and its order, counts, t_created, which surfels associate, which pixels append,
render winners, masks, overflow words -- is the same in both precisions (asserted first, on the CPU, in every test) and the kernels
must take it exactly: no surfel is set aside.  Values (averaged opts / rgb / conf, transformed points, rendered depth, NaN-filled planes)
must stay within twice the float32 restatement's own error against float64, and equal where that error is 0.

The C ABI is driven directly (``Map``: a (8, cap) block and its two words inside sentinel-filled buffers) where SurfelMap hides a knob
-- cap, n_bound, the count and overflow words, kinv --, and through SurfelMap where the method is under test."""
import ctypes

import pytest
import torch

import surfel_edges as se
import surfel_ref as sr

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32, F64 = torch.float32, torch.float64
SENT = 0x5EA7BEEF                                # sentinel word around every destination
GUARD = 256


def _lib():
    from rpe_amd import _lib as L
    return L


@pytest.fixture(scope='module', autouse=True)
def _print_worst_value_ratios():
    """After the module's tests: the worst kernel error / float32-restatement error the value checks met, per section (NOTES.md)."""
    yield
    for section, r in sorted(se.RATIOS.items()):
        print(f'worst kernel error / float32 restatement error, {section}: {r:.3f}')


def _i32(t):
    t = t.detach().contiguous()
    return t.view(torch.uint8) if t.dtype in (torch.bool, torch.uint8) else t.view(torch.int32)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(_i32(a.cpu()), _i32(b.cpu()))


class Map:
    """A map for the C ABI: an (8, cap) block (rows 0-2 opts, 3-5 rgb, 6 conf, 7 t_created) between two guards of sentinel words, and
    the count / overflow words in the middle of another sentinel buffer."""

    def __init__(self, cap, rows=None, count=None):
        self.cap = cap
        self.big = torch.full((2 * GUARD + 8 * cap,), SENT, dtype=torch.int32, device=DEV)
        self.words = torch.full((2 * GUARD + 2,), SENT, dtype=torch.int32, device=DEV)
        self.block = self.big[GUARD:GUARD + 8 * cap].view(8, cap)
        n = 0 if rows is None else rows.shape[1]
        if n:
            self.block[:, :n] = _i32(rows).to(DEV)
        self.words[GUARD] = n if count is None else count
        self.words[GUARD + 1] = 0

    def desc(self):
        base, cap, w = self.block.data_ptr(), self.cap, self.words.data_ptr() + 4 * GUARD
        return _lib().SurfelMapDesc(base, base + 3 * cap * 4, base + 6 * cap * 4, base + 7 * cap * 4, cap, w, w + 4)

    @property
    def count(self):
        return int(self.words[GUARD])

    @property
    def overflow(self):
        return int(self.words[GUARD + 1])

    def rows(self, n):
        return self.block[:, :n].cpu()

    def floats(self, n):
        return self.rows(n).view(F32)

    def assert_guards(self, used):
        """Nothing outside the first ``used`` columns of each row and the two words was written."""
        assert bool((self.big[:GUARD] == SENT).all()) and bool((self.big[GUARD + 8 * self.cap:] == SENT).all()), 'a guard was written'
        assert bool((self.block[:, used:] == SENT).all()), f'columns past {used} were written'
        w = self.words.clone()
        w[GUARD:GUARD + 2] = SENT
        assert bool((w == SENT).all()), 'a word next to count / overflow was written'


def _ws(n_bound, h, w):
    return torch.empty(max(int(_lib().lib().rpe_surfel_workspace_bytes(n_bound, h, w)), 1) + 256, dtype=torch.uint8, device=DEV)


def _scene_rows(s):
    return torch.cat((s['opts'], s['rgb'], s['conf'], s['t_created'])).to(F32)


def _frame_dev(s):
    return dict(depth=s['depth'].to(DEV).contiguous(), img=s['img'].to(DEV).contiguous(), mask=s['mask'].to(DEV).to(torch.uint8).contiguous(),
                K=s['K'].to(DEV).contiguous(), kinv=s['kinv'].to(DEV).contiguous(), pose=s['pose'].to(DEV).contiguous())


def fuse_direct(s, src, dst, n_bound, average, t_max, conf_thr):
    L = _lib()
    f = _frame_dev(s)
    ws = _ws(n_bound, s['h'], s['w'])
    p = L.ptr
    L.check(L.lib().rpe_surfel_fuse(src.desc(), n_bound, p(f['depth']), p(f['img']), p(f['mask']), s['h'], s['w'], p(f['K']), p(f['kinv']),
                                    p(f['pose']), float(s['d_thresh']), int(average), 1, float(conf_thr), int(s['tick']), int(t_max),
                                    dst.desc(), p(ws), L.stream_ptr()), 'rpe_surfel_fuse')
    torch.cuda.synchronize()


def prune_direct(src, dst, n_bound, tick, t_max):
    L = _lib()
    ws = _ws(n_bound, 1, 1)
    L.check(L.lib().rpe_surfel_prune(src.desc(), n_bound, tick, t_max, dst.desc(), L.ptr(ws), L.stream_ptr()), 'rpe_surfel_prune')
    torch.cuda.synchronize()


def _check_fused(s, case, r32, r64, got, n_old):
    """got: the (8, count) float rows the kernel left; r32 / r64: the restatement's results."""
    average = case[0]
    assert got.shape[1] == r64['n']
    assert torch.equal(got[7:8].double(), r64['t_created']), 't_created: the kept set or its order differs'
    kept_old = int(r64['keep'][:n_old].sum())
    pixels = torch.nonzero(r64['new']).reshape(-1)[r64['keep'][n_old:]]
    assert torch.equal(got[3, kept_old:], s['img'].reshape(3, -1)[0, pixels]), 'the appended pixels differ'
    if not average:
        assert se.same(got[3:6], r64['rgb']), 'rgb names the kept surfels and appended pixels: the kept set differs'
    tag = f"fuse {s.get('tag', '')} avg={case[0]} t_max={case[1]} conf_thr={case[2]}"
    se.check_values(f'{tag} opts', got[0:3], r32['opts'], r64['opts'], 'fuse')
    se.check_values(f'{tag} rgb', got[3:6], r32['rgb'], r64['rgb'], 'fuse')
    se.check_values(f'{tag} conf', got[6:7], r32['conf'], r64['conf'], 'fuse')


# ================================================================================================ 2. fuse at exact boundaries
@pytest.mark.parametrize('case', se.FUSE_CASES, ids=lambda c: f'avg{int(c[0])}-tmax{c[1]}-thr{c[2]}')
@pytest.mark.parametrize('pose', ['identity', 'shift', 'turn'])
def test_fuse_association_update_append_prune_at_exact_boundaries(rpe, pose, case):
    s = se.fuse_scene(pose)
    s['tag'] = pose
    r32, r64 = se.check_exact_fuse(s, *case)                        # precondition: float32 and float64 decide alike
    assert torch.equal(r64['flags'], s['expect'])
    n = s['opts'].shape[1]
    before = _scene_rows(s)
    src, dst = Map(n + 7, before), Map(n + 96 + 5)
    fuse_direct(s, src, dst, n, *case)
    assert dst.overflow == 0 and src.overflow == 0 and src.count == n
    # which surfels associated: fuse updates them in place in the source (conf moves unless it is NaN; opts / rgb with average_pts)
    changed = (_i32(before) != src.rows(n)).any(0)
    hidden = torch.isnan(s['conf'][0]) & (not case[0])
    assert torch.equal(changed, r64['flags'] & ~hidden), [nm for nm, a, b in zip(s['names'], changed, r64['flags'] & ~hidden) if a != b]
    src.assert_guards(n)
    assert dst.count == r64['n'], f"{dst.count} surfels, the truth has {r64['n']}"
    dst.assert_guards(dst.count)
    got = dst.floats(dst.count)
    _check_fused(s, case, r32, r64, got, n)
    by_name = dict(zip(s['names'], src.floats(n)[6]))
    if case[2] == 7:
        assert float(by_name['clamp']) == 1.0 and torch.isnan(by_name['nanconf'])
    if case[1] < 2 and case[2] == 7:
        assert dst.count == 2 and got[6].tolist() == [1.0, 1.0]      # this frame's surfels went again; 'clamp' and 'stable' stay


def test_fuse_negative_zero_coordinate_is_inside(rpe):
    s = se.negzero_scene()
    r32, r64 = se.check_exact_fuse(s, True, 2, 7)
    assert bool(r64['flags'].all())
    src, dst = Map(4, _scene_rows(s)), Map(2 + 96)
    fuse_direct(s, src, dst, 2, True, 2, 7)
    assert dst.count == r64['n'] == 96 and dst.overflow == 0         # two surfels, two matched pixels: (2, 0) and (6, 0)
    _check_fused(s, (True, 2, 7), r32, r64, dst.floats(dst.count), 2)


@pytest.mark.parametrize('h,w,n,n_bound,mask', [(8, 12, 0, 0, True), (8, 12, 0, 6, True), (8, 12, 3, 3, False), (1, 1, 2, 2, True),
                                                (8, 1, 2, 2, True)])
def test_fuse_empty_inputs(rpe, h, w, n, n_bound, mask):
    """n = 0 under n_bound = 0 (no update launch) and under n_bound > 0; an all-false mask; h = w = 1 and w = 1, where no surfel can be
    in bounds (u < w - 1 = 0) and only the pixel items matter."""
    s = se.small_scene(h, w, n, mask)
    r32, r64 = se.check_exact_fuse(s, True, 2, 7)
    src, dst = Map(max(n, n_bound, 1) + 3, _scene_rows(s)), Map(n + h * w + 1)
    fuse_direct(s, src, dst, n_bound, True, 2, 7)
    assert dst.count == r64['n'] == n + (h * w if mask else 0) and dst.overflow == 0
    assert _bits_equal(src.rows(n), _scene_rows(s))                  # nothing associated
    dst.assert_guards(dst.count)
    _check_fused(s, (True, 2, 7), r32, r64, dst.floats(dst.count), n)


# ================================================================================================ 3. prune and the compaction scan
TICK, TMAX = 20, 6


@pytest.mark.parametrize('n', se.PRUNE_SIZES)
def test_prune_compaction_at_tile_wave_and_scan_boundaries(rpe, n):
    """Truth: torch's boolean-mask gather of the same rows on the CPU, compared bit for bit.  n_bound == n and n + 1500 (blocks past
    the count); the last three sizes put the scan at one and at two blocks per scan thread."""
    for pattern in se.PRUNE_PATTERNS:
        rows, keep = se.prune_rows(n, pattern, TICK, TMAX)
        truth = rows[:, keep]
        src = Map(n + 1500, rows)
        for n_bound in (n, n + 1500):
            dst = Map(max(n, 1))
            prune_direct(src, dst, n_bound, TICK, TMAX)
            assert dst.count == truth.shape[1], (pattern, n_bound, dst.count, truth.shape[1])
            assert dst.overflow == 0
            assert torch.equal(dst.rows(dst.count), truth), (pattern, n_bound)
            dst.assert_guards(dst.count)
        assert torch.equal(src.rows(n), rows) and src.count == n     # the source is only read


def test_prune_predicate_edges(rpe):
    rows, keep = se.prune_edge_rows(TICK, TMAX)
    n = rows.shape[1]
    src, dst = Map(n, rows), Map(n)
    prune_direct(src, dst, n, TICK, TMAX)
    assert dst.count == int(keep.sum()) and dst.overflow == 0
    assert torch.equal(dst.rows(dst.count), rows[:, keep]), (dst.rows(dst.count)[0] - 1000).tolist()


def _surfel_map(opts, rgb, conf, K, shape, t_created=None, tick=0, **kw):
    from rpe_amd.surfel_map import SurfelMap
    m = SurfelMap(opts=opts.to(DEV), rgb=rgb.to(DEV), conf=conf.to(DEV), kmat=K.to(DEV), img_shape=shape, **kw)
    assert torch.equal(m._kinv.cpu(), se.kinv(K))                    # torch.linalg.inv of the dyadic K is the exact inverse
    if t_created is not None:
        m._buf[m._cur][7, :opts.shape[1]] = t_created.reshape(-1).to(DEV)
    m.tick = tick
    return m


def test_prune_method_returns_the_kernels_mask_and_keeps_the_host_bound_valid(rpe):
    s = se.fuse_scene('identity')
    n = s['opts'].shape[1]
    m = _surfel_map(s['opts'], s['rgb'], s['conf'], s['K'], (8, 12), s['t_created'], tick=se.TICK + 1, d_thresh=8.0, t_max=2, conf_thr=7,
                    average_pts=True)
    before = torch.cat((m.opts, m.rgb, m.conf, m.t_created)).cpu()
    truth = se.prune_keep(s['conf'][0], s['t_created'][0], se.TICK + 1, 2)
    assert 1 < int(truth.sum()) < n
    mask = m.remove_surfels_by_confidence_and_time()
    assert torch.equal(mask.cpu(), truth)
    assert m.n == int(mask.sum()) and m.overflowed == 0
    assert _bits_equal(torch.cat((m.opts, m.rgb, m.conf, m.t_created)), before[:, truth])
    # a following fuse: the host bound (still n) covers the pruned count
    from rpe_amd.pose_estimator import Frame
    from rpe_amd.se3 import SE3
    s2 = dict(s, opts=before[0:3, truth], rgb=before[3:6, truth], conf=before[6:7, truth], t_created=before[7:8, truth], tick=se.TICK + 1)
    r32, r64 = se.check_exact_fuse(s2, True, 2, 7)
    m.fuse(Frame(s['img'][None].to(DEV), depth=s['depth'][None, None].to(DEV), mask=s['mask'][None, None].to(DEV)),
           SE3(s['pose'].reshape(1, 7).to(DEV)))
    assert m.n == r64['n'] and m.overflowed == 0 and m.tick == se.TICK + 2
    _check_fused(s2, (True, 2, 7), r32, r64, torch.cat((m.opts, m.rgb, m.conf, m.t_created)).cpu(), int(truth.sum()))


# ================================================================================================ 4. the overflow contract
@pytest.mark.parametrize('pattern,cap', [('all', 1500), ('all', 1024), ('all', 2048), ('all', 1), ('tiles', 1024), ('tiles', 1), ('random', 500)])
def test_prune_overflow_writes_the_first_cap_items_and_nothing_else(rpe, pattern, cap):
    """include/rpe.h: a kernel that would write past cap ORs 1 into *overflow, writes nothing past cap and stores n = cap.  Caps in the
    middle of a tile, on a tile boundary (1024, 2048; with 'tiles' the first tile keeps nothing, so whole later blocks start at
    j == cap) and 1."""
    n = 5000
    rows, keep = se.prune_rows(n, pattern, TICK, TMAX)
    truth = rows[:, keep]
    assert truth.shape[1] > cap
    src, dst = Map(n, rows), Map(cap)
    prune_direct(src, dst, n, TICK, TMAX)
    assert dst.count == cap and dst.overflow & 1 and not dst.overflow & 2
    for r in range(8):                                               # row k's overflow would land in row k + 1's head
        assert torch.equal(dst.rows(cap)[r], truth[r, :cap]), f'row {r}'
    dst.assert_guards(cap)


@pytest.mark.parametrize('cap', [1, 20, 31, 50, 107])
def test_fuse_overflow_writes_the_first_cap_items_and_nothing_else(rpe, cap):
    s = se.fuse_scene('identity')
    case = (True, 2, 7)
    _, r64 = se.check_exact_fuse(s, *case)
    n = s['opts'].shape[1]
    assert r64['n'] == 108 > cap
    full = Map(n + 96)
    fuse_direct(s, Map(n, _scene_rows(s)), full, n, *case)
    assert full.count == 108 and full.overflow == 0
    dst = Map(cap)
    fuse_direct(s, Map(n, _scene_rows(s)), dst, n, *case)
    assert dst.count == cap and dst.overflow == 1
    assert torch.equal(dst.rows(cap), full.rows(108)[:, :cap])
    assert torch.equal(dst.floats(cap)[7:8].double(), r64['t_created'][:, :cap])
    dst.assert_guards(cap)


def test_wrong_host_bound_sets_bit_2_and_stays_inside(rpe):
    """*count = n_bound + 5: rpe.h promises the bit, count <= cap and no write outside the destination; nothing else."""
    rows, keep = se.prune_rows(2000, 'random', TICK, TMAX)
    for cap in (2000, 300):
        src, dst = Map(2000, rows), Map(cap)
        prune_direct(src, dst, 1995, TICK, TMAX)
        assert dst.overflow & 2 and 0 <= dst.count <= cap
        dst.assert_guards(dst.count)
    s = se.fuse_scene('identity')
    n = s['opts'].shape[1]
    src, dst = Map(n, _scene_rows(s)), Map(n + 96)
    fuse_direct(s, src, dst, n - 5, True, 2, 7)
    assert dst.overflow & 2 and 0 <= dst.count <= dst.cap
    dst.assert_guards(dst.count)
    src.assert_guards(n)


def test_overflowed_reports_either_word_and_growth_never_sets_it(rpe):
    from rpe_amd.pose_estimator import Frame
    from rpe_amd.se3 import SE3
    from rpe_amd.surfel_map import SurfelMap
    s = se.fuse_scene('identity')
    m = _surfel_map(s['opts'], s['rgb'], s['conf'], s['K'], (8, 12))
    assert m.overflowed == 0
    m._cnt[m._cur][1] = 1
    assert m.overflowed == 1
    m._cnt[1 - m._cur][1] = 2
    assert m.overflowed == 3
    # a map that starts at capacity h * w and grows through _grow_for: three fuses at d_thresh 0 (nothing associates, every pixel appends)
    depth = torch.full((1, 1, 8, 12), 4.)
    fr = Frame(s['img'][None].to(DEV), depth=depth.to(DEV), mask=torch.ones(1, 1, 8, 12, dtype=torch.bool, device=DEV),
               confidence=torch.ones(1, 1, 8, 12, device=DEV))
    g = SurfelMap(frame=fr, kmat=s['K'].to(DEV), pmat=SE3(s['pose'].reshape(1, 7).to(DEV)), d_thresh=0.0, t_max=15, conf_thr=7)
    assert g.capacity == 96 and g.n == 96
    for k in range(3):
        g.fuse(fr, SE3(s['pose'].reshape(1, 7).to(DEV)))
        assert g.n == 96 * (k + 2) and g.overflowed == 0
    assert g.capacity >= 384


# ================================================================================================ 5. render
def _render(s, depth_transformed, m=None):
    from rpe_amd.se3 import SE3
    m = m or _surfel_map(s['opts'], s['rgb'], s['conf'], s['K'], (s['h'], s['w']))
    T = SE3(s['T'].reshape(1, 7).to(DEV))
    fr = (m.render_transformed if depth_transformed else m.render)(s['K'].to(DEV), T)[0]
    return dict(img=fr.img[0].cpu(), depth=fr.depth[0, 0].cpu(), confidence=fr.confidence[0, 0].cpu(), mask=fr.mask[0, 0].cpu())


def _check_render(tag, got, r32, r64):
    assert torch.equal(got['mask'], r64['mask']), f'{tag}: mask'
    assert se.same(got['confidence'], r64['confidence']), f'{tag}: confidence (the winners)'
    assert se.same(got['img'][1], r64['img'][1]), f'{tag}: channel 1 names the winner of every pixel'
    assert not bool(torch.isnan(got['img']).any()) and not bool(torch.isnan(got['depth']).any())
    se.check_values(f'{tag} img', got['img'], r32['img'], r64['img'], 'render')
    se.check_values(f'{tag} depth', got['depth'], r32['depth'], r64['depth'], 'render')


@pytest.mark.parametrize('nan_plane', [False, True], ids=['', 'nan_plane'])
@pytest.mark.parametrize('pose', ['identity', 'shift', 'turn'])
@pytest.mark.parametrize('h,w', se.RENDER_SHAPES)
def test_render_coordinates_key_order_and_nan_fill(rpe, h, w, pose, nan_plane):
    s = se.render_scene(h, w, pose, nan_plane)
    for dt in (False, True):
        r32, r64 = se.check_exact_render(s, dt)                      # precondition, and the winners the scene was built for
        got = _render(s, dt)
        _check_render(f'render {h}x{w} {pose} dt={int(dt)}', got, r32, r64)
        if nan_plane:
            assert bool((got['img'][2] == 0).all())                  # NaN neighbours are read as 0: the plane fills to 0


def test_render_zero_and_negative_confidence_winners(rpe):
    s = se.zero_conf_scene()
    r32, r64 = se.check_exact_render(s, False)
    got = _render(s, False)
    _check_render('render zero-conf', got, r32, r64)
    assert int(got['mask'].sum()) == 1 and bool(got['mask'][1, 5])   # -inf alone on its pixel beats "empty"; conf 0 winners: mask 0 ...
    assert got['img'][0, 1, 1:6].tolist() == [10., 12., 14., 15., 17.] and bool((got['depth'][1, 1:6] == 4).all())      # ... but drawn


@pytest.mark.parametrize('axis', ['u', 'v'])
def test_render_negative_zero_coordinate_is_inside(rpe, axis):
    """u == -0.0 / v == -0.0 (the mirrored K): -0 >= 0 holds and (int)-0.0 is 0, so the surfel lands in column / row 0 and wins it."""
    s = se.render_negzero_scene(axis)
    y, x = (2, 0) if axis == 'u' else (0, 4)
    for dt in (False, True):
        r32, r64 = se.check_exact_render(s, dt)                      # precondition, and that surfel 1 is the winner of its pixel
        got = _render(s, dt)
        _check_render(f'render negzero {axis} dt={int(dt)}', got, r32, r64)
        assert float(got['img'][1, y, x]) == 1. and float(got['confidence'][y, x]) == .5 and int(got['mask'].sum()) == 2


@pytest.mark.parametrize('n,n_bound', [(0, 0), (0, 40)])
def test_render_empty_map(rpe, n, n_bound):
    s = se.render_scene(8, 12, 'identity')
    m = _surfel_map(s['opts'], s['rgb'], s['conf'], s['K'], (8, 12))
    m._cnt[m._cur][0] = 0                                            # count = 0 under the host bound of the full map
    if n_bound == 0:
        m._n_ub = 0
    got = _render(s, True, m)
    assert all(not bool(got[k].any()) for k in ('img', 'depth', 'confidence', 'mask'))


# ================================================================================================ 6. transform
def _general_pose(trans=30., rot=1.):
    from oracle import se3 as ose3
    g = torch.Generator().manual_seed(5)
    return ose3.se3_exp(torch.randn(6, generator=g, dtype=F64) * torch.tensor([trans] * 3 + [rot] * 3, dtype=F64)).float()


def transform_direct(src, in_cap, out, out_cap, count, n_bound, T):
    L = _lib()
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    Td = T.to(DEV).contiguous()
    st = L.lib().rpe_surfel_transform(L.ptr(src), in_cap, L.ptr(out), out_cap, L.ptr(cnt), n_bound, L.ptr(Td), L.stream_ptr())
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize('pose', ['identity', 'shift', 'turn', 'general'])
def test_transform_direct_strides_bounds_and_untouched_columns(rpe, pose):
    T = _general_pose() if pose == 'general' else se.pose(pose, se.RENDER_POSES)
    g = torch.Generator().manual_seed(9)
    count, n_bound, in_cap, out_cap = 700, 900, 1000, 1300
    pts = (torch.randint(-2 ** 12, 2 ** 12, (3, count), generator=g).float() / 64) if pose != 'general' else torch.randn(3, count, generator=g) * 50
    r32, r64 = sr.act(T, pts, F32), sr.act(T, pts, F64)
    if pose != 'general':
        assert torch.equal(r32.double(), r64)                        # the exact poses on dyadic points: float32 is the truth
    for in_place in (False, True):
        src = torch.full((3, in_cap), 12345., device=DEV)
        src[:, :count] = pts.to(DEV)
        out = src if in_place else torch.full((3 * out_cap + 64,), 12345., device=DEV)
        oc = in_cap if in_place else out_cap
        assert transform_direct(src, in_cap, out, oc, count, n_bound, T) == 0
        res = out.reshape(-1)[:3 * oc].reshape(3, oc).cpu()
        se.check_values(f'transform {pose} in_place={in_place}', res[:, :count], r32, r64, 'transform')
        assert bool((res[:, count:] == 12345.).all())                 # [count, n_bound) and beyond: untouched
        if not in_place:
            assert bool((out[3 * oc:] == 12345.).all()) and torch.equal(src[:, :count].cpu(), pts)
    out = torch.full((3, 8), 12345., device=DEV)
    assert transform_direct(out, 8, out, 8, 5, 0, T) == 0 and bool((out == 12345.).all())      # n_bound = 0: OK, nothing written


@pytest.mark.parametrize('pose', ['shift', 'turn', 'general'])
def test_transform_methods_and_render_transformed(rpe, pose):
    from rpe_amd.se3 import SE3
    s = se.render_scene(8, 12, pose if pose != 'general' else 'identity')
    T = _general_pose(.3, .02) if pose == 'general' else s['T']          # (a small motion: most of the scene stays in view)
    n = s['opts'].shape[1]
    m = _surfel_map(s['opts'], s['rgb'], s['conf'], s['K'], (8, 12), torch.arange(n).float(), tick=4)
    before = torch.cat((m.opts, m.rgb, m.conf, m.t_created)).cpu()
    Td = SE3(T.reshape(1, 7).to(DEV))
    cp = m.transform_cpy(Td)
    assert _bits_equal(torch.cat((m.opts, m.rgb, m.conf, m.t_created)), before) and m.tick == 4      # the source map is untouched
    assert cp.tick == 0 and cp.n == n and not bool(cp.t_created.any())
    assert _bits_equal(cp.rgb, before[3:6]) and _bits_equal(cp.conf, before[6:7])
    r32, r64 = sr.act(T, s['opts'], F32), sr.act(T, s['opts'], F64)
    se.check_values(f'transform_cpy {pose}', cp.opts.cpu(), r32, r64, 'transform')
    a, b = m.render_transformed(s['K'].to(DEV), Td)[0], cp.render(s['K'].to(DEV))[0]
    for name in ('img', 'depth', 'confidence', 'mask'):
        assert _bits_equal(getattr(a, name), getattr(b, name)), name
    m.transform(Td)                                                  # in place: the same points as the copy's
    assert _bits_equal(m.opts, cp.opts) and _bits_equal(m.t_created, before[7:8])


def _section5_scenes():
    out = se.edge_render_scenes()
    out += [(f'{h}x{w}-{p}', se.render_scene(h, w, p)) for h, w in se.RENDER_SHAPES for p in ('shift', 'turn')]
    return out


@pytest.mark.parametrize('name,s', _section5_scenes(), ids=[n for n, _ in _section5_scenes()])
def test_render_transformed_is_transform_cpy_then_render(rpe, name, s):
    """``render_transformed(K, T)`` against ``transform_cpy(T).render(K)``, bit for bit, on every render scene of this file: all
    shapes (3-pixel axes included) under each exact pose, the NaN planes, the zero-conf winners and the negative-zero coordinates."""
    from rpe_amd.se3 import SE3
    m = _surfel_map(s['opts'], s['rgb'], s['conf'], s['K'], (s['h'], s['w']))
    Td = SE3(s['T'].reshape(1, 7).to(DEV))
    a, b = m.render_transformed(s['K'].to(DEV), Td)[0], m.transform_cpy(Td).render(s['K'].to(DEV))[0]
    for key in ('img', 'depth', 'confidence', 'mask'):
        assert _bits_equal(getattr(a, key), getattr(b, key)), key
    r64 = se.render_truth(s, True, F64)
    assert torch.equal(a.mask[0, 0].cpu(), r64['mask']) and se.same(a.img[0, 1].cpu(), r64['img'][1])      # and both show the truth's winners


def test_grid_pts_of_a_full_mask_init(rpe):
    from rpe_amd.pose_estimator import Frame
    from rpe_amd.se3 import SE3
    from rpe_amd.surfel_map import SurfelMap
    h, w = 8, 12
    K, T = se.kmat(h, w), _general_pose()
    g = torch.Generator().manual_seed(3)
    depth = 1 + 9 * torch.rand(1, 1, h, w, generator=g)
    img = torch.rand(1, 3, h, w, generator=g)
    fr = Frame(img.to(DEV), depth=depth.to(DEV), mask=torch.ones(1, 1, h, w, dtype=torch.bool, device=DEV), confidence=torch.ones(1, 1, h, w, device=DEV))
    m = SurfelMap(frame=fr, kmat=K.to(DEV), pmat=SE3(T.reshape(1, 7).to(DEV)))
    grid = m.grid_pts
    assert tuple(grid.shape) == (h, w, 3) and m.n == h * w
    r32, r64 = (sr.frame_points(K, depth[0, 0], T, d, se.kinv(K)) for d in (F32, F64))
    se.check_values('grid_pts', grid.cpu().reshape(-1, 3).T, r32, r64, 'transform')
    assert _bits_equal(m.rgb, img[0].reshape(3, -1))


# ================================================================================================ 7. K maps per launch
# The argument table of a _many call is a 1040-byte head (ManyHead, 16-aligned) followed by K structs of 216 (CompactArgs), 240
# (RenderArgs) or 136 + 216 (FuseArgs + CompactArgs) bytes, put into the workspace in 2048-byte k_put chunks.  No K <= 64 makes any of
# the three tables end exactly on a chunk boundary (1040 + 216 K, 1040 + 240 K and 1040 + 352 K (+ 8 for odd K) are never multiples of
# 2048 there); the nearest are init with K = 33 (8168 bytes, 24 short of four chunks) and render with K = 4 (2000 bytes, 48 short of
# one).  Both are run below next to K = 64 (init 14864, render 16400, fuse 23568 bytes: 8, 9 and 12 chunks).
def _pattern(K):
    """empty, empty, full, empty, full, ..., ending in two empties: a leading run, a trailing run and single empty segments."""
    full = [False, False] + [k % 2 == 0 for k in range(K - 4)] + [False, False]
    return full[:K]


def _state(m):
    return m.n, m.overflowed, m.tick, torch.cat((m.opts, m.rgb, m.conf, m.t_created)).cpu()


@pytest.mark.parametrize('K', [64, 4])
def test_render_many_at_the_map_limit_with_runs_of_empty_maps(rpe, K):
    from rpe_amd import surfel_map
    from rpe_amd.se3 import SE3
    poses = ['identity', 'shift', 'turn']
    maps, Ts = [], []
    for k, full in enumerate(_pattern(K)):
        s = se.render_scene(8, 12, poses[k % 3], nan_plane=k % 5 == 0, seed=k)
        n = s['opts'].shape[1] if full else 0
        maps.append(_surfel_map(s['opts'][:, :n], s['rgb'][:, :n], s['conf'][:, :n], s['K'], (8, 12)))
        Ts.append(s['T'])
    Ks = torch.stack([se.kmat(8, 12)] * K).to(DEV)
    Ts = torch.stack(Ts).to(DEV)
    for dt in (True, False):
        fr = surfel_map.render_many(maps, Ks, Ts, depth_transformed=dt)
        for k, m in enumerate(maps):
            one = (m.render_transformed if dt else m.render)(Ks[k], SE3(Ts[k:k + 1]))[0]
            for name in ('img', 'depth', 'confidence', 'mask'):
                assert _bits_equal(getattr(fr, name)[k:k + 1], getattr(one, name)), (k, name)
            assert bool(fr.mask[k].any()) == (m.n > 0)


def _fuse_maps(K, case):
    poses = ['identity', 'shift', 'turn']
    scenes = [se.fuse_scene(p) for p in poses]
    maps = []
    for k, full in enumerate(_pattern(K)):
        s = scenes[k % 3]
        n = s['opts'].shape[1] if full else 0
        maps.append(_surfel_map(s['opts'][:, :n], s['rgb'][:, :n], s['conf'][:, :n], s['K'], (8, 12), s['t_created'][:, :n], tick=se.TICK,
                                d_thresh=8.0, average_pts=case[0], t_max=case[1], conf_thr=case[2], capacity=n + 96))
    return scenes, maps


@pytest.mark.parametrize('K', [64, 5])
def test_fuse_many_at_the_map_limit_shared_frame_rows(rpe, K):
    """Map k fuses frame row k % 3 of a batch of three (every row is shared by many maps, the last row included); empty maps append the
    frame.  Bit for bit the single fuse, and the float64 decisions."""
    from rpe_amd import surfel_map
    from rpe_amd.pose_estimator import Frame
    from rpe_amd.se3 import SE3
    case = (True, 2, 7)
    scenes, many = _fuse_maps(K, case)
    _, single = _fuse_maps(K, case)
    fr = Frame(torch.stack([s['img'] for s in scenes]).to(DEV), depth=torch.stack([s['depth'][None] for s in scenes]).to(DEV),
               mask=torch.stack([s['mask'][None] for s in scenes]).to(DEV))
    P = torch.stack([s['pose'] for s in scenes]).to(DEV)
    rows = [k % 3 for k in range(K)]
    surfel_map.fuse_many(many, fr, SE3(P), rows=rows)
    truth = [se.check_exact_fuse(s, *case)[1] for s in scenes]
    for k in range(K):
        r = rows[k]
        single[k].fuse(Frame(fr.img[r:r + 1], depth=fr.depth[r:r + 1], mask=fr.mask[r:r + 1]), SE3(P[r:r + 1]))
        a, b = _state(many[k]), _state(single[k])
        assert a[:3] == b[:3] and a[1] == 0 and _bits_equal(a[3], b[3]), k
        assert a[0] == (truth[r]['n'] if _pattern(K)[k] else 95)      # an empty map takes the 95 masked-in pixels
        if _pattern(K)[k]:
            assert torch.equal(a[3][7:8].double(), truth[r]['t_created'])


@pytest.mark.parametrize('K', [64, 33])
def test_init_many_at_the_map_limit(rpe, K):
    from rpe_amd import surfel_map
    from rpe_amd.pose_estimator import Frame
    from rpe_amd.se3 import SE3
    from rpe_amd.surfel_map import SurfelMap
    s = se.fuse_scene('identity')
    g = torch.Generator().manual_seed(K)
    mask = torch.stack([(torch.rand(1, 8, 12, generator=g) < .7) & full for full in _pattern(K)])
    depth = 1 + 7 * torch.rand(K, 1, 8, 12, generator=g)
    img = torch.rand(K, 3, 8, 12, generator=g)
    conf = 7 * torch.rand(K, 1, 8, 12, generator=g)
    pm = torch.stack([se.pose(['identity', 'shift', 'turn'][k % 3], se.RENDER_POSES) for k in range(K)]).to(DEV)
    Ks = torch.stack([s['K']] * K).to(DEV)
    fr = Frame(img.to(DEV), depth=depth.to(DEV), mask=mask.to(DEV), confidence=conf.to(DEV))
    maps = surfel_map.init_many(fr, Ks, pm)
    for k in range(K):
        one = SurfelMap(frame=Frame(fr.img[k:k + 1], depth=fr.depth[k:k + 1], mask=fr.mask[k:k + 1], confidence=fr.confidence[k:k + 1]),
                        kmat=Ks[k], pmat=SE3(pm[k:k + 1]))
        a, b = _state(maps[k]), _state(one)
        assert a[:3] == b[:3] and a[0] == int(mask[k].sum()) and a[1] == 0 and _bits_equal(a[3], b[3]), k
        r32, r64 = (sr.frame_points(s['K'], depth[k, 0], pm[k].cpu(), d, s['kinv'])[:, mask[k].reshape(-1)] for d in (F32, F64))
        se.check_values(f'init_many map {k}', a[3][0:3], r32, r64, 'init')


def test_fuse_many_with_one_map_overflowing(rpe):
    """K = 3 through the C entry point, the middle map's destination too small: its neighbours are unaffected and its own count,
    overflow word and rows are the single call's."""
    L = _lib()
    case = (True, 2, 7)
    scenes = [se.fuse_scene(p) for p in ('identity', 'shift', 'turn')]
    n = scenes[0]['opts'].shape[1]
    caps = [n + 96, 40, n + 96]

    def run(many):
        src = [Map(n, _scene_rows(s)) for s in scenes]
        dst = [Map(c) for c in caps]
        if not many:
            for k, s in enumerate(scenes):
                fuse_direct(s, src[k], dst[k], n, *case)
            return src, dst
        f = [_frame_dev(s) for s in scenes]
        depth, img, mask = (torch.stack([x[k] for x in f]).contiguous() for k in ('depth', 'img', 'mask'))
        pose = torch.stack([x['pose'] for x in f]).contiguous()
        nb = (ctypes.c_int64 * 3)(n, n, n)
        ws = torch.empty(int(L.lib().rpe_surfel_workspace_bytes_many(3, nb, 8, 12)), dtype=torch.uint8, device=DEV)
        ticks = (ctypes.c_int32 * 3)(*[se.TICK] * 3)
        rows = (ctypes.c_int32 * 3)(0, 1, 2)
        kmat = (ctypes.c_void_p * 3)(*[x['K'].data_ptr() for x in f])
        kinv = (ctypes.c_void_p * 3)(*[x['kinv'].data_ptr() for x in f])
        sd = (L.SurfelMapDesc * 3)(*[m.desc() for m in src])
        dd = (L.SurfelMapDesc * 3)(*[m.desc() for m in dst])
        L.check(L.lib().rpe_surfel_fuse_many(3, sd, nb, dd, ticks, rows, 3, L.ptr(depth), L.ptr(img), L.ptr(mask), 8, 12, kmat, kinv,
                                             L.ptr(pose), 8.0, 1, 1, 7.0, 2, L.ptr(ws), L.stream_ptr()), 'rpe_surfel_fuse_many')
        torch.cuda.synchronize()
        return src, dst

    (s1, d1), (sm, dm) = run(False), run(True)
    assert [d.overflow for d in d1] == [0, 1, 0] and [d.count for d in d1] == [108, 40, 108]
    for k in range(3):
        assert (dm[k].count, dm[k].overflow) == (d1[k].count, d1[k].overflow), k
        assert torch.equal(dm[k].rows(dm[k].count), d1[k].rows(d1[k].count)) and torch.equal(sm[k].rows(n), s1[k].rows(n)), k
        dm[k].assert_guards(dm[k].count)
        sm[k].assert_guards(n)
