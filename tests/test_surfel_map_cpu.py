"""CPU: the surfel-map ABI (declared, bound, exported, argument checks without a GPU), the plain-torch restatement of the reference's
SurfelMap against tests/golden/surfel_map.npz (made by tools/gen_surfel_golden.py from the reference's own surfel_map.py), the product's
PLY writer against the reference's bytes, and the frame-to-model tracker's construction and refusals."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import surfel_ref as sr

SURFEL_ENTRIES = ('rpe_surfel_workspace_bytes', 'rpe_surfel_init', 'rpe_surfel_fuse', 'rpe_surfel_prune', 'rpe_surfel_render',
                  'rpe_surfel_transform')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(GOLDEN, 'surfel_map.npz')))


def _scene(g):
    from rpe_amd import synth
    H, W = 32, 48
    K, frames = synth.surfel_scene(H, W, 20)
    mom = np.stack([np.concatenate([[t.double().sum(), t.double().abs().sum(), (t.double() ** 2).sum()] for t in f]) for f in frames])
    np.testing.assert_allclose(mom, g['frames_mom'], rtol=1e-12)                 # the seeded frames are the ones the golden saw
    assert torch.equal(K, torch.from_numpy(g['K']))
    return K, frames, torch.from_numpy(g['poses'])


def test_surfel_abi_declared_bound_exported(rpe):
    from rpe_amd import _lib
    L = rpe.lib()
    for name in SURFEL_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.rpe_abi_minor() >= 3 and _lib.ABI_MINOR == 3
    assert ctypes.sizeof(_lib.SurfelMapDesc) == 56


def test_surfel_bad_arguments_return_badarg_without_a_gpu(rpe):
    from rpe_amd import _lib
    L = rpe.lib()
    assert L.rpe_surfel_workspace_bytes(-1, 4, 4) == 0 and L.rpe_surfel_workspace_bytes(0, 0, 4) == 0
    assert L.rpe_surfel_workspace_bytes(1000, 512, 640) >= 512 * 640 * 8
    fake = ctypes.c_void_p(0x1000)                      # never dereferenced: every call below fails its argument check first
    good = _lib.SurfelMapDesc(fake, fake, fake, fake, 16, fake, fake)
    nullmap = _lib.SurfelMapDesc(None, fake, fake, fake, 16, fake, fake)
    zero_cap = _lib.SurfelMapDesc(fake, fake, fake, fake, 0, fake, fake)
    other = _lib.SurfelMapDesc(ctypes.c_void_p(0x2000), fake, fake, fake, 16, ctypes.c_void_p(0x3000), fake)
    B = -1
    assert L.rpe_surfel_init(None, fake, fake, fake, 4, 4, fake, fake, 7.0, good, fake, None) == B
    assert L.rpe_surfel_init(fake, fake, fake, fake, 0, 4, fake, fake, 7.0, good, fake, None) == B
    assert L.rpe_surfel_init(fake, fake, fake, fake, 4, 4, fake, fake, 7.0, nullmap, fake, None) == B
    assert L.rpe_surfel_init(fake, fake, fake, fake, 4, 4, fake, fake, 7.0, zero_cap, fake, None) == B
    args = (fake, fake, fake, 4, 4, fake, fake, fake, 0.05, 1, 1, 7.0, 0, 15)
    assert L.rpe_surfel_fuse(good, 0, *args, good, fake, None) == B                     # src == dst
    assert L.rpe_surfel_fuse(nullmap, 0, *args, other, fake, None) == B
    assert L.rpe_surfel_fuse(good, 17, *args, other, fake, None) == B                   # bound past the capacity
    assert L.rpe_surfel_fuse(good, 0, None, *args[1:], other, fake, None) == B
    up2 = args[:10] + (2,) + args[11:]
    assert L.rpe_surfel_fuse(good, 0, *up2, other, fake, None) == -3                    # RPE_E_UNSUPPORTED: upscale > 1
    assert L.rpe_surfel_prune(good, 0, 1, 15, good, fake, None) == B
    assert L.rpe_surfel_prune(good, -1, 1, 15, other, fake, None) == B
    assert L.rpe_surfel_render(good, 0, fake, fake, 1, 2, 4, fake, fake, fake, fake, fake, None) == B    # h < 3 (reflect padding)
    assert L.rpe_surfel_render(nullmap, 0, fake, fake, 1, 4, 4, fake, fake, fake, fake, fake, None) == B
    assert L.rpe_surfel_render(good, 0, None, fake, 1, 4, 4, fake, fake, fake, fake, fake, None) == B
    assert L.rpe_surfel_transform(None, 16, fake, 16, fake, 4, fake, None) == B
    assert L.rpe_surfel_transform(fake, 16, fake, 8, fake, 12, fake, None) == B


def _sha(t):
    return hashlib.sha1(t.contiguous().numpy().tobytes()).hexdigest()


def _mom(t):
    t = torch.nan_to_num(t.double(), nan=0.0, posinf=0.0, neginf=0.0)
    return torch.stack((t.sum(-1), t.abs().sum(-1), (t * t).sum(-1)), dim=-1).numpy()


CASES = {'a': dict(d_thresh=3.0, average_pts=True, t_max=15), 'b': dict(d_thresh=0.05, average_pts=False, t_max=6)}


@pytest.mark.parametrize('case', ['a', 'b'])
def test_restatement_reproduces_reference_map(rpe, gold, case):
    K, frames, poses = _scene(gold)
    img, depth, mask, conf = frames[0]
    m = sr.RefMap(K, img, depth, mask, conf, poses[0], **CASES[case])
    for s in range(21):
        if s:
            img, depth, mask, _ = frames[s]
            m.fuse(img, depth, mask, poses[s])
        assert m.opts.shape[1] == gold[f'{case}_count'][s], s
        assert _sha(m.conf) + _sha(m.t_created) == gold[f'{case}_sha'][s], s          # conf, t_created and order, bit for bit
        np.testing.assert_allclose(np.concatenate((_mom(m.opts), _mom(m.rgb))), gold[f'{case}_mom'][s], rtol=1e-6)
        if f'{case}_opts{s}' in gold:
            np.testing.assert_allclose(m.opts.numpy(), gold[f'{case}_opts{s}'], rtol=1e-6, atol=1e-6 * 60)
            np.testing.assert_allclose(m.rgb.numpy(), gold[f'{case}_rgb{s}'], rtol=1e-6, atol=1e-6 * 255)


def _check_render(got, g, key, tied, winner, opts, rgb, conf, depth_from):
    """got = (img, depth, confidence, mask) of a renderer, golden planes under ``key``: equal everywhere, except where the golden pixel
    had a tied maximum: there the golden value must be one of the tied surfels' (the reference's argsort is not stable)."""
    img, depth, confidence, mask = got
    gi, gd = g[f'img{key}'][0], g[f'depth{key}'][0, 0]
    gc, gm = g[f'rconf{key}'][0, 0], g[f'rmask{key}'][0, 0]
    h, w = gd.shape
    free = ~tied.reshape(h, w).numpy()
    np.testing.assert_array_equal(confidence.numpy(), gc)                              # ties share the conf value
    np.testing.assert_array_equal(mask.numpy(), gm)
    nanfill = np.isnan(rgb[:, winner.clamp(min=0)].numpy()).reshape(3, h, w) & (winner >= 0).reshape(1, h, w).numpy()
    exact = free[None] & ~nanfill
    np.testing.assert_array_equal(img.numpy()[exact], gi[exact])
    # a NaN-filled pixel reads its 5x5 neighbourhood: compare it where no neighbour was a tie either
    calm = ~torch.nn.functional.max_pool2d(torch.from_numpy(~free)[None, None].float(), 5, 1, 2)[0, 0].bool().numpy()
    fill = nanfill & calm[None]
    np.testing.assert_allclose(img.numpy()[fill], gi[fill], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(depth.numpy()[free], gd[free], rtol=1e-6)
    for p in np.flatnonzero(~free):                                                    # the golden pixel is some tied surfel
        y, x = divmod(int(p), w)
        cands = torch.nonzero(conf[0] == confidence.reshape(-1)[p]).reshape(-1)
        for c in range(3):                # a tied surfel's colour, or a fill value where a tied surfel's colour is NaN
            vals = rgb[c, cands]
            assert (vals == float(gi[c, y, x])).any() or torch.isnan(vals).any(), (key, p, c)
    return int((~free).sum()), int(fill.sum())


@pytest.mark.parametrize('case', ['a', 'b'])
def test_restatement_reproduces_reference_renders(rpe, gold, case):
    g = {k[2:]: v for k, v in gold.items() if k.startswith(case + '_')}
    K = torch.from_numpy(gold['K'])
    opts, rgb, conf = (torch.from_numpy(g[k]) for k in ('r_opts', 'r_rgb', 'r_conf'))
    ties = fills = 0
    for key, T, tr in ((0, g['T0'], False), (1, g['T1'], False), (2, g['T2'], False), ('_cpy', g['T1'], True)):
        img, depth, confidence, mask, winner, tied = sr.render(opts, rgb, conf, K, torch.from_numpy(T), (32, 48), tr)
        t, f = _check_render((img, depth, confidence, mask), g, key, tied, winner, opts, rgb, conf, tr)
        ties, fills = ties + t, fills + f
    print(f'case {case}: {ties} tied pixels, {fills} NaN-filled values compared')
    assert fills > 0 or case == 'a'              # (case a: most surfels saturate at conf 1, so nearly every pixel is a tie)


def test_restatement_dtype_float32_is_todays_and_float64_agrees(rpe, gold):
    """The restatement's dtype argument: float32 given explicitly reproduces the golden hashes bit for bit (as the default does
    above); float64 runs the same operations and lands within float32 rounding of it where no decision is involved (the init)."""
    K, frames, poses = _scene(gold)
    img, depth, mask, conf = frames[0]
    m = sr.RefMap(K, img, depth, mask, conf, poses[0], dtype=torch.float32, **CASES['b'])
    d = sr.RefMap(K, img, depth, mask, conf, poses[0], dtype=torch.float64, **CASES['b'])
    assert d.opts.dtype == torch.float64 and torch.allclose(d.opts, m.opts.double(), rtol=1e-5, atol=1e-4)
    for s in range(1, 21):
        img, depth, mask, _ = frames[s]
        m.fuse(img, depth, mask, poses[s])
        assert m.opts.dtype == torch.float32 and _sha(m.conf) + _sha(m.t_created) == gold[f'b_sha'][s], s
    g = {k[2:]: v for k, v in gold.items() if k.startswith('b_')}
    opts, rgb, conf = (torch.from_numpy(g[k]) for k in ('r_opts', 'r_rgb', 'r_conf'))
    T = torch.from_numpy(g['T1'])
    a = sr.render(opts, rgb, conf, K, T, (32, 48), True)
    b = sr.render(opts, rgb, conf, K, T, (32, 48), True, dtype=torch.float32)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(torch.nan_to_num(x.double()), torch.nan_to_num(y.double()))
    c = sr.render(opts, rgb, conf, K, T, (32, 48), True, dtype=torch.float64)
    assert c[0].dtype == torch.float64 and torch.equal(c[2].float(), a[2])       # the winners' conf: copied, so equal


@pytest.mark.parametrize('pose', ['identity', 'shift', 'turn'])
def test_exact_scenes_decide_alike_in_float32_and_float64(rpe, pose):
    """The precondition of tests/test_gpu_surfel_edges.py, also where there is no GPU: on the exact scenes the float32 and float64
    restatements take the same decisions, and those are the ones each scene was built to provoke."""
    import surfel_edges as se
    s = se.fuse_scene(pose)
    for case in se.FUSE_CASES:
        _, t = se.check_exact_fuse(s, *case)
        assert torch.equal(t['flags'], s['expect']), [n for n, f, e in zip(s['names'], t['flags'], s['expect']) if f != e]
        assert int(t['new'].sum()) == 77                          # 96 pixels - 1 masked - 18 matched
        if case[1] < 2 and case[2] == 7:
            assert t['n'] == 2                                    # t_max 0 / 1: the appended surfels go again; 'stable' and 'clamp' stay
    if pose == 'identity':
        _, t = se.check_exact_fuse(se.negzero_scene(), True, 2, 7)
        assert bool(t['flags'].all()) and not bool(t['new'].reshape(8, 12)[2, 0]) and not bool(t['new'].reshape(8, 12)[6, 0])
        for h, w, n, mask in ((8, 12, 0, True), (8, 12, 3, False), (1, 1, 2, True), (8, 1, 2, True)):
            _, t = se.check_exact_fuse(se.small_scene(h, w, n, mask), True, 2, 7)
            assert not bool(t['flags'].any()) and t['n'] == n + (h * w if mask else 0)
    for h, w in se.RENDER_SHAPES:
        for nan_plane in (False, True):
            for dt in (False, True):
                a, b = se.check_exact_render(se.render_scene(h, w, pose, nan_plane), dt)
                assert not bool(torch.isnan(b['img']).any())
    if pose == 'identity':
        for axis, pix in (('u', (2, 0)), ('v', (0, 4))):          # a -0.0 coordinate is inside, and its surfel wins column / row 0
            for dt in (False, True):
                _, t = se.check_exact_render(se.render_negzero_scene(axis), dt)
                assert int(t['winner'][pix[0] * 12 + pix[1]]) == 1 and float(t['confidence'][pix]) == .5
    _, t = se.check_exact_render(se.zero_conf_scene(), False)
    assert int(t['mask'].sum()) == 1 and float(t['confidence'][1, 5]) == -float('inf')       # zero-conf winners: mask 0; -inf: mask 1


def test_prune_rows_are_what_the_patterns_say(rpe):
    import surfel_edges as se
    for n in se.PRUNE_SIZES[:10]:
        for pat in se.PRUNE_PATTERNS:
            rows, keep = se.prune_rows(n, pat)
            assert rows.shape == (8, n) and keep.shape == (n,)
            if pat == 'tiles' and n > 1024:
                assert not bool(keep[:1024].any()) and bool(keep[1024:min(n, 2048)].all())
    rows, keep = se.prune_edge_rows()
    assert torch.equal(se.prune_keep(rows[6].view(torch.float32), rows[7].view(torch.float32), 20, 6), keep)


def test_render_refuses_two_pixel_axes_without_a_gpu(rpe):
    from rpe_amd import _lib
    L = rpe.lib()
    fake = ctypes.c_void_p(0x1000)
    good = _lib.SurfelMapDesc(fake, fake, fake, fake, 16, fake, fake)
    for h, w in ((2, 4), (4, 2), (2, 2)):
        assert L.rpe_surfel_render(good, 0, fake, fake, 1, h, w, fake, fake, fake, fake, fake, None) == -1
    assert L.rpe_surfel_render(good, 17, fake, fake, 1, 4, 4, fake, fake, fake, fake, fake, None) == -1      # bound past the capacity
    descs = (_lib.SurfelMapDesc * 65)(*[good] * 65)
    nb = (ctypes.c_int64 * 65)(*[0] * 65)
    assert L.rpe_surfel_render_many(65, descs, nb, fake, fake, 1, 4, 4, fake, fake, fake, fake, fake, None) == -1   # K = 65
    assert L.rpe_surfel_workspace_bytes_many(65, nb, 4, 4) == 0 and L.rpe_surfel_workspace_bytes_many(64, nb, 4, 4) > 0


def test_ply_writer_reproduces_reference_bytes(rpe, gold, tmp_path):
    from rpe_amd.surfel_map import SurfelMap
    m = SurfelMap(opts=torch.from_numpy(gold['a_opts20']), rgb=torch.from_numpy(gold['a_rgb20']), conf=torch.from_numpy(gold['a_conf20']),
                  kmat=torch.from_numpy(gold['K']), img_shape=(32, 48))
    for stable, key in ((True, 'ply_stable'), (False, 'ply_all')):
        p = tmp_path / f'{key}.ply'
        m.save_ply(str(p), stable=stable)
        assert p.read_bytes() == gold[key].tobytes(), key


def test_surfel_map_refusals(rpe):
    from rpe_amd.surfel_map import SurfelMap
    K = torch.eye(3)
    with pytest.raises(NotImplementedError):
        SurfelMap(opts=torch.ones(3, 4), rgb=torch.ones(3, 4), kmat=K, upscale=2)
    m = SurfelMap(opts=torch.ones(3, 4), rgb=torch.ones(3, 4), kmat=K)
    with pytest.raises(NotImplementedError):
        m.pcl2open3d()
    assert m.n == 4 and tuple(m.conf.shape) == (1, 4) and m.tick == 0           # the reference's conf prior for the opts= form
    assert torch.equal(m.t_created, torch.zeros(1, 4))
