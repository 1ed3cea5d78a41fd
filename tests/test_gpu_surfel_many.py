"""GPU: the batched surfel-map calls (surfel_map.init_many / render_many / fuse_many on rpe_surfel_*_many) against the single-map
methods they stand for, bit for bit: renders of K maps of different sizes (one empty) with per-map K and T at 640x512 and of the golden
render scenes (ties included); ten fuse steps over a changing subset of maps with different ticks, capacity growth and an empty map;
run-to-run determinism."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
OPTS = dict(d_thresh=0.5, average_pts=True, t_max=6)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t.view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _frame(img, depth, mask, conf=None):
    from rpe_amd.pose_estimator import Frame
    return Frame(img.to(DEV), depth=depth.to(DEV), mask=mask.to(DEV), confidence=None if conf is None else conf.to(DEV))


def _pose(k, scale):
    from rpe_amd import synth
    from rpe_amd.se3 import SE3
    return SE3.exp(synth.surfel_pose(k, scale).to(DEV))


def _state(m):
    return (m.n, m.overflowed, m.tick, m.capacity, torch.cat((m.opts, m.rgb, m.conf, m.t_created)).cpu())


def _check_render(maps, Ks, Ts, depth_transformed=True):
    from rpe_amd import surfel_map
    fr = surfel_map.render_many(maps, Ks, Ts.data, depth_transformed=depth_transformed)
    for k, m in enumerate(maps):
        one = (m.render_transformed if depth_transformed else m.render)(Ks[k], Ts[k:k + 1])[0]
        for name in ('img', 'depth', 'confidence', 'mask'):
            assert _same(getattr(fr, name)[k:k + 1], getattr(one, name)), (k, name)
    return fr


def _maps_640(seed_base=0):
    """Three 640x512 maps: more than a frame of surfels after three fuses, one frame's worth, and an empty one."""
    from rpe_amd import synth
    from rpe_amd.surfel_map import SurfelMap
    H, W = 512, 640
    maps = []
    for k, steps in enumerate((3, 0)):
        K, frames = synth.surfel_scene(H, W, steps, seed=21 + k + seed_base)
        img, depth, mask, conf = frames[0]
        m = SurfelMap(frame=_frame(img, depth, mask, conf), kmat=K.to(DEV), pmat=_pose(0, 1.0), upscale=1, **OPTS)
        for s in range(1, steps + 1):
            m.fuse(_frame(*frames[s][:3]), _pose(s, 1.0))
        maps.append(m)
    empty = SurfelMap(opts=torch.zeros(3, 0, device=DEV), rgb=torch.zeros(3, 0, device=DEV), conf=torch.zeros(1, 0, device=DEV),
                      kmat=K.to(DEV), img_shape=(H, W))
    return maps[0], empty, maps[1], K


def test_render_many_matches_single_renders_640x512(rpe):
    from rpe_amd.se3 import SE3
    big, empty, small, K = _maps_640()
    assert big.n > 512 * 640 >= small.n > 0 and empty.n == 0
    maps = [big, empty, small]
    Ks = torch.stack([K, K * torch.tensor([[1.02], [0.98], [1.0]]), K]).to(DEV)
    Ts = SE3(torch.cat([_pose(s, 1.0).inv().data for s in (3, 1, 0)]))
    for dt in (True, False):
        fr = _check_render(maps, Ks, Ts, depth_transformed=dt)
        assert int(fr.mask[0].sum()) > 0.5 * 512 * 640 and int(fr.mask[1].sum()) == 0
    # two identical runs, into caller-given output rows
    from rpe_amd import surfel_map
    out = tuple(torch.full_like(t, 7) for t in (fr.img, fr.depth, fr.confidence)) + (torch.zeros_like(fr.mask),)
    again = surfel_map.render_many(maps, Ks, Ts, out=out, depth_transformed=False)
    assert again.img is out[0] and all(_same(getattr(again, n), getattr(fr, n)) for n in ('img', 'depth', 'confidence', 'mask'))


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(GOLDEN, 'surfel_map.npz')))


def test_render_many_matches_single_renders_on_golden_scenes(rpe, gold):
    """The golden render scenes (cases a and b: many ties) as two maps of one call, under each of the golden extrinsics."""
    from rpe_amd.se3 import SE3
    from rpe_amd.surfel_map import SurfelMap
    K = torch.from_numpy(gold['K']).to(DEV)
    maps = [SurfelMap(opts=torch.from_numpy(gold[f'{c}_r_opts']).to(DEV), rgb=torch.from_numpy(gold[f'{c}_r_rgb']).to(DEV),
                      conf=torch.from_numpy(gold[f'{c}_r_conf']).to(DEV), kmat=K, img_shape=(32, 48)) for c in ('a', 'b')]
    for key in (0, 1, 2):
        Ts = SE3(torch.cat([torch.from_numpy(gold[f'{c}_T{key}']).reshape(1, 7) for c in ('a', 'b')]).to(DEV))
        for dt in (True, False):
            _check_render(maps, torch.stack([K, K]), Ts, depth_transformed=dt)


def _fuse_run(batched):
    """Three maps of 96x128 scenes over ten fuse steps; map k fuses at step s unless (s + k) % 3 == 0, so the subset and the ticks
    change.  Map 2's first frame has no valid pixel (n = 0).  Every map starts at capacity h*w and grows.  Returns the per-step states."""
    from rpe_amd import surfel_map, synth
    from rpe_amd.pose_estimator import Frame
    from rpe_amd.se3 import SE3
    from rpe_amd.surfel_map import SurfelMap
    H, W, n = 96, 128, 3
    scenes = [synth.surfel_scene(H, W, 10, seed=40 + k) for k in range(n)]
    Ks = [scenes[k][0] * torch.tensor([[1.0 + 0.03 * k], [1.0 - 0.02 * k], [1.0]]) for k in range(n)]
    first = [list(scenes[k][1][0]) for k in range(n)]
    first[2][2] = torch.zeros_like(first[2][2])
    if batched:
        f0 = Frame(torch.cat([f[0] for f in first]).to(DEV), depth=torch.cat([f[1] for f in first]).to(DEV),
                   mask=torch.cat([f[2] for f in first]).to(DEV), confidence=torch.cat([f[3] for f in first]).to(DEV))
        maps = surfel_map.init_many(f0, torch.stack(Ks).to(DEV), torch.cat([_pose(0, 0.5 + k).data for k in range(n)]), upscale=1, **OPTS)
    else:
        maps = [SurfelMap(frame=_frame(*first[k]), kmat=Ks[k].to(DEV), pmat=_pose(0, 0.5 + k), upscale=1, **OPTS) for k in range(n)]
    states = [[_state(m) for m in maps]]
    for s in range(1, 11):
        rows = [k for k in range(n) if (s + k) % 3 != 0]
        poses = [_pose(s, 0.5 + k) for k in range(n)]
        if batched:
            fr = Frame(torch.cat([scenes[k][1][s][0] for k in range(n)]).to(DEV), depth=torch.cat([scenes[k][1][s][1] for k in range(n)]).to(DEV),
                       mask=torch.cat([scenes[k][1][s][2] for k in range(n)]).to(DEV))
            surfel_map.fuse_many([maps[k] for k in rows], fr, SE3(torch.cat([p.data for p in poses])), rows=rows)
        else:
            for k in rows:
                maps[k].fuse(_frame(*scenes[k][1][s][:3]), poses[k])
        states.append([_state(m) for m in maps])
    return states


def test_fuse_many_matches_single_fuses_over_ten_steps(rpe):
    single, batched, again = _fuse_run(False), _fuse_run(True), _fuse_run(True)
    assert single[0][2][0] == 0                                            # the empty map
    assert [single[-1][k][2] for k in range(3)] == [7, 7, 6]              # the maps' ticks differ
    grew = [any(single[s][k][3] > single[s - 1][k][3] for s in range(1, 11)) for k in range(3)]
    assert any(grew)                                                       # a map grows its capacity mid-run
    for s in range(11):
        for k in range(3):
            a, b, c = single[s][k], batched[s][k], again[s][k]
            assert a[:4] == b[:4] == c[:4], (s, k, a[:4], b[:4], c[:4])
            assert a[1] == 0
            assert _same(a[4], b[4]) and _same(b[4], c[4]), (s, k)
