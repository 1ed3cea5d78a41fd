"""Surfel-map golden vectors from the reference's own core/fusion/surfel_map.py (runs ONLY where the reference checkout is present,
like oracle/gen_golden.py, whose loaders it imports unchanged).

One stand-in is added on top of ``oracle.gen_golden.load_reference()``: pinhole_transforms.transform_forward applies the SE3 to
homogeneous 4-vectors (reproject() appends w = 1), which lietorch acts on as ``[R p + t w, w]``; oracle.se3's act takes 3-vectors, so
the seeded ``lietorch.SE3.__mul__`` is wrapped to split off w.

Writes tests/golden/surfel_map.npz: a seeded 32x48 scene, SurfelMap(frame=...) then 20 fuses under prescribed poses, for two cases
  a: d_thresh 3.0 (most surfels associate), average_pts True,  t_max 15  -> confidence saturates, stable surfels survive the prune
  b: d_thresh 0.05 (almost none do),       average_pts False, t_max 6   -> the map grows by ~h*w per frame and the prune cuts it
Per step: count, the sha1 of the conf / t_created bytes (order included), f64 moments of opts / rgb; whole arrays at a few steps.
Renders of the final map of each case, with NaN rgb / NaN z / behind-the-camera surfels injected, at 3 extrinsics (render(K, T)) and
through transform_cpy(T).render(K); one save_ply output as bytes.

Writes tests/golden/tracker_f2m.npz: the reference's PoseEstimator(frame2frame=False) (core/pose/pose_estimator.py with its own
surfel_map.py) on oracle.synth.tracker_case with the seeded model oracle.gen_golden.gen_modules uses: per frame the absolute pose,
the success flag, the map count and f64 moments of the map; then the scripted-pose gate case of tracker.npz (a stand-in model hands
back prescribed relative poses) with the map count after every frame, so fuse-only-on-success is pinned.  The reference's render
sorts with an unstable argsort, which leaves the order among equal confidences undefined; the fixture is made with a stable one (one
of the orders the reference allows, and the one rpe.h documents), on one thread (see main()).

Usage:  python tools/gen_surfel_golden.py [tracker]          (from the repo root; ``tracker``: only tracker_f2m.npz)
"""
import hashlib
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 32, 48
STEPS = 20
CASES = {'a': dict(d_thresh=3.0, average_pts=True, t_max=15), 'b': dict(d_thresh=0.05, average_pts=False, t_max=6)}
FULL_STEPS = {'a': (0, 7, STEPS), 'b': (3, STEPS)}


def patch_homogeneous_act():
    from oracle import se3 as ose3
    mul = ose3.SE3.__mul__

    def __mul__(self, other):
        if isinstance(other, torch.Tensor) and other.shape[-1] == 4:
            w = other[..., 3:]
            return torch.cat((ose3.quat_rotate(self.data[..., 3:], other[..., :3]) + self.data[..., :3] * w, w), dim=-1)
        return mul(self, other)
    ose3.SE3.__mul__ = __mul__


def scene():
    """K, per-step frames (rpe_amd.synth.surfel_scene: the tests regenerate them from the seed) and poses (7,) of a slowly moving camera."""
    import rpe_amd  # noqa: F401
    from rpe_amd import synth as psynth
    from oracle import se3 as ose3
    K, frames = psynth.surfel_scene(H, W, STEPS)
    return K, frames, [ose3.SE3.exp(psynth.surfel_pose(k)).data.reshape(7) for k in range(STEPS + 1)]


def sha(t):
    return hashlib.sha1(t.contiguous().numpy().tobytes()).hexdigest()


def mom(t):
    t = t.double()
    t = torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)
    return torch.stack((t.sum(-1), t.abs().sum(-1), (t * t).sum(-1)), dim=-1).numpy()


def render_inputs(m, distinct):
    """The final map with surfels the renderer must handle: NaN rgb (NaN-fill), NaN z and behind-the-camera surfels (never drawn).
    ``distinct``: confidences made pairwise different (few ties, so almost every pixel -- NaN-filled ones included -- is pinned)."""
    opts, rgb, conf = m.opts.clone(), m.rgb.clone(), m.conf.clone()
    n = opts.shape[1]
    if distinct:
        conf = conf + torch.arange(n, dtype=torch.float32)[None] * 1e-5
    idx = torch.arange(5, n, max(n // 40, 1))
    rgb[idx % 3, idx] = float('nan')
    opts[2, idx[::4] + 1] = float('nan')
    opts[2, idx[1::4] + 2] = -opts[2, idx[1::4] + 2]
    conf[0, idx[2::4] + 3] = 0.0                     # drawn, but mask False there
    return opts, rgb, conf


@torch.no_grad()
def main():
    # one thread: the reference's CPU index_put with duplicate indices (render's scatter) splits the writes across threads, so the
    # winner of a pixel several surfels land on changes from run to run; on one thread the writes land in argsort order (the last
    # one, of the largest conf, wins) -- what the renderer is meant to do.  Only the order among equal confs stays undefined (the
    # argsort is not stable): the tests accept any of the tied surfels there.
    torch.set_num_threads(1)
    from oracle.gen_golden import REF, load_reference
    load_reference()
    patch_homogeneous_act()
    sys.path.insert(0, REF)
    import core.fusion.surfel_map as rsm
    from core.utils.frame_class import Frame
    from oracle import se3 as ose3
    K, frames, poses = scene()
    out = {'K': K.numpy(), 'poses': torch.stack(poses).numpy(),
           'frames_mom': np.stack([np.concatenate([mom(t.reshape(1, -1).float())[0] for t in f]) for f in frames])}
    for c, kw in CASES.items():
        img, depth, mask, conf = frames[0]
        f0 = Frame(img.clone(), img.clone(), depth=depth.clone(), mask=mask.clone(), confidence=conf.clone())
        m = rsm.SurfelMap(frame=f0, kmat=K.clone(), pmat=ose3.SE3(poses[0][None].clone()), upscale=1, **kw)
        counts, shas, moms = [], [], []
        for s in range(STEPS + 1):
            if s > 0:
                img, depth, mask, conf = frames[s]
                m.fuse(Frame(img.clone(), img.clone(), depth=depth.clone(), mask=mask.clone()), ose3.SE3(poses[s][None].clone()))
            counts.append(m.opts.shape[1])
            shas.append(sha(m.conf) + sha(m.t_created))
            moms.append(np.concatenate((mom(m.opts), mom(m.rgb))))
            if s in FULL_STEPS[c]:
                out[f'{c}_opts{s}'], out[f'{c}_rgb{s}'] = m.opts.numpy().copy(), m.rgb.numpy().copy()
                out[f'{c}_conf{s}'], out[f'{c}_t{s}'] = m.conf.numpy().copy(), m.t_created.numpy().copy()
            print(c, s, counts[-1], int((m.conf >= 1).sum()))
        out[f'{c}_count'], out[f'{c}_sha'], out[f'{c}_mom'] = np.array(counts), np.array(shas), np.stack(moms)
        # renders of the final map (plus injected surfels) at three extrinsics, and the tracker's transform_cpy + render pair
        opts, rgb, cf = render_inputs(m, distinct=c == 'b')
        out[f'{c}_r_opts'], out[f'{c}_r_rgb'], out[f'{c}_r_conf'] = opts.numpy(), rgb.numpy(), cf.numpy()
        rm = rsm.SurfelMap(opts=opts.clone(), rgb=rgb.clone(), conf=cf.clone(), kmat=K.clone(), img_shape=(H, W))
        Ts = [poses[STEPS], ose3.SE3(poses[STEPS][None]).inv().data.reshape(7), torch.tensor([2.0, -1.0, -62.0, 0.0, 0.0, 0.0, 1.0])]
        for j, T in enumerate(Ts):
            fr, _ = rm.render(K.clone(), ose3.SE3(T[None].clone()))
            out[f'{c}_T{j}'] = T.numpy()
            out[f'{c}_img{j}'], out[f'{c}_depth{j}'] = fr.img.numpy(), fr.depth.numpy()
            out[f'{c}_rconf{j}'], out[f'{c}_rmask{j}'] = fr.confidence.numpy(), fr.mask.numpy()
        fr, _ = rm.transform_cpy(ose3.SE3(Ts[1][None].clone())).render(K.clone())
        out[f'{c}_img_cpy'], out[f'{c}_depth_cpy'] = fr.img.numpy(), fr.depth.numpy()
        out[f'{c}_rconf_cpy'], out[f'{c}_rmask_cpy'] = fr.confidence.numpy(), fr.mask.numpy()
        if c == 'a':
            with tempfile.TemporaryDirectory() as td:
                p = os.path.join(td, 'map.ply')
                m.save_ply(p, stable=True)
                out['ply_stable'] = np.frombuffer(open(p, 'rb').read(), dtype=np.uint8)
                m.save_ply(p, stable=False)
                out['ply_all'] = np.frombuffer(open(p, 'rb').read(), dtype=np.uint8)
    path = os.path.join(ROOT, 'tests', 'golden', 'surfel_map.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


@torch.no_grad()
def gen_tracker():
    import tempfile
    import warnings
    torch.set_num_threads(1)
    from oracle.gen_golden import REF, load_reference, load_reference_modules
    from oracle import pose_net as opn, se3 as ose3, synth
    import rpe_amd  # noqa: F401
    from rpe_amd import synth as psynth
    load_reference()
    patch_homogeneous_act()
    sys.path.insert(0, REF)
    M = load_reference_modules()
    import core.fusion.surfel_map as rsm
    argsort = torch.argsort
    rsm.torch = type(sys)('torch_stable_argsort')                  # the module's `torch` with a stable argsort, nothing else changed
    rsm.torch.__dict__.update({k: getattr(torch, k) for k in dir(torch) if not k.startswith('__')})
    rsm.torch.argsort = lambda x, dim=-1, **kw: argsort(x, dim=dim, stable=True)
    Hm, Wm = synth.MODULE_HW
    cfg, sd, _ = synth.posenet_case(psynth, opn)
    frames, K, bf = synth.tracker_case(psynth, n_frames=4)
    slam = dict(frame2frame=False, dist_thr=0.05, depth_clipping=[1, 250], debug=False, conf_weighing=True, average_pts=True,
                lbgfs_iters=8)
    with tempfile.TemporaryDirectory() as td:
        ck = os.path.join(td, 'ck.pth')
        torch.save({'config': {'model': dict(cfg)}, 'state_dict': {'module.' + k: v for k, v in sd.items()}}, ck)
        est = M['pose_estimator'].PoseEstimator(slam, K, bf, ck, (Wm, Hm))
    out = {'frames_mom': np.stack([mom(torch.cat((l, r)).reshape(1, -1))[0] for l, r, _ in frames])}
    poses, ok, counts, moms = [], [], [], []
    for l, r, m in frames:
        with warnings.catch_warnings(record=True) as wl:
            warnings.simplefilter('always')
            P, scene, flow, weights = est(l.clone(), r.clone(), m.clone())
        poses.append(P.data.reshape(7).clone())
        ok.append(not any('not converged' in str(w.message) for w in wl))
        counts.append(scene.opts.shape[1])
        moms.append(np.concatenate((mom(scene.opts), mom(scene.rgb), mom(scene.conf))))
        print('f2m frame', len(poses), counts[-1], ok[-1], poses[-1].tolist())
    out.update(abs_poses=torch.stack(poses).numpy(), success=np.array(ok), count=np.array(counts), map_mom=np.stack(moms))

    rel = synth.gate_case()

    class Scripted(torch.nn.Module):
        """Stands in for PoseNet: depth 0.25 (62.5 mm after de-normalisation), prescribed relative poses."""
        def __init__(self):
            super().__init__()
            self.i = 0

        def flow2depth(self, l, r, baseline):
            return torch.full_like(l[:, :1], 0.25), torch.zeros_like(l[:, :2]), torch.ones_like(l[:, :1], dtype=torch.bool)

        def infer(self, *args, **kw):
            p = ose3.SE3(rel[self.i:self.i + 1].clone())[0]
            self.i += 1
            d = torch.full_like(args[0][:, :1], 0.25)
            return p, d, d, (d, d), torch.zeros_like(args[0][:, :2]), torch.zeros_like(args[0][:, :2])

    est.model = Scripted()
    est.frame = est.last_frame = est.scene = None
    est.last_pose = ose3.SE3.Identity(1)
    g = torch.Generator().manual_seed(21)
    tiny = torch.rand(1, 3, 8, 8, generator=g) * 255
    chain, gok, gcount = [], [], []
    for i in range(rel.shape[0]):
        with warnings.catch_warnings(record=True) as wl:
            warnings.simplefilter('always')
            P, scene, *_ = est(tiny.clone(), tiny.clone(), torch.ones(1, 1, 8, 8, dtype=torch.bool))
        chain.append(P.data.reshape(7).clone())
        gok.append(not any('not converged' in str(w.message) for w in wl))
        gcount.append(scene.opts.shape[1])
    out.update(gate_rel=rel.numpy(), gate_abs=torch.stack(chain).numpy(), gate_success=np.array(gok), gate_count=np.array(gcount),
               gate_tiny=tiny.numpy())
    print('gate', gok, gcount)
    path = os.path.join(ROOT, 'tests', 'golden', 'tracker_f2m.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'tracker':
        gen_tracker()
    else:
        main()
        gen_tracker()
