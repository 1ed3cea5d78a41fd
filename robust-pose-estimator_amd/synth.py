"""Seeded synthetic stereo inputs and weights for tests and bench.py: there is no
network for datasets or checkpoints and the reference's trained weights are stripped blobs
(.MISSING_LARGE_BLOBS), so the benchmark runs random-init weights of the reference architecture on rendered
stereo pairs.  numpy ``default_rng`` seeds; everything is built on the CPU and moved by the caller."""
import numpy as np
import torch
import torch.nn.functional as F


def intrinsics(h, w):
    return torch.tensor([[1.1 * w, 0.0, w / 2.0], [0.0, 1.1 * w, h / 2.0], [0.0, 0.0, 1.0]], dtype=torch.float32)


def _smooth(rng, c, h, w, cells):
    coarse = torch.from_numpy(rng.uniform(0.0, 1.0, size=(1, c, cells, cells + 2)).astype(np.float32))
    return F.interpolate(coarse, size=(h, w), mode='bicubic', align_corners=True)[0].clamp(0, 1)


def _warp(img, dx, dy):
    n, _, h, w = img.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    gx = 2 * (xs[None] + dx) / (w - 1) - 1
    gy = 2 * (ys[None] + dy) / (h - 1) - 1
    return F.grid_sample(img, torch.stack((gx, gy), dim=-1), align_corners=True, padding_mode='border')


def stereo_frames(seed, n, h, w, bf=7.2):
    """n independent frame pairs.  Returns dict of CPU tensors with the arguments of PoseNet.infer:
    image1l, image2l, image2r (n,3,h,w) 0..255; K (n,3,3); baseline (n,) normalised (bf/250);
    depth1 (n,1,h,w) in (0,1]; mask1, mask2 (n,1,h,w) bool; stereo_flow1 (n,2,h,w); xi_gt (n,6)."""
    rng = np.random.default_rng(seed)
    K = intrinsics(h, w)
    out = {k: [] for k in ('image1l', 'image2l', 'image2r', 'depth1', 'mask1', 'mask2', 'stereo_flow1', 'xi_gt')}
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5, indexing='ij')
    for _ in range(n):
        depth = 0.2 + 0.7 * _smooth(rng, 1, h, w, 5)[0]                                   # normalised units
        tex = 255.0 * (0.6 * _smooth(rng, 3, h, w, 24) + 0.4 * _smooth(rng, 3, h, w, 96))  # band-limited RGB
        xi = np.concatenate((rng.normal(0, 0.005, 3), rng.normal(0, 0.01, 3))).astype(np.float32)
        # small-motion flow of a rigid scene: X' = X + phi x X + tau
        X = torch.stack(((xs - K[0, 2]) / K[0, 0] * depth, (ys - K[1, 2]) / K[1, 1] * depth, depth))
        tau, phi = torch.from_numpy(xi[:3]), torch.from_numpy(xi[3:])
        Xp = X + torch.cross(phi[:, None, None].expand_as(X), X, dim=0) + tau[:, None, None]
        u = K[0, 0] * Xp[0] / Xp[2] + K[0, 2]
        v = K[1, 1] * Xp[1] / Xp[2] + K[1, 2]
        fx, fy = u - xs, v - ys
        disp = bf / depth
        img1 = tex[None]
        img2 = _warp(img1, -fx[None], -fy[None])
        img2r = _warp(img2, disp[None], torch.zeros_like(disp)[None])
        m1 = torch.ones(1, h, w, dtype=torch.bool)
        m2 = torch.ones(1, h, w, dtype=torch.bool)
        y0, x0 = int(rng.integers(0, h - h // 5)), int(rng.integers(0, w - w // 4))
        m1[:, y0:y0 + h // 5, x0:x0 + w // 4] = False                                     # 5 % rectangle cut out
        y0, x0 = int(rng.integers(0, h - h // 5)), int(rng.integers(0, w - w // 4))
        m2[:, y0:y0 + h // 5, x0:x0 + w // 4] = False
        out['image1l'].append(img1[0]); out['image2l'].append(img2[0]); out['image2r'].append(img2r[0])
        out['depth1'].append(depth[None]); out['mask1'].append(m1); out['mask2'].append(m2)
        out['stereo_flow1'].append(torch.stack((-disp, torch.zeros_like(disp))))
        out['xi_gt'].append(torch.from_numpy(xi))
    res = {k: torch.stack(v).contiguous() for k, v in out.items()}
    res['K'] = K[None].repeat(n, 1, 1)
    res['baseline'] = torch.full((n,), bf, dtype=torch.float32)
    return res


def ground_truth_flows(seed, n, h, w, bf=7.2, occluders=3):
    """What a TRAINED flow network converges to on a scene with depth edges (the lookup's realistic-coordinates roofline line in
    bench.py): a smooth background at normalised depth 0.45..0.9 with ``occluders`` foreground ellipses at depth 0.12..0.3, so
    the stereo disparities span 8..60 px with discontinuities, and the rigid temporal flow of a gate-sized camera motion
    (same distribution as stereo_frames).  Returns (time_flow, stereo_flow), each (n,2,h,w) f32 in pixels."""
    rng = np.random.default_rng(seed)
    K = intrinsics(h, w)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5, indexing='ij')
    tf, sf = [], []
    for _ in range(n):
        depth = 0.45 + 0.45 * _smooth(rng, 1, h, w, 5)[0]
        for _ in range(occluders):
            cx, cy = rng.uniform(0.15, 0.85) * w, rng.uniform(0.15, 0.85) * h
            ax, ay = rng.uniform(0.05, 0.2) * w, rng.uniform(0.05, 0.25) * h
            inside = ((xs - cx) / ax) ** 2 + ((ys - cy) / ay) ** 2 < 1.0
            depth = torch.where(inside, torch.full_like(depth, float(rng.uniform(0.12, 0.3))) + 0.02 * (xs - cx) / ax, depth)
        xi = np.concatenate((rng.normal(0, 0.005, 3), rng.normal(0, 0.01, 3))).astype(np.float32)
        X = torch.stack(((xs - K[0, 2]) / K[0, 0] * depth, (ys - K[1, 2]) / K[1, 1] * depth, depth))
        tau, phi = torch.from_numpy(xi[:3]), torch.from_numpy(xi[3:])
        Xp = X + torch.cross(phi[:, None, None].expand_as(X), X, dim=0) + tau[:, None, None]
        u = K[0, 0] * Xp[0] / Xp[2] + K[0, 2]
        v = K[1, 1] * Xp[1] / Xp[2] + K[1, 2]
        tf.append(torch.stack((u - xs, v - ys)))
        disp = bf / depth
        sf.append(torch.stack((-disp, torch.zeros_like(disp))))
    return torch.stack(tf).contiguous(), torch.stack(sf).contiguous()


def _se3_exp(xi):
    """(R (3,3), t (3,), [t | quaternion xyzw] (7,)) of exp(xi), xi = [tau, phi], in float64 (closed form; the host's ground truth)."""
    tau, phi = np.asarray(xi[:3], dtype=np.float64), np.asarray(xi[3:], dtype=np.float64)
    th = float(np.linalg.norm(phi))
    Kx = np.array([[0.0, -phi[2], phi[1]], [phi[2], 0.0, -phi[0]], [-phi[1], phi[0], 0.0]])
    if th < 1e-8:
        a, b, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th), (th - np.sin(th)) / (th ** 3)
    R = np.eye(3) + a * Kx + b * Kx @ Kx
    t = (np.eye(3) + b * Kx + c * Kx @ Kx) @ tau
    half = 0.5 * th
    q = np.concatenate(((0.5 - th * th / 48.0 if th < 1e-8 else np.sin(half) / th) * phi, [np.cos(half)]))
    return R, t, np.concatenate((t, q))


def training_pairs(seed, count, h, w, bf=7.2, batch=1):
    """``count`` training batches in the reference's format (dataset/train_datasets.py as scripts/train_posenet.py:99-101 unpacks it):
    tuples (ref_img, trg_img, ref_img_r, trg_img_r, ref_mask, trg_mask, gt_pose, intrinsics, baseline) of CPU tensors with ``batch`` rows
    -- images (b,3,h,w) 0..255, masks (b,1,h,w) bool, gt_pose (b,7) [t | quaternion], intrinsics (b,3,3), baseline (b,).  A rigid scene
    in front of a moving stereo camera, rendered like ``stereo_frames`` but with the EXACT rigid motion X' = R X + t of exp(xi), so gt_pose
    = exp(xi) is the ground truth of the flow the target image was warped with: the model sees trg as image 1 and ref as image 2, and
    gt_pose moves points of the target camera into the reference camera.  Seeded; tests and benches need no dataset."""
    rng = np.random.default_rng(seed)
    K = intrinsics(h, w)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5, indexing='ij')
    for _ in range(count):
        rows = []
        for _ in range(batch):
            depth = 0.2 + 0.7 * _smooth(rng, 1, h, w, 5)[0]
            tex = 255.0 * (0.6 * _smooth(rng, 3, h, w, 24) + 0.4 * _smooth(rng, 3, h, w, 96))
            xi = np.concatenate((rng.normal(0, 0.005, 3), rng.normal(0, 0.01, 3)))
            R, t, pose = _se3_exp(xi)
            X = torch.stack(((xs - K[0, 2]) / K[0, 0] * depth, (ys - K[1, 2]) / K[1, 1] * depth, depth))
            Xp = torch.einsum('ij,jhw->ihw', torch.from_numpy(R).float(), X) + torch.from_numpy(t).float()[:, None, None]
            fx, fy = K[0, 0] * Xp[0] / Xp[2] + K[0, 2] - xs, K[1, 1] * Xp[1] / Xp[2] + K[1, 2] - ys
            disp = (bf / depth)[None]
            trg = tex[None]
            ref = _warp(trg, -fx[None], -fy[None])
            trg_r, ref_r = _warp(trg, disp, torch.zeros_like(disp)), _warp(ref, disp, torch.zeros_like(disp))
            masks = []
            for _ in range(2):
                m = torch.ones(1, h, w, dtype=torch.bool)
                y0, x0 = int(rng.integers(0, h - h // 5)), int(rng.integers(0, w - w // 4))
                m[:, y0:y0 + h // 5, x0:x0 + w // 4] = False
                masks.append(m)
            rows.append((ref[0], trg[0], ref_r[0], trg_r[0], masks[0], masks[1], torch.from_numpy(pose).float(), K, torch.tensor(bf, dtype=torch.float32)))
        yield tuple(torch.stack(col).contiguous() for col in zip(*rows))


def flow_pairs(seed, count, h, w, batch=1):
    """``count`` batches for training RAFT on ground-truth flow (train.flow_train_step): tuples (image1, image2, flow_gt, valid) of CPU
    tensors with ``batch`` rows -- images (b,3,h,w) 0..255, flow_gt (b,2,h,w) f32 in pixels, valid (b,h,w) bool, true everywhere but one
    rectangle.  Rendered as ``training_pairs`` renders its target / reference pair: a rigid scene under the exact motion X' = R X + t of
    exp(xi), image2 = image1 warped with the flow that motion induces, which is flow_gt from image1 to image2.  Seeded."""
    rng = np.random.default_rng(seed)
    K = intrinsics(h, w)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5, indexing='ij')
    for _ in range(count):
        rows = []
        for _ in range(batch):
            depth = 0.2 + 0.7 * _smooth(rng, 1, h, w, 5)[0]
            tex = 255.0 * (0.6 * _smooth(rng, 3, h, w, 24) + 0.4 * _smooth(rng, 3, h, w, 96))
            xi = np.concatenate((rng.normal(0, 0.005, 3), rng.normal(0, 0.01, 3)))
            R, t, _ = _se3_exp(xi)
            X = torch.stack(((xs - K[0, 2]) / K[0, 0] * depth, (ys - K[1, 2]) / K[1, 1] * depth, depth))
            Xp = torch.einsum('ij,jhw->ihw', torch.from_numpy(R).float(), X) + torch.from_numpy(t).float()[:, None, None]
            fx, fy = K[0, 0] * Xp[0] / Xp[2] + K[0, 2] - xs, K[1, 1] * Xp[1] / Xp[2] + K[1, 2] - ys
            image1 = tex[None]
            image2 = _warp(image1, -fx[None], -fy[None])
            valid = torch.ones(h, w, dtype=torch.bool)
            y0, x0 = int(rng.integers(0, h - h // 5)), int(rng.integers(0, w - w // 4))
            valid[y0:y0 + h // 5, x0:x0 + w // 4] = False
            rows.append((image1[0], image2[0], torch.stack((fx, fy)), valid))
        yield tuple(torch.stack(col).contiguous() for col in zip(*rows))


def infer_args(s):
    return dict(image1l=s['image1l'], image2l=s['image2l'], intrinsics=s['K'], baseline=s['baseline'], depth1=s['depth1'],
                image2r=s['image2r'], mask1=s['mask1'], mask2=s['mask2'], stereo_flow1=s['stereo_flow1'])


def model_config(h, w, iters=12, lbgfs_iters=8, solver='lbfgs', use_weights=True, mixed_precision=False, alternate_corr=False, pad_maps=False, pad_encoders=False,
                 alt_corr_fp16=False, update_fp16=False):
    """The ``model`` section of configuration/train.yaml:1-9 of the reference + image shape / solver settings.
    ``mixed_precision`` (upstream RAFT's flag): fp16 feature maps into the correlation (BASELINE config 5).
    ``alternate_corr`` (upstream RAFT's flag): the correlation windows recomputed from the feature maps at every iteration, no all-pairs volume.
    ``alt_corr_fp16`` (needs ``alternate_corr``): that route on fp16 feature maps (BASELINE config 5 without the volume).
    ``update_fp16``: the update block's convolutions with fp16 operands on the 16-bit matrix cores (raft.UPDATE_FP16 states the contract)."""
    return dict(small=False, dropout=0.0, iters=iters, pose_scale=1.0, lbgfs_iters=lbgfs_iters, use_weights=use_weights,
                image_shape=(h, w), solver=solver, mixed_precision=mixed_precision, alternate_corr=alternate_corr, pad_maps=pad_maps, pad_encoders=pad_encoders,
                update_fp16=update_fp16, alt_corr_fp16=alt_corr_fp16)


def init_synthetic_weights(model, seed=1234, flow_bias=-0.35):
    """Seeded re-initialisation of every parameter (module default initialisers, in module order) plus one
    deterministic adjustment: a negative x bias on the flow head.  Untrained RAFT drifts to positive x flow, which
    would make every stereo depth invalid (depth = bf / -flow.x, pose_net.py:73-75) and hand the solver an
    all-masked problem; the bias keeps disparities negative so all stages do real work on synthetic data."""
    torch.manual_seed(seed)
    for m in model.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            m.reset_parameters()
        elif isinstance(m, torch.nn.BatchNorm2d):
            m.reset_parameters()
            m.reset_running_stats()
    with torch.no_grad():
        if hasattr(model, 'loss_weight'):
            model.loss_weight.fill_(1.0)
        raft = model.flow if hasattr(model, 'flow') else model
        raft.update_block.flow_head.conv2.bias.copy_(torch.tensor([flow_bias, 0.0]))
    return model


def surfel_scene(h=32, w=48, steps=20, seed=3):
    """Seeded frames for the surfel map (tests/golden/surfel_map.npz, tools/bench_f2m.py): K (3,3) and steps+1 tuples (img (1,3,h,w)
    0..255, depth (1,1,h,w) in mm around 60, mask (1,1,h,w) bool ~88 % valid, confidence (1,1,h,w) in [0.5, 1.5)).  A smooth surface
    plus 0.4 mm noise per frame; torch.Generator draws on the CPU, so every machine regenerates the same frames."""
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[41.3 * w / 48, 0.0, 23.7 * w / 48], [0.0, 40.9 * w / 48, 16.2 * h / 32], [0.0, 0.0, 1.0]])
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    base = 60.0 + 6.0 * torch.sin(xx * (48 / w) / 9.0) + 4.0 * torch.cos(yy * (32 / h) / 7.0)
    frames = []
    for _ in range(steps + 1):
        depth = (base + 0.4 * torch.randn(h, w, generator=g))[None, None]
        img = torch.rand(1, 3, h, w, generator=g) * 255.0
        mask = torch.rand(1, 1, h, w, generator=g) > 0.12
        conf = 0.5 + torch.rand(1, 1, h, w, generator=g)
        frames.append((img, depth, mask, conf))
    return K, frames


def surfel_pose(k, scale=1.0):
    """xi (1,6) of step k of the surfel scene's camera path (translation mm first, then rotation): SE3.exp of it is the step's pose."""
    return torch.tensor([[0.05 * k, -0.03 * k, 0.02 * k, 0.002 * k, -0.001 * k, 0.0015 * k]]) * scale
