"""Differentiable restatement (torch on the CPU, any float dtype) of the fused geometry stage, csrc/geometry.hip, for the tests of its backward
(csrc/geometry_backward.hip): the truth is torch autograd in float64 over these functions.  Written from the reference lines the forward cites
-- core/pose/pose_net.py:73-79 (depth from disparity, validity, proj :121-125), :104-113 (the warps and the x0.125 stacks),
core/interpol/flow_utils.py:4-14 (remap_from_flow) -- with the same torch calls as oracle/warp.py, whose ``backproject`` builds its pixel grid in
float32 and so cannot run in float64.  tests/test_geometry_backward_host.py pins this module's forward to the reference's own outputs
(tests/golden/warp.npz, geometry.npz).

Also here: the seeded cases of the GPU tests (``case``), the float32-against-float64 decision check (``decisions``) and the error measure."""
import numpy as np
import torch
import torch.nn.functional as F

INPUTS = ('stereo_flow2', 'time_flow', 'baseline', 'K', 'depth1', 'image1l', 'image2l', 'stereo_flow1', 'mask2')
UPSTREAM = ('pcl1', 'pcl2w', 'inp1', 'inp2')
GRADS = ('time_flow', 'stereo_flow2', 'stereo_flow1', 'depth1')


def grid(flow):
    n, _, h, w = flow.shape
    row, col = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    g = torch.empty_like(flow)
    g[:, 1] = 2 * (flow[:, 1] + row) / (h - 1) - 1                 # flow_utils.py:9
    g[:, 0] = 2 * (flow[:, 0] + col) / (w - 1) - 1                 # flow_utils.py:10
    return g.permute(0, 2, 3, 1)


def remap(x, flow):
    return F.grid_sample(x, grid(flow), align_corners=True)        # flow_utils.py:11 (bilinear, zero padding)


def flow2depth(stereo_flow, baseline):
    depth = baseline[:, None, None] / -stereo_flow[:, 0]           # pose_net.py:73
    valid = (depth > 0) & (depth <= 1.0)                           # :74
    return torch.where(valid, depth, torch.ones_like(depth)).unsqueeze(1), valid.unsqueeze(1)


def backproject(depth, K):
    n, _, h, w = depth.shape
    x = torch.arange(w, dtype=depth.dtype) + 0.5
    y = torch.arange(h, dtype=depth.dtype) + 0.5
    coords = torch.stack((x[None, :].expand(h, w).reshape(-1), y[:, None].expand(h, w).reshape(-1), torch.ones(h * w, dtype=depth.dtype)))
    return (depth.view(n, 1, -1) * (torch.linalg.inv(K) @ coords.view(1, 3, -1))).view(n, 3, h, w)   # proj, pose_net.py:121-125


def down8(x):
    return F.interpolate(x, scale_factor=0.125, mode='bilinear')   # pose_net.py:110-113


def remap_at_taps(taps):
    """A sampler for ``stage`` that takes the floor taps as GIVEN (x0, y0 (n,h,w) integer tensors, e.g. rpe_warp_taps' report) and the
    positions as the float32 positions widened: grid_sample's arithmetic written out (weights x0 + 1 - ix, ix - x0; a tap outside the image
    is absent), with d position / d flow = 1.  At a position that is an integer in float32 this fixes which side's taps are differentiated
    -- the forward's -- where a float64 round trip through the normalised grid could land on either side."""
    def sampler(x, flow):
        n, c, h, w = x.shape
        px32, py32 = positions(flow.detach().float(), torch.float32)
        px = px32.to(x.dtype) + (flow[:, 0] - flow[:, 0].detach())
        py = py32.to(x.dtype) + (flow[:, 1] - flow[:, 1].detach())
        x0, y0 = taps['x0'].long(), taps['y0'].long()
        flat, out = x.reshape(n, c, h * w), 0
        for dy in (0, 1):
            for dx in (0, 1):
                xx, yy = x0 + dx, y0 + dy
                ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(n, 1, h * w).expand(n, c, h * w)
                v = flat.gather(2, idx).reshape(n, c, h, w)
                wgt = ((px - x0) if dx else (x0 + 1 - px)) * ((py - y0) if dy else (y0 + 1 - py))
                out = out + torch.where(ok[:, None], v * wgt[:, None], torch.zeros_like(v))
        return out
    return sampler


def stage(stereo_flow2, time_flow, baseline, K, depth1, image1l, image2l, stereo_flow1, sampler=None):
    """pcl1, pcl2w, inp1, inp2 of rpe_depth_backproject_warp, in the dtype of the inputs (``sampler``: remap, or remap_at_taps(...))."""
    sampler = remap if sampler is None else sampler
    depth2, _ = flow2depth(stereo_flow2, baseline)
    pcl1, pcl2 = backproject(depth1, K), backproject(depth2, K)
    pcl2w = sampler(pcl2, time_flow)
    inp1 = down8(torch.cat((stereo_flow1, image1l, pcl1), dim=1))
    inp2 = down8(torch.cat((sampler(stereo_flow2, time_flow), sampler(image2l, time_flow), pcl2w), dim=1))
    return dict(pcl1=pcl1, pcl2w=pcl2w, inp1=inp1, inp2=inp2)


def stage_grads(case, upstream, dtype, sampler=None):
    """d <upstream, stage outputs> / d (time_flow, stereo_flow2, stereo_flow1, depth1) by autograd in ``dtype``; ``upstream`` maps some of
    UPSTREAM to gradient tensors (a missing one is zero).  An input no given output depends on gets zeros."""
    c = {k: case[k].to(dtype) for k in INPUTS if k != 'mask2'}
    leaves = {k: c[k].clone().requires_grad_(True) for k in GRADS}
    out = stage(leaves['stereo_flow2'], leaves['time_flow'], c['baseline'], c['K'], leaves['depth1'], c['image1l'], c['image2l'],
                leaves['stereo_flow1'], sampler=sampler)
    total = sum((out[k] * upstream[k].to(dtype)).sum() for k in UPSTREAM if upstream.get(k) is not None)
    got = torch.autograd.grad(total, [leaves[k] for k in GRADS], allow_unused=True)
    return {k: (torch.zeros_like(leaves[k]) if g is None else g).detach() for k, g in zip(GRADS, got)}


def ratio(got, truth):
    """max |got - truth| / max |truth| over EVERY element (float64); an all-zero truth admits only zeros: 0.0 then, else inf."""
    got, truth = got.detach().cpu().double(), truth.detach().cpu().double()
    assert got.shape == truth.shape, (got.shape, truth.shape)
    err, scale = float((got - truth).abs().max()), float(truth.abs().max())
    if scale == 0.0:
        return 0.0 if err == 0.0 else float('inf')
    return err / scale


# --------------------------------------------------------------------------------------------------------------------------- cases
BASELINES = (5.25, 0.8125, 2.5)
ROW_K = ((1.1, 1.3, 0.5, 0.5, 0.02), (0.9, 0.8, 0.45, 0.6, -0.05), (2.1, 1.7, 0.31, 0.77, 0.11))      # fx/w, fy/w, cx/w, cy/h, skew/w


def intrinsics(n, h, w):
    K = np.zeros((n, 3, 3), dtype=np.float32)
    for r in range(n):
        fx, fy, cx, cy, sk = ROW_K[r % 3]
        K[r] = [[fx * w, sk * w, cx * w + 0.37], [0.0, fy * w, cy * h - 1.21], [0.0, 0.0, 1.0]]
    return torch.from_numpy(K)


def flow_to(target_x, target_y):
    """time_flow (n,2,h,w) float32 = target - grid: the sampling position of pixel (y, x) is (target_x, target_y)[.., y, x] up to float32
    rounding (a few 1e-6), far inside the 0.05 margin the targets keep from every integer."""
    n, h, w = target_x.shape
    col, row = np.arange(w, dtype=np.float64)[None, None, :], np.arange(h, dtype=np.float64)[None, :, None]
    return torch.from_numpy(np.stack((target_x - col, target_y - row), axis=1).astype(np.float32))


def disparities(rng, b, shape, clamped=0.2):
    """stereo flow x: depth b / -sf.x in [0.05, 0.95] (valid), except a share ``clamped`` with the wrong sign or depth > 1; every value at
    least 1e-3 (in fact 1e-2 b) away from both thresholds (sf.x = 0 and sf.x = -b)."""
    sfx = -b / rng.uniform(0.05, 0.95, size=shape)
    u = rng.uniform(size=shape)
    sfx = np.where(u < clamped / 2, rng.uniform(0.5, 20.0, size=shape), sfx)                       # positive: negative depth
    sfx = np.where((u >= clamped / 2) & (u < clamped), -b * rng.uniform(0.05, 0.9, size=shape), sfx)   # depth in (1.1, 20)
    return sfx


def case(n, h, w, seed=0, many_to_one=False, integer_positions=False, clamp_row=None):
    """The seeded inputs of a parity test (dict of INPUTS, CPU tensors).  Targets: integer part uniform in [-1, size-1], fractional part in
    [0.05, 0.95]; about a quarter of the pixels aim more than one pixel outside the image (every tap absent).
    ``many_to_one``: every destination samples the cell (3..4, 5..6).  ``integer_positions``: integer flows (positions exactly on pixels), the
    last row and column included.  ``clamp_row``: that row's disparities are all invalid."""
    rng = np.random.default_rng(1000003 * seed + 10007 * n + 101 * h + w)
    shape = (n, h, w)
    if many_to_one:
        tx, ty = 3 + rng.uniform(0.05, 0.95, size=shape), 5 + rng.uniform(0.05, 0.95, size=shape)
    elif integer_positions:
        tx, ty = rng.integers(-2, w + 2, size=shape).astype(np.float64), rng.integers(-2, h + 2, size=shape).astype(np.float64)
        tx[:, :, -1], ty[:, -1, :] = w - 1, h - 1                        # exactly on the last column / row
        tx[:, 0, :], ty[:, :, 0] = w - 1, h - 1
    else:
        tx = rng.integers(-1, w, size=shape) + rng.uniform(0.05, 0.95, size=shape)
        ty = rng.integers(-1, h, size=shape) + rng.uniform(0.05, 0.95, size=shape)
        out = rng.uniform(size=shape) < 0.25
        side = rng.uniform(size=shape) < 0.5
        far = rng.integers(2, 6, size=shape) + rng.uniform(0.05, 0.95, size=shape)
        tx = np.where(out & side, np.where(rng.uniform(size=shape) < 0.5, -far, w - 1 + far), tx)
        ty = np.where(out & ~side, np.where(rng.uniform(size=shape) < 0.5, -far, h - 1 + far), ty)
    b = np.array([BASELINES[r % 3] for r in range(n)], dtype=np.float32)
    bb = b.astype(np.float64)[:, None, None]
    sf2 = np.stack((disparities(rng, bb, shape), rng.normal(0, 1.0, size=shape)), axis=1)
    if clamp_row is not None:
        sf2[clamp_row, 0] = rng.uniform(0.5, 20.0, size=(h, w))
    sf1 = np.stack((disparities(rng, bb, shape), rng.normal(0, 1.0, size=shape)), axis=1)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
    return dict(stereo_flow2=t32(sf2), time_flow=flow_to(tx, ty), baseline=torch.from_numpy(b), K=intrinsics(n, h, w),
                depth1=t32(rng.uniform(0.1, 1.0, size=(n, 1, h, w))), image1l=t32(rng.uniform(0, 255, size=(n, 3, h, w))),
                image2l=t32(rng.uniform(0, 255, size=(n, 3, h, w))), stereo_flow1=t32(sf1), mask2=torch.from_numpy(rng.uniform(size=(n, 1, h, w)) > 0.2))


def upstream(n, h, w, seed=0, only=None):
    """Random incoming gradients (dict of UPSTREAM, float32); with ``only`` the others are None."""
    g = torch.Generator().manual_seed(77 + seed)
    shapes = dict(pcl1=(n, 3, h, w), pcl2w=(n, 3, h, w), inp1=(n, 8, h // 8, w // 8), inp2=(n, 8, h // 8, w // 8))
    full = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    return {k: (v if only is None or k == only else None) for k, v in full.items()}


def positions(flow, dtype):
    """The un-normalised grid_sample positions (ix, iy) of ``flow`` evaluated in ``dtype``, operation by operation as torch does."""
    f = flow.to(dtype)
    n, _, h, w = f.shape
    gr = grid(f)
    return ((gr[..., 0] + 1) / 2) * (w - 1), ((gr[..., 1] + 1) / 2) * (h - 1)


def decisions(c, positions_too=True, margins=True):
    """Asserts that float32 and float64 take the same decisions on case ``c``: the same floor taps, every position's fractional part inside
    [0.04, 0.96] in both (``positions_too``; the integer-position cases are judged at the forward's own taps instead: remap_at_taps), and
    the same depth validity for both stereo flows, every disparity at least 1e-3 away from both thresholds."""
    if positions_too:
        (x32, y32), (x64, y64) = positions(c['time_flow'], torch.float32), positions(c['time_flow'], torch.float64)
        assert torch.equal(x32.floor().double(), x64.floor()) and torch.equal(y32.floor().double(), y64.floor())
        for p in (x32.double(), y32.double(), x64, y64):
            f = p - p.floor()
            assert float(f.min()) > 0.04 and float(f.max()) < 0.96
    for k in ('stereo_flow1', 'stereo_flow2'):
        v32, v64 = flow2depth(c[k], c['baseline'])[1], flow2depth(c[k].double(), c['baseline'].double())[1]
        assert torch.equal(v32, v64), k
        s, b = c[k][:, 0].double(), c['baseline'].double()[:, None, None]
        assert not margins or (float(s.abs().min()) >= 1e-3 and float((s + b).abs().min()) >= 1e-3)
