"""Independent float64 truth for the backward of the declarative pose layer (csrc/pose_backward.hip, and the forward reduce of
csrc/pose.hip), and the edge cases its tests run.  No tests in here.

The truth shares no algebra with the kernels or with oracle/pose_grad.py: the objective of the reference's core/pose/pose_head.py:12-58 is
written plainly in torch float64 as a function of a tangent vector xi at a fixed pose T0,
    X = (expm(hat(xi)) T0) pcl1 ,  a = K X ,  d = clamp(a_z, 1e-12) ,  r2 = |pix + flow - a_xy / d|^2 w1 ,  r3 = |X - pcl2|^2 w2 ,
    f = lw1 mean(where(bad, 0, r2)) / (h w) + lw0 mean(where(m1 & m2, r3, 0)) ,
with ``torch.linalg.matrix_exp`` of the 4x4 twist, and everything else is autograd at xi = 0:
    fY = df/dxi ;  H = d2f/dxi2 (the Hessian of f(exp(xi) T0), which is what the reference's symmetrised fYY equals: the symmetrised product
    of left Lie derivatives) ;  the input gradients for a given u are d(u . fY)/dx by double backward.
No ``Transform`` trick, no hand-written Jacobian, no derivative of the projection appears.  Rows are independent, so a batch is one graph.

tests/test_pose_grad_truth_cpu.py pins this to the reference's own autograd results (tests/golden/backward_{a,b}.npz) and measures its
float64 disagreement with oracle/pose_grad.py on every case below (``F64_DISAGREEMENT``)."""
import numpy as np
import torch

from oracle import se3 as ose3
from oracle import synth

F64 = torch.float64
GRADS = ('flow', 'pcl1', 'pcl2', 'w1', 'w2')
F32_EPS = 2.0 ** -23

# Largest float64 disagreement seen between this file and oracle/pose_grad.py over every case of ``CASES``, per per-pixel output, as a
# fraction of the PIXEL's own largest |gradient| over its channels (a per-pixel output is a per-pixel computation: its rounding scales with
# the pixel, not with the row).  The figures as measured (docstring of tests/test_pose_grad_truth_cpu.py).  They move with the host's
# float64 library in the last bits, amplified where a pixel's terms cancel (w1 was 7.6e-12 on one host, 3.7e-11 on another), so the host
# test holds a run to the floor these figures give the GPU comparison, ten times them, not to the figures themselves.
F64_DISAGREEMENT = dict(flow=1.3e-14, pcl1=1.1e-14, pcl2=1.9e-15, w1=3.7e-11, w2=1.2e-11)


# ------------------------------------------------------------------------------------------------- the truth
def _pose_matrix(vec7):
    """(n,7) [t, q = (x, y, z, w)] -> (n,4,4)."""
    t, (x, y, z, w) = vec7[:, :3], vec7[:, 3:].unbind(-1)
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)), dim=-1).reshape(-1, 3, 3)
    M = torch.zeros(vec7.shape[0], 4, 4, dtype=F64)
    M[:, :3, :3], M[:, :3, 3], M[:, 3, 3] = R, t, 1.0
    return M


def _twist(xi):
    """hat(xi) (n,4,4) of xi = (tau, phi)."""
    tx, ty, tz, px, py, pz = xi.unbind(-1)
    o = torch.zeros_like(tx)
    return torch.stack((o, -pz, py, tx, pz, o, -px, ty, -py, px, o, tz, o, o, o, o), dim=-1).reshape(-1, 4, 4)


def objective(x, T0, xi):
    """f (n,), its two terms without loss weight, and what the gates saw, at the pose exp(xi) T0.  ``x``: dict of float64 leaves."""
    n, _, h, w = x['flow'].shape
    P = torch.linalg.matrix_exp(_twist(xi)) @ T0
    X = P[:, :3, :3] @ x['pcl1'].reshape(n, 3, -1) + P[:, :3, 3:]
    a = x['K'] @ X
    d = torch.clamp(a[:, 2], 1e-12, None)
    px = torch.arange(w, dtype=F64) + 0.5
    py = torch.arange(h, dtype=F64) + 0.5
    pix = torch.stack((px[None, :].expand(h, w).reshape(-1), py[:, None].expand(h, w).reshape(-1)))
    fo = pix[None] + x['flow'].reshape(n, 2, -1)
    r2 = ((fo - a[:, :2] / d[:, None]) ** 2).sum(1) * x['w1'].reshape(n, -1)
    m1, m2 = x['mask1'].reshape(n, -1), x['mask2'].reshape(n, -1)
    inimg = (fo[:, 0] > 0) & (fo[:, 1] > 0) & (fo[:, 0] < w) & (fo[:, 1] < h)
    bad = torch.isinf(r2) | torch.isnan(r2) | ~inimg | ~m1
    loss2d = torch.where(bad, torch.zeros_like(r2), r2).mean(1) / (h * w)
    r3 = ((X - x['pcl2'].reshape(n, 3, -1)) ** 2).sum(1) * x['w2'].reshape(n, -1)
    loss3d = torch.where(m1 & m2, r3, torch.zeros_like(r3)).mean(1)
    f = x['loss_weight'][:, 1] * loss2d + x['loss_weight'][:, 0] * loss3d
    return f, loss2d, loss3d, dict(a_z=a[:, 2].detach(), inimg=inimg, bad=bad, ok3=m1 & m2)


def truth(args, T, u=None):
    """Everything the kernels return, by autograd: f, fY, g2u, g3u (n,6), H (n,6,6), the gates, and with ``u`` (n,6) the gradients of u . fY
    for flow, pcl1, pcl2, w1, w2, loss_weight -- raw: 0 * NaN is NaN, as in the reference (``nan_rule`` is its clean-up)."""
    names = ('flow', 'pcl1', 'pcl2', 'w1', 'w2', 'mask1', 'mask2', 'K', 'loss_weight')
    x = {k: (a.detach().to(F64).requires_grad_(k in GRADS or k == 'loss_weight') if a.is_floating_point() else a.bool()) for k, a in zip(names, args)}
    n = x['flow'].shape[0]
    T0 = _pose_matrix(torch.as_tensor(T).detach().to(F64).reshape(n, 7))
    xi = torch.zeros(n, 6, dtype=F64, requires_grad=True)
    f, l2, l3, gates = objective(x, T0, xi)
    grad = torch.autograd.grad
    fY, = grad(f.sum(), xi, create_graph=True)
    g2u, = grad(l2.sum(), xi, retain_graph=True)
    g3u, = grad(l3.sum(), xi, retain_graph=True)
    H = torch.stack([grad(fY[:, i].sum(), xi, retain_graph=True)[0] for i in range(6)], dim=1)
    out = dict(f=f.detach(), fY=fY.detach(), g2u=g2u, g3u=g3u, H=H, **gates)
    if u is not None:
        wrt = GRADS + ('loss_weight',)
        gs = grad((torch.as_tensor(u).to(F64).reshape(n, 6) * fY).sum(), [x[k] for k in wrt])
        out.update({'g_' + k: g for k, g in zip(wrt, gs)})
    return out


def nan_rule(g):
    """gradient[isnan] = 0 (declerative_node_lie.py:76)."""
    return torch.where(torch.isnan(g), torch.zeros_like(g), g)


def reference_returns_zeros(fY, eps=1e-3):
    """declerative_node_lie.py:43-47: the layer's backward warns and returns zeros unless |fY| <= eps everywhere (NaN fails the check)."""
    return not torch.allclose(fY, torch.zeros_like(fY), rtol=0.0, atol=eps)


def pixel_scale(t):
    """(n,1,h,w): each pixel's largest |gradient| over its channels."""
    return t.abs().amax(dim=1, keepdim=True)


def pixel_bound(t, name):
    """Per element: one float32 rounding of the truth + ten times the float64 disagreement of the two CPU evaluations at that pixel (the
    factor covers a third operation order, the kernel's)."""
    return F32_EPS * t.abs() + 10.0 * F64_DISAGREEMENT[name] * pixel_scale(t)


def pixel_misses(got, t, name):
    """Elements of the float32 ``got`` outside ``pixel_bound`` of the float64 truth ``t`` (equal infinities pass; nothing is left out)."""
    g = got.detach().cpu().to(F64)
    return int((~((g == t) | ((g - t).abs() <= pixel_bound(t, name)))).sum())


# ------------------------------------------------------------------------------------------------- the cases
def general_K(n, h, w):
    """Skew and an off-centre principal point in every row (cycling over three variants); the third variant also fills K[1,0] and the last
    row, which no camera has but the kernels multiply through."""
    rows = []
    for i in range(n):
        skew, ox, oy = ((3.0, 0.11, -0.07), (-2.0, -0.09, 0.13), (0.75, 0.06, 0.05))[i % 3]
        K = np.array([[1.1 * w, skew, (0.5 + ox) * w], [0.0, 1.23 * w, (0.5 + oy) * h], [0.0, 0.0, 1.0]])
        if i % 3 == 2:
            K[1, 0], K[2] = 1.5, (0.02, -0.03, 1.05)
        rows.append(K)
    return torch.from_numpy(np.stack(rows)).float()


def _base(seed, n, h, w, xi_gt, mask_p=0.85, lw=((0.3, 2.0), (1.0, 0.0), (0.7, 1.3))):
    """synth.solver_case's depths and weights, re-posed: general K, points that project onto their own pixels, flow and pcl2 induced by the
    motion ``xi_gt`` (n,6) plus noise, random masks; evaluated at T = exp(delta) exp(xi_gt) with |delta| ~ 0.01 and a seeded u."""
    c = synth.solver_case(seed, n, h, w, full_masks=True, outliers=False)
    rng = np.random.default_rng(seed + 1000)
    K = general_K(n, h, w)
    px = torch.arange(w, dtype=F64) + 0.5
    py = torch.arange(h, dtype=F64) + 0.5
    pix = torch.stack((px[None, :].expand(h, w).reshape(-1), py[:, None].expand(h, w).reshape(-1), torch.ones(h * w, dtype=F64)))
    ray = torch.linalg.inv(K.double()) @ pix[None]
    pcl1 = (c['pcl1'][:, 2].double().reshape(n, 1, -1) * ray / ray[:, 2:3]).float()
    xi_gt = torch.as_tensor(xi_gt, dtype=F64).reshape(-1, 6)
    xi_gt = xi_gt[torch.arange(n) % xi_gt.shape[0]]
    Tg = ose3.se3_exp(xi_gt)
    X = ose3.se3_act(Tg[:, None], pcl1.double().permute(0, 2, 1)).permute(0, 2, 1)
    a = K.double() @ X
    flow = a[:, :2] / a[:, 2:3] - pix[None, :2] + 0.05 * torch.from_numpy(rng.normal(size=(n, 2, h * w)))
    pcl2 = X + 1e-3 * torch.from_numpy(rng.normal(size=(n, 3, h * w)))
    m1 = torch.from_numpy(rng.uniform(size=(n, 1, h, w)) < mask_p)
    m2 = torch.from_numpy(rng.uniform(size=(n, 1, h, w)) < mask_p)
    T = ose3.se3_mul(ose3.se3_exp(torch.from_numpy(rng.normal(0, 0.01, size=(n, 6)))), Tg)
    u = torch.from_numpy(rng.normal(size=(n, 6)))
    lw = torch.tensor(lw)[torch.arange(n) % len(lw)]
    return dict(flow=flow.float().reshape(n, 2, h, w), pcl1=pcl1.reshape(n, 3, h, w), pcl2=pcl2.float().reshape(n, 3, h, w), w1=c['w1'], w2=c['w2'],
                mask1=m1, mask2=m2, K=K, loss_weight=lw, T=T, u=u, planted={})


SMALL = [[0.01, -0.02, 0.015, 0.02, -0.03, 0.025]]
# up to 0.5 rad about directions off every axis, |t| about 0.1
LARGE = [[0.06, -0.05, 0.06, 0.5 / 3, 1.0 / 3, -1.0 / 3], [-0.05, 0.07, 0.04, -0.2, 0.1, 0.2], [0.04, 0.06, -0.07, 0.24, -0.12, 0.36]]


def _set(c, key, row, y, x, val):
    c[key][row, :, y, x] = torch.as_tensor(val, dtype=c[key].dtype)


def _plant(c, name, row, y, x, **vals):
    for key, val in vals.items():
        _set(c, key, row, y, x, val)
    c['planted'].setdefault(name, []).append((row, y, x))


def _f32_towards(v, to):
    return float(np.nextafter(np.float32(v), np.float32(to)))


def case_motion():
    """Large motion and general K: 3 rows of 33x41 (more than one block in both kernels), loss weights (0.3, 2), (1, 0), (0.7, 1.3)."""
    return _base(81, 3, 33, 41, LARGE)


def case_gates():
    """The strict image bounds from both sides, the four mask combinations and zero weights, in two rows of 9x13 (large motion, general K)."""
    h, w = 9, 13
    c = _base(82, 2, h, w, LARGE[1:], mask_p=1.1, lw=((0.3, 2.0), (0.7, 1.3)))
    for r in range(2):
        on = dict(mask1=True, mask2=True, w1=0.4, w2=0.6)
        _plant(c, 'fx_on_0', r, 1, 2, flow=(-2.5, 0.25), **on)                                   # fx == 0: out (strict)
        _plant(c, 'fx_on_W', r, 2, 5, flow=(w - 5.5, 0.25), **on)
        _plant(c, 'fy_on_0', r, 3, 4, flow=(0.25, -3.5), **on)
        _plant(c, 'fy_on_H', r, 4, 7, flow=(0.25, h - 4.5), **on)
        _plant(c, 'fx_inside_0', r, 1, 8, flow=(_f32_towards(-8.5, 0), 0.25), **on)              # the nearest float32 flow on the inside: in
        _plant(c, 'fx_inside_W', r, 2, 9, flow=(_f32_towards(w - 9.5, 0), 0.25), **on)
        _plant(c, 'fy_inside_0', r, 5, 3, flow=(0.25, _f32_towards(-5.5, 0)), **on)
        _plant(c, 'fy_inside_H', r, 6, 10, flow=(0.25, _f32_towards(h - 6.5, 0)), **on)
        for k, (a, b) in enumerate(((True, True), (True, False), (False, True), (False, False))):
            _plant(c, 'mask_%d%d' % (a, b), r, 7, 1 + 2 * k, flow=(0.5, -0.25), mask1=a, mask2=b, w1=0.4, w2=0.6)
        _plant(c, 'w1_zero', r, 8, 2, flow=(0.5, -0.25), mask1=True, mask2=True, w1=0.0, w2=0.6)
        _plant(c, 'w2_zero', r, 8, 4, flow=(0.5, -0.25), mask1=True, mask2=True, w1=0.4, w2=0.0)
        _plant(c, 'w12_zero', r, 8, 6, flow=(0.5, -0.25), mask1=True, mask2=True, w1=0.0, w2=0.0)
    return c


def case_clamp():
    """Points on and behind the camera plane, one with an in-image and one with an out-of-image flow each, in rows of their own (they
    outweigh ordinary pixels by ~1e24): row 0 a_z < 0 at a general pose, row 1 a_z == 0 exactly (rotation about z, t_z = 0, p_z = 0, and
    K's last row (0, 0, 1)), row 2 a_z < 0 again under the K that fills its last row (a_z = K[2] . X; an exact zero needs the last row (0, 0, 1))."""
    h, w = 6, 7
    c = _base(83, 3, h, w, LARGE, mask_p=1.1, lw=((0.3, 2.0), (0.7, 1.3), (1.0, 0.5)))
    zrot = ose3.se3_exp(torch.tensor([[0.05, -0.03, 0.0, 0.0, 0.0, 0.4]], dtype=F64))
    c['T'][1], c['T'][2] = zrot[0], zrot[0]
    on = dict(mask1=True, mask2=True, w1=0.4, w2=0.6)
    inside, outside = (0.5, -0.25), (-20.0, 0.25)
    _plant(c, 'behind_in', 0, 2, 3, pcl1=(0.05, -0.04, -0.25), flow=inside, **on)
    _plant(c, 'behind_out', 0, 4, 1, pcl1=(-0.03, 0.06, -0.5), flow=outside, **on)
    _plant(c, 'on_plane_in', 1, 1, 2, pcl1=(0.05, -0.04, 0.0), flow=inside, **on)
    _plant(c, 'on_plane_out', 1, 3, 5, pcl1=(-0.03, 0.06, 0.0), flow=outside, **on)
    _plant(c, 'behind_in', 2, 2, 2, pcl1=(0.05, -0.04, -0.25), flow=inside, **on)
    _plant(c, 'behind_out', 2, 5, 4, pcl1=(-0.03, 0.06, -0.5), flow=outside, **on)
    return c


SHAPES = [(2, 1, 1), (2, 5, 7), (1, 15, 17), (1, 6, 43), (2, 31, 33), (1, 25, 41), (1025, 2, 3)]


def case_shape(n, h, w):
    """Small motion, general K: 1x1, h w < 64, h w on both sides of 256 and of 1024 (the block size, and one block's share of the moments),
    odd widths, and 1025 rows, where the moments' block count is set by the batch and not by the image."""
    return _base(84 + n + h * w, n, h, w, SMALL, mask_p=1.1 if h * w == 1 else 0.85)


NONFINITE = tuple('%s_%s_%s' % (k, v, g) for k in ('flow', 'w1', 'pcl2', 'w2') for v in ('nan', 'inf') for g in ('in', 'out'))
NONFINITE_2D, NONFINITE_3D = NONFINITE[:8], NONFINITE[8:]       # rows 0..7: the reprojection term's inputs, rows 8..15: the 3D term's
FLOW_ROWS = slice(0, 4)                                          # the rows whose FLOW is not finite


def case_nonfinite():
    """One non-finite value per row of 5x7, at pixel (2, 3): NaN and inf in each of flow, w1, pcl2 and w2 (row = 4 input + 2 value + gate,
    names in ``NONFINITE``), in a pixel that is gated in ('_in': masks set, flow inside unless it is the planted value) or that its term's
    gate leaves out ('_out': mask1 cleared for flow, w1 and w2, mask2 cleared for pcl2)."""
    c = _base(85, 16, 5, 7, SMALL, mask_p=1.1, lw=((0.3, 2.0), (0.7, 1.3)))
    for r, name in enumerate(NONFINITE):
        key, val, gate = name.split('_')
        v = float(val)
        masks = dict(mask1=True, mask2=True) if gate == 'in' else (dict(mask1=True, mask2=False) if key == 'pcl2' else dict(mask1=False, mask2=True))
        vals = dict(flow=(0.5, -0.25))
        vals[key] = {'flow': (v, 0.25) if val == 'nan' else (0.25, v), 'pcl2': (0.1, v, 0.5)}.get(key, v)
        _plant(c, name, r, 2, 3, **vals, **masks)
    return c


# What the closed forms -- the kernels and oracle/pose_grad.py alike -- hold at the planted pixel after the NaN -> 0 rule, per output in the
# order of ``GRADS`` (flow 2, pcl1 3, pcl2 3, w1 1, w2 1 entries): 0 zero, f finite and non-zero, I +-inf.  The reference's own value is 0
# everywhere here (NaN throughout the row, then the rule); it returns zeros for the whole layer anyway, because fY is not finite.
PLANTED_PIXEL = dict(
    flow_nan_in='00 fff fff 0 f', flow_nan_out='00 000 000 0 0', flow_inf_in='00 fff fff 0 f', flow_inf_out='00 000 000 0 0',
    w1_nan_in='00 000 fff 0 f', w1_nan_out='00 000 000 0 0', w1_inf_in='00 000 fff 0 f', w1_inf_out='00 000 000 0 0',
    pcl2_nan_in='ff 000 fff f 0', pcl2_nan_out='ff 000 000 f 0', pcl2_inf_in='ff I00 fff f I', pcl2_inf_out='ff 000 000 f 0',
    w2_nan_in='ff 000 000 f f', w2_nan_out='00 000 000 0 0', w2_inf_in='ff 000 III f f', w2_inf_out='00 000 000 0 0')
# The kernels' g2u and g3u entry by entry: f finite, n NaN, I +-inf, x NaN or +-inf (which of the two depends on signs).  A non-finite flow
# leaves both finite (the pinned deviation); a non-finite w1 or w2 reaches all six entries of its term; pcl2's y coordinate reaches the
# entries it enters, J^T g = (g, X x g): 1, 3 and 5.  (Autograd and oracle/pose_grad.py spread every NaN over all six through 0 * NaN in
# their matrix products, so they agree with this row by row, not entry by entry.)
MOMENT_ENTRIES = dict(
    flow_nan_in='ffffff ffffff', flow_nan_out='ffffff ffffff', flow_inf_in='ffffff ffffff', flow_inf_out='ffffff ffffff',
    w1_nan_in='nnnnnn ffffff', w1_nan_out='nnnnnn ffffff', w1_inf_in='nnnnnn ffffff', w1_inf_out='nnnnnn ffffff',
    pcl2_nan_in='ffffff fnfnfn', pcl2_nan_out='ffffff fnfnfn', pcl2_inf_in='ffffff fIfIfI', pcl2_inf_out='ffffff fnfnfn',
    w2_nan_in='ffffff nnnnnn', w2_nan_out='ffffff nnnnnn', w2_inf_in='ffffff xxxxxx', w2_inf_out='ffffff nnnnnn')


def classes(v, like=None):
    """One letter per entry of ``v``: n NaN, I +-inf, 0 zero, f other; with ``like``, 'x' wherever ``like`` has it and ``v`` is n or I."""
    out = ['n' if x != x else ('I' if abs(x) == float('inf') else ('0' if x == 0 else 'f')) for x in v.reshape(-1).tolist()]
    if like is not None:
        out = ['x' if (l == 'x' and o in 'nI') else o for o, l in zip(out, like.replace(' ', ''))]
    return ''.join(out)


def planted_classes(grads, c):
    """{name: 'flow pcl1 pcl2 w1 w2' classes} of per-pixel gradients (dict by ``GRADS``) at the planted pixels of ``case_nonfinite``."""
    return {name: ' '.join(classes(grads[k][r, :, y, x].cpu()) for k in GRADS) for name in NONFINITE for r, y, x in c['planted'][name]}


def sanitised(c):
    """``case_nonfinite`` with every planted value replaced by a finite one and its term gated out by other means: a flow that leaves the
    image for the reprojection term's rows, mask2 cleared for the 3D term's.  The other pixels' gradients do not depend on the planted
    pixel, and for a non-finite FLOW the kernels compute exactly this case's moments too (they select 0 for a non-finite 2D residual where
    autograd multiplies by it), so its truth pins their present values."""
    s = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    for name in NONFINITE_2D + NONFINITE_3D:
        for r, y, x in c['planted'][name]:
            if name in NONFINITE_2D:
                _set(s, 'flow', r, y, x, (-50.0, 0.25))
                _set(s, 'w1', r, y, x, 0.4)
            else:
                _set(s, 'pcl2', r, y, x, (0.1, 0.2, 0.5))
                _set(s, 'w2', r, y, x, 0.6)
                _set(s, 'mask2', r, y, x, False)
    return s


CASES = dict(motion=case_motion, gates=case_gates, clamp=case_clamp, nonfinite=case_nonfinite,
             **{'shape_%dx%dx%d' % s: (lambda s=s: case_shape(*s)) for s in SHAPES})
_cache = {}


def case(name):
    """(case, truth at its T and u): built once, shared, never modified."""
    if name not in _cache:
        c = CASES[name]()
        _cache[name] = (c, truth(args_of(c), c['T'], c['u']))
    return _cache[name]


def args_of(c):
    return tuple(c[k] for k in ('flow', 'pcl1', 'pcl2', 'w1', 'w2', 'mask1', 'mask2', 'K', 'loss_weight'))


def planted_mask(c, names=None):
    """(n,1,h,w) bool: the planted pixels of the named classes (all by default)."""
    m = torch.zeros_like(c['mask1'], dtype=torch.bool)
    for name, where in c['planted'].items():
        if names is None or name in names:
            for r, y, x in where:
                m[r, 0, y, x] = True
    return m
