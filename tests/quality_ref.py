"""Test infrastructure: float64 CPU truth of the solve-quality report (rpe_pose_quality, include/rpe.h) and the seeded inputs the
kernel tests share.

``reference`` takes f, g and H from ``oracle.pose_head._prep`` / ``evaluate(need_hessian=True)`` -- the restatement of the reference's
objective that the solver tests already trust -- restates the two gates of core/pose/pose_head.py:12-58 for the counts and sums
(``bad`` / ``ok3`` of oracle.pose_head.evaluate) and inverts H with torch.linalg.inv:  C = (2 f / (m - 6)) H^-1.
"""
import torch

from oracle import pose_head as oph
from oracle import se3 as ose3

F64 = torch.float64


def reference(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight, T):
    """dict of (n, ...) f64 / int64 tensors named after the slots of rpe_pose_quality, plus H (n,6,6) and cond (n,)."""
    P = oph._prep(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight)
    n, h, w = P['n'], P['h'], P['w']
    T = torch.as_tensor(T).to(F64).reshape(n, 7)
    ev = oph.evaluate(P, T, need_hessian=True)
    # the gates, restated (oracle.pose_head.evaluate: ``bad`` / ``ok3``)
    X = ose3.se3_act(T.reshape(n, 1, 7), P['pcl1'].permute(0, 2, 1))
    ipts = torch.einsum('nij,npj->npi', P['K'], X)
    depth = torch.clamp(ipts[..., 2], 1e-12, None)
    fx = P['pix'][0][None] + P['flow'][:, 0]
    fy = P['pix'][1][None] + P['flow'][:, 1]
    ex, ey = fx - ipts[..., 0] / depth, fy - ipts[..., 1] / depth
    e2 = ex * ex + ey * ey
    r2 = e2 * P['w1']
    inimg = (fx > 0) & (fy > 0) & (fx < w) & (fy < h)
    keep2 = ~(torch.isinf(r2) | torch.isnan(r2) | ~inimg | ~P['m1'])
    keep3 = P['m1'] & P['m2']
    e3 = ((X - P['pcl2'].permute(0, 2, 1)) ** 2).sum(-1)
    zero = torch.zeros_like(e2)
    sel = lambda keep, v: torch.where(keep, v, zero).sum(1)
    n2d, n3d = keep2.sum(1), keep3.sum(1)
    m = 2 * n2d + 3 * n3d
    f, g, H = ev['f'], ev['g'], ev['H']
    _, info = torch.linalg.cholesky_ex(H)
    pd = (info == 0) & (m > 6) & torch.isfinite(f)
    C = torch.full((n, 6, 6), float('nan'), dtype=F64)
    cond = torch.full((n,), float('nan'), dtype=F64)
    for i in range(n):
        if bool(pd[i]):
            C[i] = (2.0 * f[i] / float(m[i] - 6)) * torch.linalg.inv(H[i])
            cond[i] = torch.linalg.cond(H[i])
    return dict(n2d=n2d, n3d=n3d, sum_w1=sel(keep2, P['w1']), sum_w2=sel(keep3, P['w2']), sse2d=sel(keep2, r2), sse3d=sel(keep3, e3 * P['w2']),
                rms2d_px=torch.sqrt(sel(keep2, e2) / n2d.to(F64)), rms3d=torch.sqrt(sel(keep3, e3) / n3d.to(F64)),
                f=f, g=g, grad_max=g.abs().max(dim=1).values, cov=C, pd=pd, m=m, H=H, cond=cond)


def make_inputs(n, h, w, seed, nan_rows=(), z_rows=(), z_in_image=False):
    """Seeded solver inputs with a known geometry, so that a solve has something to find and H is well conditioned: pcl1 back-projects
    the pixel grid at a smooth random depth in [0.6, 1.4]; pcl2 and the flow are what a small rigid motion makes of it, plus noise.
    On top: partial masks, non-unit weights in [0.05, 1], a band of flows that leave the image on each border; in ``nan_rows`` one NaN
    flow value (a NaN residual); in ``z_rows`` one point with z = -0.5 < 1e-12 (the depth clamp) -- with its flow leaving the image, or
    (``z_in_image``) kept by the reprojection term with w1 = 0, where its 1e13-pixel residual enters the unweighted RMS alone.
    CPU tensors in the order of the pose layer's arguments."""
    g = torch.Generator().manual_seed(seed)
    K1 = torch.tensor([[1.1 * w, 0.0, w / 2.0], [0.0, 1.1 * w, h / 2.0], [0.0, 0.0, 1.0]], dtype=F64)
    pix = oph.img_coords(h, w).to(F64)                                                   # (3, hw)
    coarse = torch.rand(n, 1, 5, 7, generator=g, dtype=F64)
    depth = 0.6 + 0.8 * torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=True).reshape(n, 1, -1)
    pcl1 = (torch.linalg.inv(K1) @ pix)[None] * depth                                    # (n, 3, hw)
    xi = torch.randn(n, 6, generator=g, dtype=F64) * torch.tensor([0.01, 0.01, 0.01, 0.004, 0.004, 0.004], dtype=F64)
    Tt = ose3.se3_exp(xi)
    Xt = ose3.se3_act(Tt.reshape(n, 1, 7), pcl1.permute(0, 2, 1))                        # (n, hw, 3)
    ip = torch.einsum('ij,npj->npi', K1, Xt)
    proj = torch.stack((ip[..., 0] / ip[..., 2], ip[..., 1] / ip[..., 2]), dim=1)        # (n, 2, hw)
    flow = proj - pix[None, :2] + 0.3 * torch.randn(n, 2, h * w, generator=g, dtype=F64)
    pcl2 = Xt.permute(0, 2, 1) + 0.004 * torch.randn(n, 3, h * w, generator=g, dtype=F64)
    flow = flow.reshape(n, 2, h, w).float()
    flow[:, 0, :, :2] -= 4.0                                                             # left / top band: targets left of / above the image
    flow[:, 1, :2, :] -= 4.0
    flow[:, 0, :, -1] += 3.0                                                             # right / bottom edge: beyond it
    flow[:, 1, -1, :] += 3.0
    pcl1 = pcl1.reshape(n, 3, h, w).float()
    pcl2 = pcl2.reshape(n, 3, h, w).float()
    w1 = 0.05 + 0.95 * torch.rand(n, 1, h, w, generator=g)
    w2 = 0.05 + 0.95 * torch.rand(n, 1, h, w, generator=g)
    m1 = torch.rand(n, 1, h, w, generator=g) > 0.15
    m2 = torch.rand(n, 1, h, w, generator=g) > 0.2
    y0, x0 = h // 2, w // 3
    for r in nan_rows:
        flow[r, 0, y0, x0] = float('nan')
        m1[r, 0, y0, x0] = True
    for r in z_rows:
        pcl1[r, :, y0 + 1, x0 + 2] = torch.tensor([0.0, 0.0, -0.5])                      # behind the camera: iz < 1e-12 at any pose near the identity
        pcl2[r, :, y0 + 1, x0 + 2] = torch.tensor([0.001, -0.002, -0.497])                # (an ordinary 3-D residual)
        m1[r, 0, y0 + 1, x0 + 2] = m2[r, 0, y0 + 1, x0 + 2] = True
        if z_in_image:
            flow[r, :, y0 + 1, x0 + 2] = 0.5
            w1[r, 0, y0 + 1, x0 + 2] = 0.0
        else:
            flow[r, 0, y0 + 1, x0 + 2] = -2.0 * w
    K = K1.float()[None].repeat(n, 1, 1)
    lw = torch.tensor([[1.0, 1.0], [0.7, 1.3], [2.0, 0.5]])[torch.arange(n) % 3]
    return [flow, pcl1, pcl2, w1, w2, m1, m2, K, lw]
