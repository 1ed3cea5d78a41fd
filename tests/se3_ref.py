"""Float64 SE(3) truth for the tests, written from the definition of the group and sharing nothing with csrc/se3_device.h or
oracle/se3.py (no import from either, none of their branches): a pose is the 4x4 matrix [[R, t], [0, 1]], the exponential is the
matrix exponential of the 4x4 twist, products / inverses / actions are matrix products.  tests/test_se3_cpu.py checks this file
against 50-digit mpmath, so it is not trusted on faith either.

Layouts are the project's: pose [tx ty tz qx qy qz qw], tangent [tau(3) phi(3)].  Everything is batched (n, .) float64 on the CPU;
inputs of another dtype are widened exactly first, so a float32 kernel is compared with the truth of the numbers it was given."""
import math

import torch

F64 = torch.float64


def _d(x):
    return x.detach().to('cpu', F64)


def hat(phi):
    """(n,3) -> (n,3,3), hat(phi) v = phi x v."""
    phi = _d(phi)
    H = torch.zeros(phi.shape[0], 3, 3, dtype=F64)
    H[:, 0, 1], H[:, 0, 2] = -phi[:, 2], phi[:, 1]
    H[:, 1, 0], H[:, 1, 2] = phi[:, 2], -phi[:, 0]
    H[:, 2, 0], H[:, 2, 1] = -phi[:, 1], phi[:, 0]
    return H


def twist_matrix(xi):
    """(n,6) -> (n,4,4): [[hat(phi), tau], [0, 0]]."""
    xi = _d(xi)
    A = torch.zeros(xi.shape[0], 4, 4, dtype=F64)
    A[:, :3, :3] = hat(xi[:, 3:])
    A[:, :3, 3] = xi[:, :3]
    return A


def exp_matrix(xi):
    """(n,6) -> (n,4,4), the matrix exponential of the twist.  The translation column of exp is linear in tau, so a large tau is divided
    by a power of two first (exactly) and the column multiplied back: matrix_exp scales and squares by the NORM of its argument, and at
    |tau| = 250 the squarings cost two digits of the rotation as well (seen against mpmath: 2e-13, with the division 1e-15)."""
    xi = _d(xi).clone()
    s = torch.exp2(torch.ceil(torch.log2(xi[:, :3].abs().amax(1).clamp(min=1.0))))
    xi[:, :3] /= s[:, None]
    M = torch.linalg.matrix_exp(twist_matrix(xi))
    M[:, :3, 3] *= s[:, None]
    return M


def rot_to_quat(R):
    """(n,3,3) rotation matrices -> unit quaternions [x y z w] with w >= 0.  Of the four ways to read a quaternion off a rotation matrix
    (divide by 4w, 4x, 4y or 4z) each row takes the one with the largest divisor, so nothing is divided by a small number."""
    R = _d(R)
    r00, r11, r22 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    four_sq = torch.stack((1 + r00 - r11 - r22, 1 - r00 + r11 - r22, 1 - r00 - r11 + r22, 1 + r00 + r11 + r22), dim=1)   # 4x^2 4y^2 4z^2 4w^2
    best = four_sq.argmax(dim=1)
    d = 2.0 * torch.sqrt(four_sq.gather(1, best[:, None])[:, 0])            # 4 * (the largest component)
    sxy, sxz, syz = R[:, 1, 0] + R[:, 0, 1], R[:, 0, 2] + R[:, 2, 0], R[:, 2, 1] + R[:, 1, 2]   # 4xy 4xz 4yz
    ax, ay, az = R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]      # 4wx 4wy 4wz
    by = (torch.stack((d / 4, sxy / d, sxz / d, ax / d), 1), torch.stack((sxy / d, d / 4, syz / d, ay / d), 1),
          torch.stack((sxz / d, syz / d, d / 4, az / d), 1), torch.stack((ax / d, ay / d, az / d, d / 4), 1))
    q = torch.stack(by, dim=1)[torch.arange(R.shape[0]), best]
    q = q / torch.linalg.norm(q, dim=1, keepdim=True)
    return torch.where(q[:, 3:] < 0, -q, q)


def quat_to_rot(q):
    """(n,4) [x y z w] -> (n,3,3); q is normalised first (a float32 quaternion is unit only to its rounding)."""
    q = _d(q)
    q = q / torch.linalg.norm(q, dim=1, keepdim=True)
    x, y, z, w = q.unbind(1)
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), dim=1)
    return R.reshape(-1, 3, 3)


def to_matrix(T):
    """(n,7) poses -> (n,4,4)."""
    T = _d(T)
    M = torch.zeros(T.shape[0], 4, 4, dtype=F64)
    M[:, :3, :3] = quat_to_rot(T[:, 3:])
    M[:, :3, 3] = T[:, :3]
    M[:, 3, 3] = 1.0
    return M


def from_matrix(M):
    """(n,4,4) -> (n,7) poses, quaternion with w >= 0."""
    return torch.cat((M[:, :3, 3], rot_to_quat(M[:, :3, :3])), dim=1)


def exp(xi):
    """(n,6) twists -> (n,7) poses."""
    return from_matrix(exp_matrix(xi))


def _left_jacobian(phi):
    """(n,3) -> (n,3,3): J = sum_k hat(phi)^k / (k+1)!, the series itself at every angle (no closed form, so no branch and no
    cancelling subtraction): for |phi| <= pi its largest term is below 2 and the 40th is below 1e-28."""
    H = hat(phi)
    eye = torch.eye(3, dtype=F64).expand_as(H)
    series, term = eye.clone(), eye.clone()
    for k in range(1, 40):
        term = term @ H / (k + 1)
        series = series + term
    return series


def log(T):
    """(n,7) poses -> (n,6) twists with |phi| <= pi: the rotation vector from atan2(|v|, w) of the quaternion taken with w >= 0, then
    tau from the linear system J(phi) tau = t."""
    T = _d(T)
    q = T[:, 3:] / torch.linalg.norm(T[:, 3:], dim=1, keepdim=True)
    q = torch.where(q[:, 3:] < 0, -q, q)
    v, w = q[:, :3], q[:, 3]
    n = torch.linalg.norm(v, dim=1)
    theta = 2.0 * torch.atan2(n, w)
    zero = n == 0
    coef = torch.where(zero, 2.0 / w, theta / torch.where(zero, torch.ones_like(n), n))
    phi = coef[:, None] * v
    tau = torch.linalg.solve(_left_jacobian(phi), T[:, :3, None])[:, :, 0]
    return torch.cat((tau, phi), dim=1)


def mul(A, B):
    return from_matrix(to_matrix(A) @ to_matrix(B))


def inv(T):
    M = to_matrix(T)
    Mi = torch.zeros_like(M)                      # [[R^T, -R^T t], [0, 1]]: the inverse of a rigid motion, no general solve
    Mi[:, :3, :3] = M[:, :3, :3].transpose(1, 2)
    Mi[:, :3, 3] = -(Mi[:, :3, :3] @ M[:, :3, 3:])[:, :, 0]
    Mi[:, 3, 3] = 1.0
    return from_matrix(Mi)


def act(T, pts):
    """T (n,7) on pts (n,m,3) -> (n,m,3): the first three rows of M [p; 1]."""
    M = to_matrix(T)
    pts = _d(pts)
    return pts @ M[:, :3, :3].transpose(1, 2) + M[:, None, :3, 3]


def chain(rel, scale=250.0, init=None):
    """The tracker's running product over (m,7) relative poses: P_k = P_{k-1} * inv(rel_k with its translation times scale), P_0 = init
    (identity if None).  Returns the (m,7) absolute poses."""
    R = to_matrix(rel)
    R[:, :3, 3] *= scale
    P = torch.eye(4, dtype=F64) if init is None else to_matrix(init.reshape(1, 7))[0]
    out = []
    for k in range(R.shape[0]):
        Ri = torch.eye(4, dtype=F64)
        Ri[:3, :3] = R[k, :3, :3].T
        Ri[:3, 3] = -Ri[:3, :3] @ R[k, :3, 3]
        P = P @ Ri
        out.append(P)
    return from_matrix(torch.stack(out))


def quat_err(q, q_ref):
    """(n,) largest component difference between unit quaternions as rotations: q and -q are one rotation."""
    q, q_ref = _d(q), _d(q_ref)
    return torch.minimum((q - q_ref).abs().amax(1), (q + q_ref).abs().amax(1))


def unit_axes(n, gen):
    a = torch.randn(n, 3, dtype=F64, generator=gen)
    return a / torch.linalg.norm(a, dim=1, keepdim=True)


PI = math.pi
# rotation angles (rad) the SE(3) tests sample: every decade from far inside the Taylor branch to pi, and both sides of the theta^2 < 1e-6 guard
ANGLES = (1e-8, 1e-6, 1e-5, 3e-4, 9.99e-4, 1.001e-3, 2e-3, 5e-3, 1e-2, 3e-2, 1e-1, 0.3, 1.0, 2.0, 3.0, PI - 1e-3, PI - 1e-6)
F64_ONLY_ANGLES = (PI - 1e-6,)                    # float32 cannot tell pi - 1e-6 from pi
TAU_SCALES = (1.0, 250.0)                         # N(0,1) translations, and the tracker's depth scale


def angles_for(dtype):
    return tuple(a for a in ANGLES if dtype == F64 or a not in F64_ONLY_ANGLES)


def decade_twists(angle, tau_scale, n, dtype, seed):
    """n twists with |phi| = angle about random axes and tau ~ N(0,1) * tau_scale, rounded to dtype (returned in that dtype)."""
    gen = torch.Generator().manual_seed(seed)
    phi = unit_axes(n, gen) * angle
    tau = torch.randn(n, 3, dtype=F64, generator=gen) * tau_scale
    return torch.cat((tau, phi), dim=1).to(dtype)


def inf_norm(x):
    return _d(x).abs().amax(1)


def scale_of(*translations):
    """(n,) max(1, |.|_inf of every given (n,3) translation-sized quantity): what an error bar is multiplied by."""
    s = torch.ones(translations[0].shape[0], dtype=F64)
    for t in translations:
        s = torch.maximum(s, inf_norm(t))
    return s


# the bars of tests/test_gpu_pose.py::test_se3_kernels_match_oracle (tol for exp, tol * 10 for the rest), times scale_of(...)
BARS = {torch.float32: {'exp': 2e-6, 'other': 2e-5}, F64: {'exp': 1e-13, 'other': 1e-12}}
