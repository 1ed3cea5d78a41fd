"""Plain-torch CPU restatement of the reference's surfel map (core/fusion/surfel_map.py) for the surfel tests: the same torch operations
in the same order, written against the (3,N) / (1,N) layout, SE3 as 7-vectors acted on with oracle.se3.  Used to pin the HIP kernels
at sizes the golden file does not hold, and to find the candidates of a rendered pixel (ties).

Every function takes ``dtype``: torch.float32 (the default) is the reference's own arithmetic, bit for bit; torch.float64 runs the same
operations on the same inputs in double precision -- the truth of tests/test_gpu_surfel_edges.py, with float32 as its yardstick."""
import torch

from oracle import se3 as ose3


def act(T, p, dtype=torch.float32):
    """T (7,) on points p (3,N): lietorch's R p + t (homogeneous w = 1 gives the same numbers)."""
    return ose3.se3_act(T.to(dtype).reshape(1, 7), p.to(dtype).T).T


def inv(T):
    return ose3.se3_inv(T.reshape(1, 7)).reshape(7)


def project(K, p, dtype=torch.float32):
    q = torch.bmm(K.to(dtype)[None], p.to(dtype)[None])[0]
    d = torch.clamp(q[2], 1e-12, None)
    return q[0] / d, q[1] / d


def pixel_coords(h, w, dtype=torch.float32):
    x = torch.linspace(0, w - 1, w, dtype=dtype).repeat(1, h, 1) + .5
    y = torch.linspace(0, h - 1, h, dtype=dtype).repeat(1, w, 1).transpose(1, 2) + .5
    return torch.vstack([x.flatten(), y.flatten(), torch.ones(h * w, dtype=dtype)])


def frame_points(K, depth, pose, dtype=torch.float32, kinv=None):
    """kinv: the inverse to use in place of torch.linalg.inv(K) (a caller that hands the kernels an exact inverse)."""
    h, w = depth.shape[-2:]
    rays = (torch.linalg.inv(K.to(dtype)) if kinv is None else kinv.to(dtype)) @ pixel_coords(h, w, dtype)
    return act(pose, depth.to(dtype).reshape(1, -1) * rays, dtype)


class RefMap:
    def __init__(self, K, img, depth, mask, confidence, pmat, d_thresh, average_pts, conf_thr=7, t_max=15, dtype=torch.float32, kinv=None):
        self.K, self.conf_thr, self.t_max, self.d_thresh, self.average = K.to(dtype), conf_thr, t_max, d_thresh, average_pts
        self.dtype, self.kinv = dtype, kinv
        self.shape = tuple(depth.shape[-2:])
        m = mask.reshape(-1)
        self.opts = frame_points(K, depth, pmat, dtype, kinv)[:, m]
        self.rgb = img.to(dtype).reshape(3, -1)[:, m]
        self.conf = confidence.to(dtype).reshape(1, -1)[:, m] / conf_thr
        self.t_created = torch.zeros(1, self.opts.shape[1], dtype=dtype)
        self.tick = 0

    def associate(self, depth, mask, pose):
        """(surfel flags, their pixels, u, v, depth difference) of fuse's association test."""
        h, w = depth.shape[-2:]
        dtype, pose = self.dtype, pose.to(self.dtype)
        fopts = frame_points(self.K, depth, pose, dtype, self.kinv)
        u, v = project(self.K, act(inv(pose), self.opts, dtype), dtype)
        inb = (u >= 0) & (v >= 0) & (u < w - 1) & (v < h - 1)
        pix = (torch.round(v[inb] - .5) * w + torch.round(u[inb] - .5)).long()
        diff = fopts[2, pix] - self.opts[2, inb]
        ok = torch.abs(diff) < self.d_thresh
        ok &= mask.reshape(-1)[pix]
        flags = inb.clone()
        flags[inb] = ok
        return flags, pix[ok], fopts, u, v, diff

    def fuse(self, img, depth, mask, pose):
        flags, pix, fopts, *_ = self.associate(depth, mask, pose)
        ccor = (torch.ones(1, depth.numel(), dtype=self.dtype) / self.conf_thr)[:, pix]
        c = self.conf[:, flags]
        rgb = img.to(self.dtype).reshape(3, -1)
        if self.average:
            self.opts[:, flags] = (c * self.opts[:, flags] + ccor * fopts[:, pix]) / (c + ccor)
            self.rgb[:, flags] = (c * self.rgb[:, flags] + ccor * rgb[:, pix]) / (c + ccor)
        self.conf[:, flags] = torch.clamp(c + ccor, 0.0, 1.0)
        new = torch.ones(depth.numel(), dtype=torch.bool)
        new[pix] = False
        new &= mask.reshape(-1)
        self.opts = torch.cat((self.opts, fopts[:, new]), dim=-1)
        self.rgb = torch.cat((self.rgb, rgb[:, new]), dim=-1)
        self.conf = torch.cat((self.conf, (torch.ones(1, depth.numel(), dtype=self.dtype) / self.conf_thr)[:, new]), dim=-1)
        self.t_created = torch.cat((self.t_created, self.tick * torch.ones(1, int(new.sum()), dtype=self.dtype)), dim=-1)
        self.tick += 1
        keep = ((self.conf >= 1.0) | ((self.tick - self.t_created) < self.t_max)).squeeze(0)
        self.last_flags, self.last_keep, self.last_new = flags, keep, new      # (association of the old surfels, prune of old + new, appended pixels: for the tests)
        self.opts, self.rgb, self.conf, self.t_created = self.opts[:, keep], self.rgb[:, keep], self.conf[:, keep], self.t_created[:, keep]


def gauss_kernel(dtype=torch.float32):
    x = torch.arange(0, 5, dtype=dtype) - 2.0
    g1 = torch.exp(-x ** 2 / (2 * 2.0 ** 2))
    g = torch.outer(g1, g1)
    g[2, 2] = 0
    return g / g.sum()


def nan_fill(x, dtype=torch.float32):
    """SparseImgInterpolator(5, 2, 0) on (C,h,w)."""
    x = x.to(dtype).clone()
    nan = torch.isnan(x)
    x[nan] = 0.0
    pad = torch.nn.functional.pad(x[None], (2, 2, 2, 2), mode='reflect')
    conv = torch.nn.functional.conv2d(pad, gauss_kernel(dtype).repeat(x.shape[0], 1, 1, 1), groups=x.shape[0])[0]
    x[nan] = conv[nan]
    return x


def render(opts, rgb, conf, K, T, shape, depth_transformed, dtype=torch.float32):
    """render with the documented winner rule (largest conf, ties to the largest index).  Returns (img (3,h,w), depth, confidence,
    mask, winner (h*w,) long or -1, tied (h*w,) bool: the pixel's largest conf was shared by several surfels)."""
    h, w = shape
    opts, rgb, conf = opts.to(dtype), rgb.to(dtype), conf.to(dtype)
    p = act(T, opts, dtype)
    u, v = project(K, p, dtype)
    valid = (v < h) & (u < w) & (v >= 0) & (u >= 0)
    idx = torch.nonzero(valid).reshape(-1)
    pix = v[idx].long() * w + u[idx].long()
    # ascending conf with ties in index order, then grouped by pixel (both sorts stable): the last of each group wins.  (Not a
    # scatter with duplicate indices: torch's CPU index_put splits those across threads, and the winner changes from run to run.)
    order = torch.argsort(conf[0, idx], stable=True)
    order = order[torch.argsort(pix[order], stable=True)]
    ps = pix[order]
    last = torch.ones_like(ps, dtype=torch.bool)
    last[:-1] = ps[1:] != ps[:-1]
    winner = torch.full((h * w,), -1, dtype=torch.long)
    winner[ps[last]] = idx[order][last]
    best = torch.full((h * w,), float('-inf'), dtype=dtype)
    best = best.scatter_reduce(0, pix, torch.nan_to_num(conf[0, idx], nan=float('inf')), 'amax')
    cnt = torch.zeros(h * w, dtype=torch.long).index_add_(0, pix, (torch.nan_to_num(conf[0, idx], nan=float('inf')) == best[pix]).long())
    has = winner >= 0
    wi = winner[has]
    img = torch.zeros(3, h * w, dtype=dtype)
    depth = torch.zeros(1, h * w, dtype=dtype)
    confidence = torch.zeros(h * w, dtype=dtype)
    img[:, has] = rgb[:, wi]
    depth[0, has] = (p if depth_transformed else opts)[2, wi]
    confidence[has] = conf[0, wi]
    img = nan_fill(img.reshape(3, h, w), dtype)
    depth = nan_fill(depth.reshape(1, h, w), dtype)
    return img, depth[0], confidence.reshape(h, w), (confidence != 0).reshape(h, w), winner, cnt > 1
