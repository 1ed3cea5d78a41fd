"""Surfel map of frame-to-model tracking on the rpe_surfel_* kernels: host mirror of the reference's core/fusion/surfel_map.py.

``SurfelMap(frame=, kmat=, pmat=, ...)`` or ``SurfelMap(opts=, rgb=, kmat=, ...)`` as in the reference; ``fuse``, ``render``,
``transform``, ``transform_cpy``, ``remove_surfels_by_confidence_and_time``, ``save_ply``, ``to`` and the properties ``opts``, ``rgb``,
``conf``, ``t_created``, ``confidence``, ``grid_pts``, ``tick``.  ``render_transformed(K, T)`` is ``transform_cpy(T).render(K)`` in one
launch (what the tracker calls every frame).

Storage: two SoA f32 buffers (8, cap) -- rows 0-2 opts, 3-5 rgb, 6 conf, 7 t_created -- and two device words per buffer (count,
overflow).  The compactions of fuse / prune read one buffer and write the other (include/rpe.h), so the map ping-pongs.  The host keeps
an upper bound of the count (+ h*w per fuse); only when that bound would pass the capacity does it read the true count (one host
synchronisation) and, if needed, grow both buffers geometrically.  The ``opts`` / ``rgb`` / ``conf`` / ``t_created`` properties are
``[:, :n]`` views and read the count (a synchronisation): they are for callers, not for the per-frame path.

``init_many`` / ``render_many`` / ``fuse_many`` run the same operations over K maps (several sequences tracked side by side) with one
launch per stage; every map stays a full SurfelMap and ends bit for bit as the single-map call leaves it.
"""
import ctypes

import numpy as np
import torch

from ._lib import SURFEL_MAX_MAPS, RpeError, SurfelMapDesc, check, lib, ptr, stream_ptr
from .se3 import SE3

_ROWS = 8


def _f32(t, name, dev):
    if not isinstance(t, torch.Tensor):
        raise RpeError(f'SurfelMap: {name} must be a tensor')
    return t.to(device=dev, dtype=torch.float32).contiguous()


def write_ply(pts, rgb, path):
    """core/utils/save_ply.py: ASCII PLY of (Z,3) points and colours; rows with NaN / inf dropped, colours x255 when max <= 1."""
    if np.max(rgb) <= 1:
        rgb *= 255
    ptsrgb = np.column_stack((pts, rgb))
    valid = ptsrgb[np.sum(np.isinf(ptsrgb) + np.isnan(ptsrgb), axis=1) == 0]
    rows = ['%010f %010f %010f %d %d %d\n' % tuple(pt) for pt in valid]
    with open(path, 'w') as f:
        f.write('ply\nformat ascii 1.0\n')
        f.write('element vertex %d\n' % len(rows))
        f.write('property float x\nproperty float y\nproperty float z\n')
        f.write('property uchar red\nproperty uchar green\nproperty uchar blue\n')
        f.write('end_header\n')
        f.writelines(rows)
    return True


class SurfelMap:
    def __init__(self, frame=None, kmat=None, pmat=None, d_thresh=100.0, average_pts=True, upscale=1, conf_thr=7, t_max=15,
                 depth_scale=1.0, opts=None, rgb=None, conf=None, img_shape=None, ignore_mask=False, capacity=None):
        self._configure(kmat, pmat, d_thresh, average_pts, upscale, conf_thr, t_max, depth_scale)
        if opts is not None:
            if rgb is None:
                raise RpeError('SurfelMap: opts= needs rgb=')
            dev = opts.device
            self.img_shape = None if img_shape is None else tuple(img_shape)
            opts = _f32(opts, 'opts', dev).reshape(3, -1)
            n = opts.shape[1]
            if conf is None:                                    # surfel_map.py:40-42
                gamma = opts[2].flatten() / torch.max(opts[2])
                conf = torch.exp(-.5 * gamma ** 2 / .6 ** 2)[None, :]
            self._setup(kmat, dev, max(n, 1) if capacity is None else max(capacity, n, 1))
            buf = self._buf[0]
            buf[0:3, :n] = opts
            buf[3:6, :n] = _f32(rgb, 'rgb', dev).reshape(3, -1)
            buf[6, :n] = _f32(conf, 'conf', dev).reshape(-1)
            buf[7, :n] = 0
            self._cnt[0][0] = n
            self._n_ub = n
        else:
            if frame is None:
                raise RpeError('SurfelMap: give frame= or opts= / rgb=')
            dev = frame.depth.device
            self.img_shape = tuple(frame.shape)
            h, w = self.img_shape
            self._setup(kmat, dev, max(h * w, capacity or 0, 1))
            mask = torch.ones((h, w), dtype=torch.bool, device=dev) if ignore_mask else frame.mask.reshape(h, w).bool().contiguous()
            depth = _f32(frame.depth, 'depth', dev)
            img = _f32(frame.img, 'img', dev)
            confidence = _f32(frame.confidence, 'confidence', dev)
            pm = self._pose(self.pmat)
            ws = self._ws(0, h, w)
            check(lib().rpe_surfel_init(ptr(depth), ptr(img), ptr(mask), ptr(confidence), h, w, ptr(self._kinv), ptr(pm), float(conf_thr),
                                        self._desc(self._cur), ptr(ws), stream_ptr()), 'rpe_surfel_init')
            self._n_ub = h * w

    def _configure(self, kmat, pmat, d_thresh, average_pts, upscale, conf_thr, t_max, depth_scale):
        if upscale != 1:
            raise NotImplementedError('SurfelMap: only upscale == 1 is supported (super-sampled fusion is not built)')
        if kmat is None:
            raise RpeError('SurfelMap: kmat is required')
        self.pmat = SE3.Identity(1) if pmat is None else pmat
        self.conf_thr, self.t_max, self.upscale, self.d_thresh = conf_thr, t_max, upscale, d_thresh
        self.depth_scale, self.average_points = depth_scale, average_pts
        self.tick = 0

    # ------------------------------------------------------------------------------------------------ storage
    def _setup(self, kmat, dev, cap):
        self.device = torch.device(dev)
        self.kmat = kmat.to(torch.float32).reshape(3, 3)
        # reproject() inverts K with torch.linalg.inv on every call (pinhole_transforms.py:81); K is fixed, so once, on the host
        self._kinv = torch.linalg.inv(self.kmat.cpu()).to(self.device).contiguous()
        self.kmat = self.kmat.to(self.device).contiguous()
        self._buf = [torch.zeros(_ROWS, cap, device=self.device), None]      # the second buffer: allocated by the first compaction
        self._cnt = [torch.zeros(2, dtype=torch.int32, device=self.device) for _ in range(2)]
        self._cur = 0
        self._n_ub = 0

    @property
    def capacity(self):
        return self._buf[self._cur].shape[1]

    def _desc(self, k):
        if self._buf[k] is None or self._buf[k].shape[1] != self.capacity:
            self._buf[k] = torch.empty(_ROWS, self.capacity, device=self.device)      # a compaction's destination: never read first
        b, c = self._buf[k], self._cnt[k]
        cap, base = b.shape[1], b.data_ptr()
        return SurfelMapDesc(base, base + 3 * cap * 4, base + 6 * cap * 4, base + 7 * cap * 4, cap, c.data_ptr(), c.data_ptr() + 4)

    def _ws(self, n_bound, h, w):
        return torch.empty(max(int(lib().rpe_surfel_workspace_bytes(n_bound, h, w)), 1), dtype=torch.uint8, device=self.device)

    def _pose(self, T):
        d = T.data if isinstance(T, SE3) else T
        return d.reshape(7).to(device=self.device, dtype=torch.float32).contiguous()

    def _grow_for(self, extra):
        """Make room for ``extra`` more surfels than the host bound allows: read the true count once, then grow geometrically."""
        if self._n_ub + extra <= self.capacity:
            return
        self._n_ub = self.n                                       # the one host synchronisation of the scheme
        need = self._n_ub + extra
        if need <= self.capacity:
            return
        cap = max(need, 2 * self.capacity)
        nb = torch.zeros(_ROWS, cap, device=self.device)
        nb[:, :self._n_ub] = self._buf[self._cur][:, :self._n_ub]
        self._buf = [None, None]                                  # the other buffer is re-made at the new size when a compaction needs it
        self._buf[self._cur] = nb

    @property
    def n(self):
        return int(self._cnt[self._cur][0])

    @property
    def overflowed(self):
        """Non-zero when a kernel would have passed the capacity (1) or the host bound was wrong (2): include/rpe.h."""
        return int(self._cnt[self._cur][1]) | int(self._cnt[1 - self._cur][1])

    def _rows(self, lo, hi):
        return self._buf[self._cur][lo:hi, :self.n]

    @property
    def opts(self):
        return self._rows(0, 3)

    @property
    def rgb(self):
        return self._rows(3, 6)

    @property
    def conf(self):
        return self._rows(6, 7)

    @property
    def t_created(self):
        return self._rows(7, 8)

    @property
    def confidence(self):
        return self.conf.view(-1)

    @property
    def grid_pts(self):
        assert self.img_shape is not None
        return self.opts.T.reshape((*self.img_shape, 3))

    # ------------------------------------------------------------------------------------------------ the reference's interface
    @torch.no_grad()
    def fuse(self, frame, pose, *args):
        """surfel_map.py:73-158: associate, update, append the unmatched masked pixels, tick += 1, prune."""
        h, w = (int(s) for s in frame.shape)
        self.img_shape = (h, w)
        self._grow_for(h * w)
        depth = _f32(frame.depth, 'depth', self.device)
        img = _f32(frame.img, 'img', self.device)
        mask = frame.mask.reshape(h, w).bool().contiguous()
        P = self._pose(pose)
        nxt = 1 - self._cur
        ws = self._ws(self._n_ub, h, w)
        check(lib().rpe_surfel_fuse(self._desc(self._cur), self._n_ub, ptr(depth), ptr(img), ptr(mask), h, w, ptr(self.kmat), ptr(self._kinv),
                                    ptr(P), float(self.d_thresh), int(bool(self.average_points)), int(self.upscale), float(self.conf_thr),
                                    int(self.tick), int(self.t_max), self._desc(nxt), ptr(ws), stream_ptr()), 'rpe_surfel_fuse')
        self._cur = nxt
        self._n_ub += h * w
        self.tick += 1

    @torch.no_grad()
    def remove_surfels_by_confidence_and_time(self):
        """surfel_map.py:150-158; returns the kept-surfel mask like the reference."""
        ok = ((self.conf >= 1.0) | ((self.tick - self.t_created) < self.t_max)).squeeze(0)
        nxt = 1 - self._cur
        check(lib().rpe_surfel_prune(self._desc(self._cur), self._n_ub, int(self.tick), int(self.t_max), self._desc(nxt),
                                     ptr(self._ws(self._n_ub, 1, 1)), stream_ptr()), 'rpe_surfel_prune')
        self._cur = nxt
        return ok

    @torch.no_grad()
    def transform(self, tr):
        """opts <- tr . opts, in place (surfel_map.py:205-210)."""
        b, cap = self._buf[self._cur], self.capacity
        check(lib().rpe_surfel_transform(ptr(b), cap, ptr(b), cap, ptr(self._cnt[self._cur]), self._n_ub, ptr(self._pose(tr)), stream_ptr()),
              'rpe_surfel_transform')

    @torch.no_grad()
    def transform_cpy(self, tr):
        """A new map with opts = tr . opts, the same rgb / conf, tick and t_created reset, pmat identity (surfel_map.py:212-219)."""
        cp = SurfelMap.__new__(SurfelMap)
        cp.__dict__.update(self.__dict__)
        cp.pmat = SE3.Identity(1)
        cp.tick = 0
        cp._buf = [None, None]                                    # only the live buffer is copied; the other is made when the copy compacts
        cp._buf[cp._cur] = self._buf[self._cur].clone()
        cp._cnt = [c.clone() for c in self._cnt]
        cp._buf[cp._cur][7].zero_()
        cp.transform(tr)
        return cp

    @torch.no_grad()
    def render(self, intrinsics=None, extrinsics=None):
        """surfel_map.py:230-264: (Frame(colors, depth, mask, confidence), None).  Depth is the untransformed z, as in the reference."""
        return self._render(intrinsics, self.pmat if extrinsics is None else extrinsics, False)

    @torch.no_grad()
    def render_transformed(self, intrinsics, T):
        """``transform_cpy(T).render(intrinsics)`` in one launch: depth is the z of T . opts."""
        return self._render(intrinsics, T, True)

    def _render(self, intrinsics, T, depth_transformed):
        from .pose_estimator import Frame
        if self.img_shape is None:
            raise RpeError('SurfelMap.render: the map has no image shape (construct it from a frame or pass img_shape=)')
        h, w = self.img_shape
        K = self.kmat if intrinsics is None else intrinsics.reshape(3, 3).to(device=self.device, dtype=torch.float32).contiguous()
        img = torch.empty(1, 3, h, w, device=self.device)
        depth = torch.empty(1, 1, h, w, device=self.device)
        confidence = torch.empty(1, 1, h, w, device=self.device)
        mask = torch.empty(1, 1, h, w, dtype=torch.bool, device=self.device)
        check(lib().rpe_surfel_render(self._desc(self._cur), self._n_ub, ptr(K), ptr(self._pose(T)), int(depth_transformed), h, w, ptr(img),
                                      ptr(depth), ptr(confidence), ptr(mask), ptr(self._ws(0, h, w)), stream_ptr()), 'rpe_surfel_render')
        return Frame(img, depth=depth, mask=mask, confidence=confidence), None

    def pcl2open3d(self, stable=True, filter=None):
        raise NotImplementedError('SurfelMap.pcl2open3d needs open3d, which this project does not depend on: use save_ply')

    def save_ply(self, path, stable=True):
        """surfel_map.py:289-300 + core/utils/save_ply.py: the stable (conf >= 1) or all surfels as ASCII PLY."""
        conf = self.conf
        keep = (conf >= 1.0).squeeze(0) if stable else torch.ones(conf.shape[1], dtype=torch.bool, device=conf.device)
        opts = self.opts.T[keep].cpu().numpy() / self.depth_scale
        rgb = self.rgb.T[keep].cpu().numpy() if self.rgb.numel() > 0 else np.zeros_like(opts)
        if (len(opts) > 0) & (len(rgb) > 0):
            write_ply(opts, rgb, path)

    def to(self, d):
        dev = torch.empty(0).to(d).device if not isinstance(d, torch.dtype) else self.device
        if isinstance(d, torch.dtype) and d != torch.float32:
            raise RpeError('SurfelMap: the kernels are f32 only')
        self._buf = [None if b is None else b.to(dev) for b in self._buf]
        self._cnt = [c.to(dev) for c in self._cnt]
        self.kmat, self._kinv = self.kmat.to(dev), self._kinv.to(dev)
        self.pmat = self.pmat.to(dev)
        self.device = dev
        return self


# ---------------------------------------------------------------------------------------------------- K maps per launch
# Several sequences tracked side by side (pose_estimator.MultiSurfelPoseEstimator): the rpe_surfel_*_many entry points run each stage
# once over all maps, and map k ends bit for bit as the single-map method leaves it.  Each map stays a full SurfelMap.

def _descs(descs):
    return (SurfelMapDesc * len(descs))(*descs)


def _ws_many(n_bounds, h, w, dev):
    nb = (ctypes.c_int64 * len(n_bounds))(*n_bounds)
    size = int(lib().rpe_surfel_workspace_bytes_many(len(n_bounds), nb, h, w))
    if size <= 0:
        raise RpeError(f'rpe_surfel_workspace_bytes_many: bad arguments ({len(n_bounds)} maps, {h}x{w})')
    return nb, torch.empty(size, dtype=torch.uint8, device=dev)


def _check_count(maps, what):
    if len(maps) > SURFEL_MAX_MAPS:
        raise RpeError(f'{what}: {len(maps)} maps, at most {SURFEL_MAX_MAPS} per call (RPE_SURFEL_MAX_MAPS)')


def _check_rows(frames, n, h, w, what, names=('img', 'depth', 'mask')):
    for name, c in (('img', 3), ('depth', 1), ('mask', 1), ('confidence', 1)):
        if name in names and getattr(frames, name).numel() != n * c * h * w:
            raise RpeError(f'{what}: frames.{name} {tuple(getattr(frames, name).shape)} is not ({n},{c},{h},{w})')


@torch.no_grad()
def init_many(frames, kmats, pmats, d_thresh=100.0, average_pts=True, upscale=1, conf_thr=7, t_max=15, depth_scale=1.0, ignore_mask=False,
              capacity=None):
    """``[SurfelMap(frame=row k of frames, kmat=kmats[k], pmat=SE3(pmats[k]), ...) for k]`` with one launch per stage: frames is a Frame
    of K rows, kmats (K,3,3), pmats (K,7) (SE3 or tensor).  Returns the K maps."""
    n = frames.img.shape[0]
    h, w = (int(v) for v in frames.shape)
    dev = frames.depth.device
    pm = (pmats.data if isinstance(pmats, SE3) else pmats).reshape(n, 7)
    maps = []
    for k in range(n):
        m = SurfelMap.__new__(SurfelMap)
        m._configure(kmats[k], SE3(pm[k:k + 1]), d_thresh, average_pts, upscale, conf_thr, t_max, depth_scale)
        m.img_shape = (h, w)
        m._setup(kmats[k], dev, max(h * w, capacity or 0, 1))
        m._n_ub = h * w
        maps.append(m)
    if n == 0:
        return maps
    _check_count(maps, 'init_many')
    _check_rows(frames, n, h, w, 'init_many', ('img', 'depth', 'mask', 'confidence'))
    mask = torch.ones((n, 1, h, w), dtype=torch.bool, device=dev) if ignore_mask else frames.mask.reshape(n, 1, h, w).bool().contiguous()
    depth, img = _f32(frames.depth, 'depth', dev), _f32(frames.img, 'img', dev)
    confidence = _f32(frames.confidence, 'confidence', dev)
    pmf = pm.to(device=dev, dtype=torch.float32).contiguous()
    kinv = (ctypes.c_void_p * n)(*[m._kinv.data_ptr() for m in maps])
    _, ws = _ws_many([0] * n, h, w, dev)
    check(lib().rpe_surfel_init_many(n, ptr(depth), ptr(img), ptr(mask), ptr(confidence), h, w, kinv, ptr(pmf), float(conf_thr),
                                     _descs([m._desc(m._cur) for m in maps]), ptr(ws), stream_ptr()), 'rpe_surfel_init_many')
    return maps


@torch.no_grad()
def render_many(maps, Ks, Ts, out=None, depth_transformed=True):
    """``maps[k].render_transformed(Ks[k], Ts[k])`` for every k in one splat and one resolve launch (``depth_transformed=False``:
    ``render(Ks[k], Ts[k])``).  Ks (K,3,3), Ts (K,7) (SE3 or tensor); the maps share one image shape.  The outputs are the rows of
    batch tensors -- img (K,3,h,w), depth / confidence (K,1,h,w), mask (K,1,h,w) bool -- or of ``out`` = (img, depth, confidence, mask)
    when given.  Returns a Frame of K rows."""
    from .pose_estimator import Frame
    n = len(maps)
    if n == 0:
        raise RpeError('render_many: no maps')
    _check_count(maps, 'render_many')
    shapes = {m.img_shape for m in maps}
    if len(shapes) != 1 or None in shapes:
        raise RpeError(f'render_many: the maps must share one image shape, got {sorted(map(str, shapes))}')
    h, w = shapes.pop()
    dev = maps[0].device
    K = Ks.reshape(n, 3, 3).to(device=dev, dtype=torch.float32).contiguous()
    T = (Ts.data if isinstance(Ts, SE3) else Ts).reshape(n, 7).to(device=dev, dtype=torch.float32).contiguous()
    if out is None:
        out = (torch.empty(n, 3, h, w, device=dev), torch.empty(n, 1, h, w, device=dev), torch.empty(n, 1, h, w, device=dev),
               torch.empty(n, 1, h, w, dtype=torch.bool, device=dev))
    img, depth, confidence, mask = out
    for t, c, dt in ((img, 3, torch.float32), (depth, 1, torch.float32), (confidence, 1, torch.float32), (mask, 1, torch.bool)):
        if tuple(t.shape) != (n, c, h, w) or t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise RpeError(f'render_many: output {tuple(t.shape)} {t.dtype} must be a contiguous ({n},{c},{h},{w}) {dt} tensor on {dev}')
    nb, ws = _ws_many([m._n_ub for m in maps], h, w, dev)
    check(lib().rpe_surfel_render_many(n, _descs([m._desc(m._cur) for m in maps]), nb, ptr(K), ptr(T), int(bool(depth_transformed)), h, w,
                                       ptr(img), ptr(depth), ptr(confidence), ptr(mask), ptr(ws), stream_ptr()), 'rpe_surfel_render_many')
    return Frame(img, depth=depth, mask=mask, confidence=confidence)


@torch.no_grad()
def fuse_many(maps, frames, poses, rows=None):
    """``maps[j].fuse(row rows[j] of frames, row rows[j] of poses)`` for every j, one launch per stage (update, block counts, scan,
    scatter): frames is a Frame of B rows, poses (B,7) (SE3 or tensor), rows defaults to 0..len(maps)-1.  The maps may differ in size
    and capacity but share d_thresh, average_pts, conf_thr and t_max; each first grows as its own fuse would (``_grow_for``), then
    flips its ping-pong buffer and advances its tick."""
    n = len(maps)
    if n == 0:
        return
    _check_count(maps, 'fuse_many')
    rows = list(range(n)) if rows is None else [int(r) for r in rows]
    B = frames.img.shape[0]
    h, w = (int(v) for v in frames.shape)
    if len(rows) != n or any(r < 0 or r >= B for r in rows):
        raise RpeError(f'fuse_many: {n} maps need {n} frame rows in [0, {B}), got {rows}')
    _check_rows(frames, B, h, w, 'fuse_many')
    if len({id(m) for m in maps}) != n:
        raise RpeError('fuse_many: a map is listed twice')
    m0 = maps[0]
    opts = (m0.d_thresh, bool(m0.average_points), m0.upscale, m0.conf_thr, m0.t_max)
    if any((m.d_thresh, bool(m.average_points), m.upscale, m.conf_thr, m.t_max) != opts for m in maps):
        raise RpeError('fuse_many: the maps must share d_thresh, average_pts, upscale, conf_thr and t_max')
    dev = m0.device
    for m in maps:
        m.img_shape = (h, w)
        m._grow_for(h * w)
    depth, img = _f32(frames.depth, 'depth', dev), _f32(frames.img, 'img', dev)
    mask = frames.mask.reshape(B, 1, h, w).bool().contiguous()
    P = (poses.data if isinstance(poses, SE3) else poses).reshape(B, 7).to(device=dev, dtype=torch.float32).contiguous()
    src = _descs([m._desc(m._cur) for m in maps])
    dst = _descs([m._desc(1 - m._cur) for m in maps])
    nb, ws = _ws_many([m._n_ub for m in maps], h, w, dev)
    ticks = (ctypes.c_int32 * n)(*[int(m.tick) for m in maps])
    rws = (ctypes.c_int32 * n)(*rows)
    kmat = (ctypes.c_void_p * n)(*[m.kmat.data_ptr() for m in maps])
    kinv = (ctypes.c_void_p * n)(*[m._kinv.data_ptr() for m in maps])
    check(lib().rpe_surfel_fuse_many(n, src, nb, dst, ticks, rws, B, ptr(depth), ptr(img), ptr(mask), h, w, kmat, kinv, ptr(P),
                                     float(m0.d_thresh), int(bool(m0.average_points)), int(m0.upscale), float(m0.conf_thr), int(m0.t_max),
                                     ptr(ws), stream_ptr()), 'rpe_surfel_fuse_many')
    for m in maps:
        m._cur = 1 - m._cur
        m._n_ub += h * w
        m.tick += 1
