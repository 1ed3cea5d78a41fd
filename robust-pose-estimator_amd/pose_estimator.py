"""Frame-to-frame tracker host mirror: ``PoseEstimator(config, intrinsics, baseline, checkpoint, img_shape)``
called once per stereo frame, as scripts/infer_trajectory.py:50-51,71-77 of the reference does.

Follows core/pose/pose_estimator.py:26-48 (checkpoint + config overrides, 1/depth_clipping scale),
:50-96 (forward: failure gate ``isnan | |log| > 0.1`` -> identity, de-normalise, chain
``last_pose <- last_pose * rel^-1``) and :98-125 (get_pose_f2f), and core/utils/frame_class.py:5-50 (Frame).
Frame-to-model tracking (``frame2frame: False``, :56-96,127-150 with core/fusion/surfel_map.py) is ``SurfelPoseEstimator`` below;
``from_config`` picks the class from the config as scripts/infer_trajectory.py:50-51 would.  ``MultiPoseEstimator`` / ``MultiSurfelPoseEstimator``
advance K independent sequences in lockstep, one batched pass per step (``from_config_many``).
"""
import time
import warnings
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import ops
from .pose_net import PoseNet
from .se3 import SE3


class Frame:
    """Carrier of img / rimg / depth / mask / confidence / flow between consecutive calls (frame_class.py)."""

    def __init__(self, img, rimg=None, depth=None, mask=None, confidence=None, flow=None):
        assert img.ndim == 4
        self.img = img.contiguous()
        self.rimg = img.contiguous() if rimg is None else rimg.contiguous()
        shape, dev = self.img.shape[-2:], self.img.device
        n = self.img.shape[0]
        self.mask = (torch.ones((n, 1, *shape), dtype=torch.bool, device=dev) if mask is None else mask).bool()
        self.depth = torch.ones((n, 1, *shape), device=dev) if depth is None else depth.contiguous()
        self.confidence = torch.ones((n, 1, *shape), device=dev) if confidence is None else confidence.contiguous()
        self.flow = torch.zeros((n, 2, *shape), device=dev) if flow is None else flow.contiguous()
        assert self.rimg.shape == self.img.shape
        for t in (self.depth, self.mask, self.confidence, self.flow):
            assert t.shape[-2:] == shape

    @property
    def shape(self):
        return self.img.shape[-2:]

    @property
    def device(self):
        return self.img.device

    def to(self, d):
        for k in ('img', 'rimg', 'depth', 'mask', 'confidence'):
            setattr(self, k, getattr(self, k).to(d))
        return self


QUALITY_F64 = ('pd', 'n2d', 'n3d', 'rms2d_px', 'rms3d', 'f', 'grad_max')
QUALITY_I32 = ('n_iter', 'func_evals', 'stop_reason')


def blank_quality(n, device):
    """The report of n frames that had no solve (a sequence's first frame): NaN covariance, RMS, f and gradient, pd = 0, zero counts."""
    nan = float('nan')
    q = dict(cov=torch.full((n, 6, 6), nan, dtype=torch.float64, device=device))
    for k in QUALITY_F64:
        q[k] = torch.full((n,), 0.0 if k in ('pd', 'n2d', 'n3d') else nan, dtype=torch.float64, device=device)
    for k in QUALITY_I32:
        q[k] = torch.zeros(n, dtype=torch.int32, device=device)
    return q


def denormalise_quality(q, inv_scale):
    """PoseNet.infer's quality dict (the solve's normalised depth units) in the units of the pose the tracker returns
    (core/pose/pose_estimator.py:90 scales the translation by 1 / scale): rows and columns 0..2 of ``cov`` and ``rms3d`` times 1 / scale
    (millimetres); counts, ``rms2d_px`` and the solver's bookkeeping have no unit; ``f`` and ``grad_max`` stay the solver's own numbers.
    Device arithmetic only."""
    out = dict(q)
    cov = q['cov'].clone()
    cov[:, :3, :] *= inv_scale
    cov[:, :, :3] *= inv_scale
    out['cov'] = cov
    out['rms3d'] = q['rms3d'] * inv_scale
    return out


def _warn_skipped(n=1):
    """One warning per frame the gate rejected (core/pose/pose_estimator.py:82)."""
    for _ in range(n):
        warnings.warn('pose estimation not converged, skip.', RuntimeWarning)


class PoseEstimator(torch.nn.Module):
    _f2m = False

    def __init__(self, config, intrinsics, baseline, checkpoint, img_shape, init_pose=None):
        """config: the ``slam`` section of the inference YAML (configuration/infer_f2f.yaml:1-11);
        img_shape = (W, H) as in the reference; checkpoint: path, ``{'state_dict','config'}`` dict or a PoseNet."""
        super().__init__()
        if not config.get('frame2frame', True) and not self._f2m:
            raise NotImplementedError('PoseEstimator tracks frame to frame; frame2frame: False is SurfelPoseEstimator (or from_config)')
        if isinstance(checkpoint, PoseNet):
            model = checkpoint
        else:
            ckp = torch.load(checkpoint, map_location='cpu') if isinstance(checkpoint, str) else checkpoint
            mcfg = dict(ckp['config']['model'])
            mcfg['image_shape'] = (img_shape[1], img_shape[0])          # pose_estimator.py:28
            mcfg['lbgfs_iters'] = config['lbgfs_iters']
            mcfg['use_weights'] = config['conf_weighing']
            if 'solver' in config:
                mcfg['solver'] = config['solver']
            model = PoseNet(mcfg)
            state = OrderedDict((k.replace('module.', ''), v) for k, v in ckp['state_dict'].items())
            model.load_state_dict(state)
        model.eval()
        self.model = model
        self.config = config
        self.register_buffer('intrinsics', intrinsics.unsqueeze(0).float(), persistent=False)
        self.register_buffer('scale', torch.tensor(1 / config['depth_clipping'][1]), persistent=False)
        self._inv_scale = float(1 / self.scale)                      # (f32 division, once, on the host: what `1 / self.scale` gives per call in the reference, :90)
        self.register_buffer('baseline', torch.tensor(baseline).unsqueeze(0).float(), persistent=False)
        self._init_pose = SE3.Identity(1) if init_pose is None else init_pose.float()
        self.last_pose = self._init_pose
        self.frame = None
        self.last_frame = None
        # streaming: encoder outputs of the current left image, reused as image1l's on the next call (exact: both
        # encoders normalise per sample); set reuse_features=False to re-encode like the reference does
        self.reuse_features = config.get('reuse_features', True)
        self._enc_cache = None
        self._pending = []                                            # submit() / result(): frames whose encoders are already on the side stream
        self._prefetch_stream = None
        # warm start (``warm_start: True``): the temporal RAFT pass of frame t starts from ops.forward_interpolate of frame t-1's temporal
        # 1/8 flow (upstream RAFT's video warm start).  Cold after the first frame, after reset() and after a frame the gate rejected.
        self.warm_start = bool(config.get('warm_start', False))
        self._flow_low = None                                         # the last accepted temporal pass's 1/8 flow (1,2,h/8,w/8), or None
        self._low_pass = None                                         # ... of the pass in flight, until the gate has seen it
        # ``report_quality: True``: every call leaves ``last_quality`` -- PoseNet.infer's solve-quality report (covariance of the relative
        # pose's left tangent, counts, RMS residuals, the solver's stop reason ...), de-normalised like the pose, one row per frame, as device
        # tensors -- whether or not the gate accepts the frame.  Two more launches per frame and no host synchronisation; off, nothing changes.
        self.report_quality = bool(config.get('report_quality', False))
        self.last_quality = None
        self._q_pass = None                                           # the report of the pass in flight

    @property
    def device(self):
        return self.intrinsics.device

    def reset(self):
        """Forget the sequence (frames, chained pose, cached encoder outputs): the next call is a first frame again."""
        self.last_pose = self._init_pose
        self.frame = self.last_frame = None
        self._enc_cache = None
        self._pending = []
        self._flow_low = None
        self.last_quality = self._q_pass = None
        return self

    def _set_quality(self, q, n, device):
        """``last_quality`` from a pass's report ``q`` (None: n frames without a solve)."""
        if self.report_quality:
            self.last_quality = blank_quality(n, device) if q is None else denormalise_quality(q, self._inv_scale)

    def _quality_kw(self):
        return {'ret_quality': True} if self.report_quality else {}

    def _flow_init(self):
        """The temporal pass's flow_init / ret_lowres keywords of PoseNet.infer: {} without warm start."""
        if not self.warm_start:
            return {}
        return dict(ret_lowres=True, flow_init=None if self._flow_low is None else ops.forward_interpolate(self._flow_low))

    @torch.no_grad()
    def submit(self, limg, rimg, mask):
        """Pipelined form of ``forward`` for a caller that has the next frame before it needs this one's pose (a video file, a camera
        queue; scripts/infer_trajectory.py:57,71-77 iterates a DataLoader): ``submit(frame t+1)`` then ``result()`` -> frame t's pose.
        submit() puts the frame's encoder work (PoseNet.encode_frame: fnet on both images, cnet on the left one -- it depends on nothing
        else) on a side stream at once; the frame waits in a queue until result() runs the rest of ``forward`` for the oldest queued
        frame.  With frame t+1 submitted before result() is called for frame t, its encoders (~1.3 ms of launches) run beside frame t's
        update loop, whose ~100 launches per iteration leave most of the chip idle at batch 1.  Same kernels, same inputs: the poses are
        bit-identical to calling forward() frame by frame (tests/test_gpu_pipeline.py).  Requires reuse_features (the default)."""
        if not self.reuse_features:
            raise RuntimeError('submit / result reuse the encoder outputs across frames: construct the estimator with reuse_features=True')
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(limg.device))          # the images are ready on the caller's stream NOW (recorded later, the
        self._pending.append([limg, rimg, mask, None, None, ready])   #  event would sit behind the running frame's whole queue)
        if len(self._pending) == 1:
            self._start_encoders(self._pending[0])            # nothing is running that it could hide behind: start at once

    def _start_encoders(self, item):
        """Frame ``item``'s encoder work onto the side stream (once)."""
        if item[3] is not None:
            return
        limg, rimg = item[0], item[1]
        dev = limg.device
        if self._prefetch_stream is None or self._prefetch_stream.device != dev:
            self._prefetch_stream = torch.cuda.Stream(device=dev)
        side = self._prefetch_stream
        with torch.cuda.stream(side):
            side.wait_event(item[5])
            item[3] = self.model.encode_frame(limg, rimg)
            item[4] = torch.cuda.Event()
            item[4].record(side)
        for t in (limg, rimg):
            t.record_stream(side)

    @torch.no_grad()
    def result(self):
        """``forward`` for the oldest submitted frame, on its prefetched encoder outputs.  The NEXT queued frame's encoders are started
        once this frame's work has been handed to the GPU and before the host waits for its success flag: they then run beside the tail
        of this frame -- the last update iterations, the weight heads and the 20-iteration solve, whose launches occupy a few
        workgroups each."""
        if not self._pending:
            raise RuntimeError('result() without a submitted frame')
        self._start_encoders(self._pending[0])
        limg, rimg, mask, enc, done, _ = self._pending.pop(0)
        cur = torch.cuda.current_stream(limg.device)
        cur.wait_event(done)
        for t in enc.values():
            t.record_stream(cur)                              # allocated on the side stream, consumed (and freed) on the caller's
        return self.forward(limg, rimg, mask, _enc=enc)

    @torch.no_grad()
    def forward(self, limg, rimg, mask, _enc=None):
        """limg, rimg: (1,3,h,w) 0..255; mask: (1,1,h,w) True = valid.  Returns (absolute pose SE3, None, flow, weights)."""
        self.last_pose = self.last_pose.to(limg.device)
        self.last_frame = self.frame
        self.frame = Frame(limg, rimg, mask=mask)
        rel_pose, ret_frame, flow, weights = self.get_pose_f2f(_enc)
        self._gate_and_chain(rel_pose, ret_frame)
        return self.last_pose, None, flow, weights

    def _pass(self, f1, limg, rimg, mask, intrinsics, baseline, **kw):
        """A tracker's ``model.infer`` from frame 1 ``f1`` (the previous Frame, or the rendered model frame(s)) to the stereo frame(s)
        (limg, rimg, mask).  ``kw``: what differs between the trackers (cache1 / enc2 / ret_cache, the warm start's flow_init / ret_lowres,
        rows_alone), handed on as given; the quality keyword is added under ``report_quality``.  The ONE place that knows the positions in
        infer's tuple: the details, then the quality dict if asked for, then the cache dict if asked for, whose 'time_flow_low' (the
        temporal 1/8 flow of ret_lowres) is taken out of it.  Returns the parts by name; what was not asked for is None."""
        r = self.model.infer(f1.img, limg, intrinsics, baseline, depth1=f1.depth * self.scale, image2r=rimg, mask1=f1.mask, mask2=mask,
                             stereo_flow1=f1.flow, ret_details=True, **kw, **self._quality_kw())
        cache = r[-1] if kw.get('ret_cache') else None
        return SimpleNamespace(rel=r[0], depth2=r[2], weights=r[3], flow=r[4], stereo_flow=r[5], quality=r[6] if self.report_quality else None,
                               cache=cache, flow_low=cache.pop('time_flow_low') if kw.get('ret_lowres') else None)

    def _gate_and_chain(self, rel_pose, ret_frame):
        """The tail of a frame behind its network pass, core/pose/pose_estimator.py:81-91 in one launch (ops.pose_gate_chain): the gate
        isnan | |log| > 0.1 -> identity, de-normalisation of the depth scaling and last_pose <- last_pose * rel^-1, with ONE host
        synchronisation (the success flag) instead of a dozen element-wise launches and two."""
        rel, pose, ok = ops.pose_gate_chain(rel_pose.data.reshape(1, 7), self.last_pose.data, self._inv_scale, 1.0e-1)
        self._set_quality(self._q_pass, 1, self.frame.device)
        low, self._low_pass = self._low_pass, None
        if self._pending:
            self._start_encoders(self._pending[0])            # (submit / result) the next frame's encoders, before the host waits for this one
        self.t_enqueued = time.perf_counter()             # everything of this frame has been handed to the runtime; what follows waits for the GPU
        self.success = bool(ok[0])
        if not self.success:
            _warn_skipped()
        self._flow_low = low if self.success else None                # (a rejected frame: the next pair spans two frames, start it cold)
        self.last_rel_pose = SE3(rel)
        self.last_frame = ret_frame
        self.last_pose = SE3(pose)

    @torch.no_grad()
    def forward_chunk(self, limgs, rimgs, masks):
        """``forward`` for c consecutive frames in ONE pass (PoseNet.infer_chunk): limgs, rimgs (c,3,h,w), masks (c,1,h,w), after at
        least one ``forward`` call (the sequence's first frame only gets its stereo depth).  Bit-identical to c single calls: same
        relative poses, same gate decisions, same chained poses, same Frame left behind.  Returns the (c,7) absolute poses;
        ``last_rel_poses`` (c,7) gated relative poses and ``successes`` (c,) bool are left on the estimator, the gate is evaluated on
        the device with ONE host synchronisation per chunk (for the warnings) instead of two per frame."""
        if self.warm_start:
            raise ValueError('forward_chunk computes a chunk\'s temporal flows in one RAFT pass, so frame t cannot start from frame t-1\'s '
                             'flow: warm_start needs forward (or submit / result) frame by frame')
        if self.frame is None:
            raise RuntimeError('forward_chunk: call forward() on the first frame of the sequence (it has no predecessor to pair with)')
        c = limgs.shape[0]
        prev = self.frame
        masks = masks.bool().contiguous()
        self.last_pose = self.last_pose.to(limgs.device)
        vec7, depth2, weights, flow, stereo_flow, cache, *q = self.model.infer_chunk(
            prev.img, limgs, rimgs, self.intrinsics, self.baseline * self.scale, depth0=prev.depth * self.scale, mask0=prev.mask,
            masks=masks, stereo_flow0=prev.flow, cache0=self._enc_cache, depth_roundtrip=self.scale, **self._quality_kw())
        self._set_quality(q[0] if q else None, c, limgs.device)
        self._enc_cache = cache if self.reuse_features else None
        rel, poses, ok = ops.pose_gate_chain(vec7.reshape(c, 7), self.last_pose.data, self._inv_scale, 1.0e-1)   # :81-91, every frame
        bad = ok == 0
        n_bad = int(bad.sum())                                             # the chunk's one host synchronisation
        _warn_skipped(n_bad)
        self.successes = ~bad
        self.success = not bool(bad[-1]) if n_bad else True
        self.last_rel_poses = rel
        self.last_rel_pose = SE3(rel[c - 1:])
        self.last_pose = SE3(poses[c - 1:])
        self.last_frame = Frame(limgs[c - 2:c - 1], rimgs[c - 2:c - 1]) if c > 1 else prev      # (only .img of it is ever read again)
        self.frame = Frame(limgs[c - 1:], rimgs[c - 1:], depth=depth2[c - 1:] / self.scale, mask=masks[c - 1:], flow=stereo_flow[c - 1:])
        return poses, None, flow, weights

    def get_pose_f2f(self, enc=None):
        flow = None
        self._low_pass = self._q_pass = None
        if self.last_frame is None:
            rel = SE3.IdentityLike(self.last_pose)
            depth, stereo_flow, valid, cache = self.model.flow2depth(self.frame.img, self.frame.rimg,
                                                                     self.baseline * self.scale, ret_cache=True, **({'enc': enc} if enc is not None else {}))
            self._enc_cache = cache if self.reuse_features else None
            self.frame.depth = depth / self.scale
            self.frame.flow = stereo_flow
            return rel, None, None, None
        p = self._pass(self.last_frame, self.frame.img, self.frame.rimg, self.frame.mask, self.intrinsics, self.baseline * self.scale,
                       cache1=self._enc_cache, ret_cache=True, **({'enc2': enc} if enc is not None and self._enc_cache is not None else {}),
                       **self._flow_init())
        self._q_pass, self._low_pass = p.quality, p.flow_low
        self._enc_cache = p.cache if self.reuse_features else None
        self.frame.depth = p.depth2 / self.scale
        self.frame.flow = p.stereo_flow
        return SE3(p.rel.data.reshape(1, 7)), self.last_frame, p.flow, p.weights


class SurfelPoseEstimator(PoseEstimator):
    """Frame-to-model tracker (``frame2frame: False``, configuration/infer_scared.yaml): every frame is tracked against a render of a
    fused surfel map (surfel_map.SurfelMap on the rpe_surfel_* kernels) at the last pose, following core/pose/pose_estimator.py:
    first frame -> stereo depth, ``mask &= valid``, map at last_pose (:56-65); every frame -> render at last_pose^-1 (transform_cpy +
    render in one launch), PoseNet.infer against it (:127-150), the gate and chain of PoseEstimator (one host synchronisation), and on
    success ``fuse(frame, last_pose)`` (:94-95).  Reads ``dist_thr`` and ``average_pts`` from the config.  Frames depend on the map the
    previous frame fused, so there is no chunked or pipelined form."""
    _f2m = True

    def __init__(self, config, intrinsics, baseline, checkpoint, img_shape, init_pose=None):
        if config.get('frame2frame', True):
            raise ValueError('SurfelPoseEstimator is frame-to-model tracking: it needs frame2frame: False (PoseEstimator tracks frame to frame)')
        super().__init__(config, intrinsics, baseline, checkpoint, img_shape, init_pose)
        self.scene = None

    def reset(self):
        super().reset()
        self.scene = None
        return self

    def submit(self, *a, **k):
        raise RuntimeError('SurfelPoseEstimator: frame t+1 is tracked against the map frame t fused, so frames cannot be pipelined')

    def forward_chunk(self, *a, **k):
        raise RuntimeError('SurfelPoseEstimator: frame t+1 is tracked against the map frame t fused, so frames cannot be chunked')

    @torch.no_grad()
    def forward(self, limg, rimg, mask):
        """limg, rimg: (1,3,h,w) 0..255; mask: (1,1,h,w) True = valid.  Returns (absolute pose SE3, the SurfelMap, flow, weights)."""
        from .surfel_map import SurfelMap
        self.last_pose = self.last_pose.to(limg.device)
        self.last_frame = self.frame
        self.frame = Frame(limg, rimg, mask=mask)
        if self.scene is None:                                             # :56-65
            depth, stereo_flow, valid = self.model.flow2depth(self.frame.img, self.frame.rimg, self.baseline * self.scale)
            self.frame.depth = depth / self.scale
            self.frame.mask &= valid
            self.frame.flow = stereo_flow
            self.scene = SurfelMap(frame=self.frame, kmat=self.intrinsics.squeeze(0), upscale=1, d_thresh=self.config['dist_thr'],
                                   pmat=self.last_pose, average_pts=self.config['average_pts'])
        rel_pose, ret_frame, flow, weights = self.get_pose_f2m()
        self._gate_and_chain(rel_pose, ret_frame)
        if self.success and flow is not None:                              # :94-95
            self.scene.fuse(self.frame, self.last_pose)
        return self.last_pose, self.scene, flow, weights

    def get_pose_f2m(self):
        """:127-150: the map rendered at the last camera pose, PoseNet.infer of render -> frame (mask2 &= valid in place)."""
        model_frame = self.scene.render_transformed(self.intrinsics.squeeze(0), self.last_pose.inv())[0]
        warm = self._flow_init()                                           # (warm start: the previous render -> frame flow, pushed forward)
        p = self._pass(model_frame, self.frame.img, self.frame.rimg, self.frame.mask, self.intrinsics, self.baseline * self.scale,
                       **(dict(warm, ret_cache=True) if warm else {}))
        self._q_pass, self._low_pass = p.quality, p.flow_low
        self.frame.depth = p.depth2 / self.scale
        self.frame.flow = p.stereo_flow
        model_frame.confidence = p.weights[0]
        return SE3(p.rel.data.reshape(1, 7)), model_frame, p.flow, p.weights


def _many_args(who, intrinsics, baselines, init_poses, max_seq, max_name):
    """The per-sequence constructor arguments of the lockstep trackers, checked: (intrinsics (K,3,3), baselines (K,), init_poses (K,7)
    tensor or None, K)."""
    intrinsics = torch.as_tensor(intrinsics)
    baselines = torch.as_tensor(baselines)
    if intrinsics.ndim != 3 or tuple(intrinsics.shape[1:]) != (3, 3):
        raise ValueError(f'{who}: intrinsics must be (K,3,3), got {tuple(intrinsics.shape)}')
    n = intrinsics.shape[0]
    if baselines.shape != (n,):
        raise ValueError(f'{who}: {n} intrinsics need baselines of shape ({n},), got {tuple(baselines.shape)}')
    if init_poses is not None:
        init_poses = (init_poses.data if hasattr(init_poses, 'data') and not isinstance(init_poses, torch.Tensor) else init_poses)
        if tuple(init_poses.shape) != (n, 7):
            raise ValueError(f'{who}: {n} sequences need init_poses of shape ({n}, 7), got {tuple(init_poses.shape)}')
    if not 1 <= n <= max_seq:
        raise ValueError(f'{who}: 1 to {max_seq} sequences ({max_name}), got {n}')
    return intrinsics, baselines, init_poses, n


def _many_rows(who, rows, n_seq, limgs, rimgs, masks):
    """``rows`` of a lockstep ``forward`` as a checked list (default: every sequence in order), one input row each."""
    rows = list(range(n_seq)) if rows is None else [int(k) for k in rows]
    R = len(rows)
    if R == 0 or len(set(rows)) != R or any(k < 0 or k >= n_seq for k in rows):
        raise ValueError(f'{who}.forward: rows must be distinct sequence indices in [0, {n_seq}), got {rows}')
    if limgs.shape[0] != R or rimgs.shape[0] != R or masks.shape[0] != R:
        raise ValueError(f'{who}.forward: {R} rows need {R} images and masks, got {limgs.shape[0]}, {rimgs.shape[0]}, {masks.shape[0]}')
    return rows


class MultiSurfelPoseEstimator(PoseEstimator):
    """K independent frame-to-model sequences advanced in lockstep (e.g. the (start, end) scenarios of the reference's
    scripts/benchmark_test.py): ``forward(limgs, rimgs, masks, rows)`` moves every listed sequence on by one frame with one batched
    network pass, one render and one fuse launch chain over all maps, and ONE host synchronisation for all success flags.  Sequence k
    gets bit for bit what a ``SurfelPoseEstimator`` fed its frames alone gets -- poses, success flags and map -- whichever rows share
    the batch: every kernel computes a row independently of its batch, the solve runs with ``partition_rows = 1`` (its launch-per-
    evaluation route when the rows do not all fit on the chip at once, bit-identical) and the map kernels are the single-map ones.
    intrinsics (K,3,3), baselines (K,), init_poses (K,7) (SE3 or tensor; default identity).  State per sequence: ``last_pose[k]``,
    ``success[k]``, ``scenes[k]`` (None until its first frame)."""
    _f2m = True

    def __init__(self, config, intrinsics, baselines, checkpoint, img_shape, init_poses=None):
        from ._lib import SURFEL_MAX_MAPS
        if config.get('frame2frame', True):
            raise ValueError('MultiSurfelPoseEstimator is frame-to-model tracking (frame2frame: False); frame-to-frame tracking already '
                             'batches the frames of one sequence: PoseEstimator.forward_chunk')
        intrinsics, baselines, init_poses, n = _many_args('MultiSurfelPoseEstimator', intrinsics, baselines, init_poses, SURFEL_MAX_MAPS,
                                                          'RPE_SURFEL_MAX_MAPS')
        super().__init__(config, intrinsics[0], 0.0, checkpoint, img_shape)
        self.intrinsics = intrinsics.float()                              # (K,3,3): the buffer PoseEstimator registered, per sequence
        self.baseline = baselines.float()                                 # (K,): torch.tensor(b).float() of each single tracker
        self.n_seq = n
        self._init_poses = None if init_poses is None else init_poses.float()
        self.reset()

    def _init_pose_of(self, k):
        return SE3.Identity(1) if self._init_poses is None else SE3(self._init_poses[k:k + 1])

    def reset(self, rows=None):
        """Forget sequences ``rows`` (default: all): each restarts at its initial pose with no map."""
        if rows is None:
            self.last_pose = [None] * self.n_seq
            self.success = [True] * self.n_seq
            self.scenes = [None] * self.n_seq
            self._flow_lows = [None] * self.n_seq                         # warm start: each sequence's last accepted temporal 1/8 flow
            rows = range(self.n_seq)
        for k in rows:
            self.last_pose[k] = self._init_pose_of(k)
            self.success[k] = True
            self.scenes[k] = None
            self._flow_lows[k] = None                                      # (warm start: the sequence's next pass is cold)
        return self

    def submit(self, *a, **k):
        raise RuntimeError('MultiSurfelPoseEstimator: frame t+1 is tracked against the map frame t fused, so frames cannot be pipelined')

    def forward_chunk(self, *a, **k):
        raise RuntimeError('MultiSurfelPoseEstimator: frame t+1 is tracked against the map frame t fused, so frames cannot be chunked; '
                           'it batches sequences instead (forward with rows=)')

    @torch.no_grad()
    def forward(self, limgs, rimgs, masks, rows=None):
        """One frame of each sequence in ``rows`` (default: all, in order): limgs, rimgs (R,3,h,w) 0..255, masks (R,1,h,w) True = valid,
        row j of the inputs belonging to sequence rows[j].  Returns (absolute poses SE3 (R,7), success (R,) bool on the host, the R
        maps, flow (R,2,h,w), weights)."""
        from . import surfel_map
        rows = _many_rows('MultiSurfelPoseEstimator', rows, self.n_seq, limgs, rimgs, masks)
        R = len(rows)
        dev = limgs.device
        limgs, rimgs = limgs.contiguous(), rimgs.contiguous()
        masks = masks.bool()                                               # (a bool mask is the caller's tensor, as Frame keeps it)
        for k in rows:
            self.last_pose[k] = self.last_pose[k].to(dev)
        every = rows == list(range(self.n_seq))                            # (device slices, not an index tensor: no blocking host copy)
        K = self.intrinsics if every else torch.cat([self.intrinsics[k:k + 1] for k in rows])
        baseline = (self.baseline if every else torch.cat([self.baseline[k:k + 1] for k in rows])) * self.scale
        new = [j for j, k in enumerate(rows) if self.scenes[k] is None]
        if new:                                                            # :56-65 for every sequence that starts here
            sub = new if len(new) < R else None
            pick = (lambda t: torch.cat([t[j:j + 1] for j in sub])) if sub is not None else (lambda t: t)
            depth, stereo_flow, valid = self.model.flow2depth(pick(limgs), pick(rimgs), pick(baseline))
            if sub is None:
                masks &= valid
                m_new = masks
            else:
                m_new = pick(masks) & valid
                for i, j in enumerate(sub):
                    masks[j:j + 1] = m_new[i:i + 1]
            pm = torch.cat([self.last_pose[rows[j]].data.reshape(1, 7) for j in new])
            maps = surfel_map.init_many(Frame(pick(limgs), pick(rimgs), depth=depth / self.scale, mask=m_new), pick(K), pm, upscale=1,
                                        d_thresh=self.config['dist_thr'], average_pts=self.config['average_pts'])
            for j, m in zip(new, maps):
                self.scenes[rows[j]] = m
        # :127-150 for every row: the maps rendered at the last camera poses, straight into the network's input rows
        last = torch.cat([self.last_pose[k].data.reshape(1, 7) for k in rows])
        model = surfel_map.render_many([self.scenes[k] for k in rows], K, ops.se3_inv(last))
        warm = {}
        if self.warm_start:
            # per sequence: forward_interpolate of its last accepted render -> frame flow, or zeros (= the cold pass, bit for bit) for a
            # sequence without one; one launch over the R rows (a row's result does not depend on its batch)
            prev = [self._flow_lows[k] for k in rows]
            have = [p for p in prev if p is not None]
            warm['ret_lowres'], warm['ret_cache'] = True, True
            if have:
                zero = torch.zeros_like(have[0])
                warm['flow_init'] = ops.forward_interpolate(torch.cat([zero if p is None else p for p in prev]))
        p = self._pass(model, limgs, rimgs, masks, K, baseline, rows_alone=True, **warm)   # (a row's solve as if alone, as PoseNet.infer_chunk)
        rel_g, pose, ok = ops.pose_gate_chain_rows(p.rel.data.reshape(R, 7), last, self._inv_scale, 1.0e-1)     # :81-91, row by row
        if self.report_quality:
            self._set_quality(p.quality, R, dev)                           # row j belongs to sequence rows[j]
        self.t_enqueued = time.perf_counter()
        okh = ok.cpu().bool()                                              # the lockstep frame's one host synchronisation
        _warn_skipped(R - int(okh.sum()))
        for j, k in enumerate(rows):
            self.success[k] = bool(okh[j])
            self.last_pose[k] = SE3(pose[j:j + 1])
            if warm:
                self._flow_lows[k] = p.flow_low[j:j + 1] if self.success[k] else None
        self.last_rel_poses = rel_g
        passed = [j for j in range(R) if okh[j]]
        if passed:                                                         # :94-95
            surfel_map.fuse_many([self.scenes[rows[j]] for j in passed], Frame(limgs, rimgs, depth=p.depth2 / self.scale, mask=masks),
                                 pose, rows=passed)
        return SE3(pose), okh, [self.scenes[k] for k in rows], p.flow, p.weights


MULTI_MAX_SEQUENCES = 64            # (MultiSurfelPoseEstimator's bound, RPE_SURFEL_MAX_MAPS: from_config_many takes the same K in either mode)


def _stack_rows(parts):
    """Rows ``(tensor, j)`` as one batch: the tensor itself when they are exactly its rows in order (the lockstep steady state: no copy),
    else device slices concatenated (no index tensor, so no blocking host copy)."""
    t0 = parts[0][0]
    if t0.shape[0] == len(parts) and all(t is t0 and j == i for i, (t, j) in enumerate(parts)):
        return t0
    return torch.cat([t[j:j + 1] for t, j in parts])


class MultiPoseEstimator(PoseEstimator):
    """K independent frame-to-frame sequences advanced in lockstep, frames arriving one at a time per sequence (K live feeds, or the
    (start, end) scenarios of the reference's scripts/benchmark_test.py): ``forward(limgs, rimgs, masks, rows)`` moves every listed
    sequence on by one frame with ONE RAFT pass over the 2 R' pairs of the R' rows that have a previous frame, one ``flow2depth`` for the
    rows that do not (both kinds may share a call), one solve (``rows_alone=True``), one ``ops.pose_gate_chain_rows`` and ONE host
    synchronisation for all success flags.  Sequence k gets bit for bit what a ``PoseEstimator`` fed its frames alone gets -- poses,
    success flags, flow, ``last_quality`` rows -- whichever rows share the call: every kernel computes a row independently of its batch
    and the solve runs with ``partition_rows = 1``.  Honours ``warm_start`` (per row; a row without a kept flow starts from zeros, which
    is the cold pass bit for bit), ``report_quality`` (row j of ``last_quality`` belongs to sequence rows[j]) and ``reuse_features``.
    intrinsics (K,3,3), baselines (K,), init_poses (K,7) (SE3 or tensor; default identity).  State per sequence: ``last_pose[k]``,
    ``success[k]``, and its last frame (image, depth, mask, stereo flow, encoder outputs) and kept 1/8 flow as a row of the batch
    that produced them, so a lockstep step over the same rows as the last one builds its inputs without a copy."""

    def __init__(self, config, intrinsics, baselines, checkpoint, img_shape, init_poses=None):
        if not config.get('frame2frame', True):
            raise ValueError('MultiPoseEstimator is frame-to-frame tracking (frame2frame: True); several frame-to-model sequences are '
                             'MultiSurfelPoseEstimator (or from_config_many)')
        intrinsics, baselines, init_poses, n = _many_args('MultiPoseEstimator', intrinsics, baselines, init_poses, MULTI_MAX_SEQUENCES,
                                                          'MULTI_MAX_SEQUENCES')
        super().__init__(config, intrinsics[0], 0.0, checkpoint, img_shape)
        self.intrinsics = intrinsics.float()                              # (K,3,3): the buffer PoseEstimator registered, per sequence
        self.baseline = baselines.float()                                 # (K,): torch.tensor(b).float() of each single tracker
        self.n_seq = n
        self._init_poses = None if init_poses is None else init_poses.float()
        self.reset()

    def _init_pose_of(self, k):
        return SE3.Identity(1) if self._init_poses is None else SE3(self._init_poses[k:k + 1])

    def reset(self, rows=None):
        """Forget sequences ``rows`` (default: all): each restarts at its initial pose, its next frame is a first frame again."""
        if rows is None:
            self.last_pose = [None] * self.n_seq
            self.success = [True] * self.n_seq
            self._prev = [None] * self.n_seq                              # (the batch dict that holds the sequence's last frame, its row)
            self._flow_lows = [None] * self.n_seq                         # warm start: (a pass's temporal 1/8 flows, the sequence's row)
            self.last_quality = None
            rows = range(self.n_seq)
        for k in rows:
            self.last_pose[k] = self._init_pose_of(k)
            self.success[k] = True
            self._prev[k] = None
            self._flow_lows[k] = None
        return self

    def submit(self, *a, **k):
        raise RuntimeError('MultiPoseEstimator: submit / result hide ONE sequence\'s encoders behind its previous frame; here the frames '
                           'of K sequences share each pass, so they cannot be pipelined as well (forward with rows=)')

    def forward_chunk(self, *a, **k):
        raise RuntimeError('MultiPoseEstimator: forward_chunk batches frames of ONE sequence that are already known, so frames cannot be '
                           'chunked here; it batches sequences instead (forward with rows=)')

    def _warm_rows(self, seqs):
        """``_flow_init`` for the tracked sequences ``seqs`` of a call: one forward_interpolate launch over their kept 1/8 flows, zeros for
        a sequence without one; no flow_init at all (the cold pass) when none has one."""
        if not self.warm_start:
            return {}
        lows = [self._flow_lows[k] for k in seqs]
        have = [x for x in lows if x is not None]
        if not have:
            return dict(ret_lowres=True)
        zero = (torch.zeros_like(have[0][0][:1]), 0)
        return dict(ret_lowres=True, flow_init=ops.forward_interpolate(_stack_rows([zero if x is None else x for x in lows])))

    @torch.no_grad()
    def forward(self, limgs, rimgs, masks, rows=None):
        """One frame of each sequence in ``rows`` (default: all, in order): limgs, rimgs (R,3,h,w) 0..255, masks (R,1,h,w) True = valid,
        row j of the inputs belonging to sequence rows[j].  Returns (absolute poses SE3 (R,7), success (R,) bool on the host, flow
        (R,2,h,w), weights (w2d, w3d) each (R,1,h,w)).  A row on its sequence's first frame has nothing to be tracked against: it returns
        the sequence's initial pose and success True, its rows of flow and weights are ZEROS (PoseEstimator returns None there) and its
        ``last_quality`` row is the report of a frame without a solve.  A row the gate rejects keeps its pose, and its frame becomes the
        sequence's next reference, as in PoseEstimator."""
        rows = _many_rows('MultiPoseEstimator', rows, self.n_seq, limgs, rimgs, masks)
        R = len(rows)
        dev = limgs.device
        limgs, rimgs = limgs.contiguous(), rimgs.contiguous()
        masks = masks.bool()                                               # (a bool mask is the caller's tensor, as Frame keeps it)
        for k in rows:
            self.last_pose[k] = self.last_pose[k].to(dev)
        every = rows == list(range(self.n_seq))                            # (device slices, not an index tensor: no blocking host copy)
        K = self.intrinsics if every else torch.cat([self.intrinsics[k:k + 1] for k in rows])
        baseline = (self.baseline if every else torch.cat([self.baseline[k:k + 1] for k in rows])) * self.scale
        tracked = [j for j in range(R) if self._prev[rows[j]] is not None]
        new = [j for j in range(R) if self._prev[rows[j]] is None]
        at = {j: i for i, j in enumerate(tracked)}                         # input row -> row of the pass

        def pick(t, idx):
            return t if len(idx) == R else torch.cat([t[j:j + 1] for j in idx])

        def merge(t, fill):
            """(R, ...) in input-row order from the pass's rows ``t`` and ``fill`` (1, ...) for every first-frame row."""
            if not new:
                return t
            return torch.cat([t[at[j]:at[j] + 1] if j in at else fill for j in range(R)])
        if new:                                                            # first frames: stereo depth only (get_pose_f2f)
            l, r = pick(limgs, new), pick(rimgs, new)
            depth, stereo_flow, _, cache = self.model.flow2depth(l, r, pick(baseline, new), ret_cache=True)
            first = dict(img=l, depth=depth / self.scale, mask=pick(masks, new), flow=stereo_flow, fmap=cache['fmap'], cnet=cache['cnet'])
        p = None
        if tracked:                                                        # every other row: previous frame -> frame, one pass
            prev = [self._prev[rows[j]] for j in tracked]
            f1 = SimpleNamespace(**{name: _stack_rows([(b[name], i) for b, i in prev]) for name in ('img', 'depth', 'mask', 'flow')})
            cache1 = {name: _stack_rows([(b[name], i) for b, i in prev]) for name in ('fmap', 'cnet')} if self.reuse_features else None
            l, r, m = pick(limgs, tracked), pick(rimgs, tracked), pick(masks, tracked)
            p = self._pass(f1, l, r, m, pick(K, tracked), pick(baseline, tracked), cache1=cache1, ret_cache=True, rows_alone=True,
                           **self._warm_rows([rows[j] for j in tracked]))
            if new:
                for j, i in at.items():
                    masks[j:j + 1] = m[i:i + 1]                            # (`mask2 &= valid` reaches the caller's tensor, as in PoseEstimator)
            cur = dict(img=l, depth=p.depth2 / self.scale, mask=m, flow=p.stereo_flow, fmap=p.cache['fmap'], cnet=p.cache['cnet'])
        # :81-91, row by row; a first-frame row chains the identity onto its initial pose, as PoseEstimator.forward does
        last = torch.cat([self.last_pose[k].data.reshape(1, 7) for k in rows])
        rel = merge(p.rel.data.reshape(-1, 7) if tracked else None, SE3.Identity(1, device=dev).data if new else None)
        rel_g, pose, ok = ops.pose_gate_chain_rows(rel, last, self._inv_scale, 1.0e-1)
        if self.report_quality:                                            # row j belongs to sequence rows[j]; also filled for a rejected row
            q = denormalise_quality(p.quality, self._inv_scale) if tracked else None
            blank = blank_quality(1, dev) if new else None
            self.last_quality = {key: merge(q[key] if tracked else None, blank[key] if new else None) for key in (q or blank)}
        zeros = (lambda c: torch.zeros((1, c, *limgs.shape[-2:]), device=dev)) if new else (lambda c: None)
        flow = merge(p.flow if tracked else None, zeros(2))
        weights = tuple(merge(p.weights[i] if tracked else None, zeros(1)) for i in range(2))
        self.t_enqueued = time.perf_counter()
        okh = ok.cpu().bool()                                              # the lockstep frame's one host synchronisation
        _warn_skipped(R - int(okh.sum()))
        for j, k in enumerate(rows):
            self.success[k] = bool(okh[j])
            self.last_pose[k] = SE3(pose[j:j + 1])
            self._prev[k] = (cur, at[j]) if j in at else (first, new.index(j))
            if self.warm_start:                                            # (a rejected frame: the next pair spans two frames, start it cold)
                self._flow_lows[k] = (p.flow_low, at[j]) if j in at and self.success[k] else None
        self.last_rel_poses = rel_g
        return SE3(pose), okh, flow, weights


def from_config_many(config, intrinsics, baselines, checkpoint, img_shape, init_poses=None):
    """``from_config`` for K sequences in lockstep (intrinsics (K,3,3), baselines (K,), init_poses (K,7) or None): MultiPoseEstimator for
    frame2frame True, MultiSurfelPoseEstimator for False."""
    cls = MultiPoseEstimator if config.get('frame2frame', True) else MultiSurfelPoseEstimator
    return cls(config, intrinsics, baselines, checkpoint, img_shape, init_poses)


def from_config(config, intrinsics, baseline, checkpoint, img_shape, init_pose=None):
    """The tracker the config asks for (scripts/infer_trajectory.py:50-51): PoseEstimator for frame2frame True, SurfelPoseEstimator for False."""
    cls = PoseEstimator if config.get('frame2frame', True) else SurfelPoseEstimator
    return cls(config, intrinsics, baseline, checkpoint, img_shape, init_pose)
