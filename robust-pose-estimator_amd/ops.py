"""Tensor-level wrappers of the C ABI (include/rpe.h): argument checking, output allocation from torch's
caching allocator, and launch on torch's current HIP stream.  PyTorch is plumbing here (device memory and
streams); every operation below runs in librpe_hip.so.  Tensors must live on a ROCm device -- there is no
CPU path."""
import ctypes
import operator

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

SOLVER_LBFGS, SOLVER_GN = 0, 1


class OpList:
    """A prepared launch list for rpe_run_ops (include/rpe.h): the launches of a host loop -- RAFT.forward's update iterations, core/RAFT/
    core/raft.py -- enqueued by ONE call into the library instead of one Python-dispatched call each.  Built from the ``prepare=True``
    launchers of this module (their ``.op`` = (RPE_OP_* kind, argument struct)); every op runs through the same public entry point with
    the same arguments as the launcher would, so results are bit-identical to launching them one by one.  ``stream`` indexes the
    stream tuple given to run().  Event cells: cell(i) is a void* slot holding a raw hipEvent_t handle (0 = the op is skipped)."""

    def __init__(self, n_cells=0):
        self._items, self._keep, self._arr = [], [], None
        self.cells = (ctypes.c_void_p * max(1, n_cells))()
        self._streams = (ctypes.c_void_p * 4)()
        self._failed = ctypes.c_int(-1)

    def __len__(self):
        return len(self._items)

    def add(self, launcher, stream=0):
        kind, args = launcher.op
        self._items.append((kind, stream, ctypes.addressof(args)))
        self._keep.append(launcher)                       # (the launcher keeps the struct and every tensor it points to alive)
        self._arr = None
        return self

    def _cell_op(self, kind, cell, stream):
        self._items.append((kind, stream, ctypes.addressof(self.cells) + ctypes.sizeof(ctypes.c_void_p) * cell))
        self._arr = None
        return self

    def record(self, cell, stream=0):
        return self._cell_op(_lib.OP_EVENT_RECORD, cell, stream)

    def wait(self, cell, stream=0):
        return self._cell_op(_lib.OP_STREAM_WAIT, cell, stream)

    def mark(self):
        """Index of the next op: run(start, stop) takes such marks (a caller that needs the state between iterations runs slices)."""
        return len(self._items)

    def run(self, streams, start=0, stop=None):
        """Enqueue ops [start, stop) on ``streams`` (raw hipStream_t handles as ints, index = the ops' ``stream``)."""
        if self._arr is None:
            self._arr = (_lib.Op * max(1, len(self._items)))(*[_lib.Op(k, s, a) for k, s, a in self._items])
        stop = len(self._items) if stop is None else stop
        if stop <= start:
            return
        for i, h in enumerate(streams):
            self._streams[i] = h
        st = lib().rpe_run_ops(ctypes.cast(ctypes.byref(self._arr, ctypes.sizeof(_lib.Op) * start), ctypes.POINTER(_lib.Op)), stop - start, self._streams,
                               len(streams), ctypes.byref(self._failed))
        if st != 0:
            check(st, f'rpe_run_ops (op {start + self._failed.value} of the list, kind {self._items[start + self._failed.value][0]})')


_REC = None          # the active Recorder (one host thread drives one GPU)


class Recorder(OpList):
    """An OpList filled by RUNNING a piece of host code once: inside ``with recorder:`` every wrapper of this module that a launch list
    can carry (the convolutions, stems, instance-norm passes, plane copies, the correlation build, the convex up-sampling) launches as
    usual AND logs its argument block -- so the recording pass is an ordinary pass with an ordinary result.  Every tensor a logged
    launch touches is kept alive by the recorder: the intermediates of the pass become the list's private workspace, at fixed addresses.
    ``bind(name, tensor)`` then marks a tensor of the pass as an external input / output: replay({name: new_tensor, ...}) rewrites every
    pointer of the list that points into it (base + the same offset: channel / batch slices stay slices) and enqueues the whole list
    with one rpe_run_ops call on the current stream.  The caller guarantees what the list cannot see: same shapes and dtypes, same
    weights, replays on the stream it was recorded on (the workspace is reused without synchronisation)."""

    def __init__(self):
        super().__init__()
        self._structs, self._bound, self._claimed = [], {}, set()
        self.complete = False         # set when the pass has ended and every library launch of it was logged

    def __enter__(self):
        global _REC
        if _REC is not None:
            raise _lib.RpeError('Recorder: recordings do not nest')
        self._count = _lib.CountingLib().__enter__()
        _REC = self
        return self

    def __exit__(self, *exc):
        global _REC
        _REC = None
        self._count.__exit__(*exc)
        # a launch that went to the library without being logged (a wrapper this class does not know, a fallback route) would be
        # missing from every replay: such a recording is not usable, and the caller keeps launching the pass call by call
        self.complete = exc[0] is None and self._count.calls == len(self._items)
        self.unlogged = [] if self.complete else sorted(set(self._count.names))
        del self._count
        return False

    def log(self, kind, args, keep):
        self._items.append((kind, 0, ctypes.addressof(args)))
        self._keep.append((args, keep))
        self._structs.append(args)
        self._arr = None

    def bind(self, name, t):
        """Every pointer field of the logged argument blocks that points into ``t``'s memory -> (struct, field, offset)."""
        lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
        sites = []
        for i, st in enumerate(self._structs):
            for fname, ftype in _lib.struct_fields(st):
                if ftype is ctypes.c_void_p and (i, fname) not in self._claimed:
                    v = getattr(st, fname)
                    if v is not None and lo <= v < hi:
                        sites.append((st, fname, v - lo))
                        self._claimed.add((i, fname))
        self._bound[name] = (sites, tuple(t.shape), t.dtype, t.device)
        return len(sites)

    def patch(self, tensors):
        """Rewrite every pointer bound to ``name`` for the tensors given (same shape, dtype and device as at recording time, contiguous)."""
        for name, t in tensors.items():
            sites, shape, dtype, device = self._bound[name]
            if tuple(t.shape) != shape or t.dtype != dtype or t.device != device or not t.is_contiguous():
                raise _lib.RpeError(f'Recorder.replay: {name} must be a contiguous {dtype} tensor of shape {shape} on {device}')
            base = t.data_ptr()
            for st, fname, off in sites:
                setattr(st, fname, base + off)

    def replay(self, tensors):
        self.patch(tensors)
        self.run((raw_stream(),))


def raw_stream(stream=None):
    """The raw hipStream_t handle (int) of a torch stream (default: the current stream of the current device)."""
    return _lib.stream_ptr().value or 0 if stream is None else stream.cuda_stream


class _Launcher:
    """A prepared launch (``prepare=True``): calling it runs the entry point on the current stream with the CURRENT fields of its argument
    struct, so a struct that Recorder.patch rewrote is seen here as in a launch list.  ``.op`` = (kind, struct) for OpList.add; ``.keep``
    = what the struct points into.  ``L`` is the library whose entry point it calls."""

    def __init__(self, kind, a, keep, result, L):
        entry, struct = _lib.ALL_LIST_OPS[kind]
        self.op, self.keep, self._result, self._entry, self._fn = (kind, a), keep, result, entry, getattr(L, entry)
        self._args = (lambda d, ref=ctypes.byref(a): (ref,)) if struct is _lib.ConvDesc else operator.attrgetter(*(f for f, _ in struct._fields_))

    def __call__(self):
        kind, a = self.op
        if _REC is not None:
            _REC.log(kind, a, self.keep)
        st = self._fn(*self._args(a), stream_ptr())
        if st != 0:
            check(st, self._entry)
        return self._result


def _launch(kind, args, keep, result, prepare=False):
    """The launch policy of every wrapper a launch list can carry.  ``args``: the entry point's arguments without the stream, in the order
    of its argument struct (the descriptor itself for the rpe_conv_desc kinds); ``keep``: the objects they point into.  Launches on the
    current stream and returns ``result``, or (``prepare``) returns a _Launcher on the real library -- never on a CountingLib that stands
    in while it is built.  While a Recorder is active, every launch is logged with its struct."""
    entry, struct = _lib.ALL_LIST_OPS[kind]
    desc = struct is _lib.ConvDesc
    if not prepare and _REC is None:                  # call by call: no struct beyond the descriptor the wrapper built anyway
        st = getattr(lib(), entry)(*((ctypes.byref(args),) if desc else args), stream_ptr())
        if st != 0:
            check(st, entry)
        return result
    launch = _Launcher(kind, args if desc else struct(*args), keep, result, _lib.real_lib() if prepare else lib())
    return launch if prepare else launch()


_DT = {torch.float32: 0, torch.float64: 1}


def _on_current_device(t, name):
    """Kernels are enqueued on the CURRENT device's stream: a tensor of another GPU would be written through a foreign
    pointer.  One process drives one GPU here (torch.cuda.set_device(LOCAL_RANK)); anything else is refused."""
    if t.device.index != torch.cuda.current_device():
        raise _lib.RpeError(f'{name}: tensor lives on {t.device} but the current device is cuda:{torch.cuda.current_device()} '
                            '(call torch.cuda.set_device first; multi-device use from one process is unsupported)')


def _dev(t, dtype=None, name='tensor'):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.RpeError(f'{name}: expected a tensor on the GPU (the HIP path has no CPU fallback)')
    _on_current_device(t, name)
    if dtype is not None and t.dtype != dtype:
        raise _lib.RpeError(f'{name}: expected dtype {dtype}, got {t.dtype}')
    return t if t.is_contiguous() else t.contiguous()


def _is_f32(t, shape=None, numel=None):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() \
        and (shape is None or tuple(t.shape) == tuple(shape)) and (numel is None or t.numel() == numel)


def _f32(t, name, shape=None, numel=None):
    """``t`` if it is a contiguous float32 GPU tensor [of this shape / of this many elements]; ``name`` = 'wrapper: argument'."""
    if not _is_f32(t, shape, numel):
        what = f' of shape {tuple(shape)}' if shape is not None else f' of {numel} elements' if numel is not None else ''
        raise _lib.RpeError(f'{name} must be a contiguous float32 GPU tensor{what}')
    return t


def bounded_put(cache, key, value, keep=2):
    """Insert into a small insertion-ordered cache, evicting the oldest entries (and the buffers / launch descriptors they pin)."""
    while len(cache) >= keep:
        cache.pop(next(iter(cache)))
    cache[key] = value


def wkey(*tensors):
    """Cache key of what is made from ``tensors`` (None = absent, and stays None in its place): an in-place update bumps the version,
    .to() / .float() move the data, and a replaced Parameter is another tensor."""
    return tuple(None if t is None else (t._version, t.data_ptr()) for t in tensors)


def _mask(t, name):
    t = _dev(t, None, name)
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    if t.dtype == torch.uint8:
        return t
    raise _lib.RpeError(f'{name}: expected bool/uint8 mask')


# ------------------------------------------------------------------------------------------------- SE(3)
def _se3_unary(fn, x, din, dout):
    x = _dev(x, None, 'se3 input')
    if x.dtype not in _DT or x.shape[-1] != din:
        raise _lib.RpeError('se3: bad dtype/shape')
    out = torch.empty(*x.shape[:-1], dout, dtype=x.dtype, device=x.device)
    n = x.numel() // din
    check(fn(ptr(x), ptr(out), n, _DT[x.dtype], stream_ptr()), 'rpe_se3')
    return out


def se3_exp(xi):
    return _se3_unary(lib().rpe_se3_exp, xi, 6, 7)


def se3_log(T):
    return _se3_unary(lib().rpe_se3_log, T, 7, 6)


def se3_inv(T):
    return _se3_unary(lib().rpe_se3_inv, T, 7, 7)


def se3_mul(A, B):
    A, B = torch.broadcast_tensors(A, B)
    A, B = _dev(A, None, 'A'), _dev(B, A.dtype, 'B')
    out = torch.empty_like(A)
    check(lib().rpe_se3_mul(ptr(A), ptr(B), ptr(out), A.numel() // 7, _DT[A.dtype], stream_ptr()), 'rpe_se3_mul')
    return out


def se3_act(T, pts):
    """T (n,7) or (n,1,7) acting on pts (n,m,3)."""
    pts = _dev(pts, None, 'pts')
    n, m = pts.shape[0], pts.shape[1]
    T = _dev(T.reshape(n, 7), pts.dtype, 'T')
    out = torch.empty_like(pts)
    check(lib().rpe_se3_act(ptr(T), ptr(pts), ptr(out), n, m, _DT[pts.dtype], stream_ptr()), 'rpe_se3_act')
    return out


def se3_chain(rel, scale=1.0, init=None):
    rel = _dev(rel.reshape(-1, 7), None, 'rel')
    init = _dev(init.reshape(7), rel.dtype, 'init') if init is not None else None
    out = torch.empty_like(rel)
    check(lib().rpe_se3_chain(ptr(rel), ptr(init), ptr(out), rel.shape[0], float(scale), _DT[rel.dtype], stream_ptr()),
          'rpe_se3_chain')
    return out


def pose_gate_chain(rel, init, scale, thr=0.1):
    """rpe_pose_gate_chain: PoseEstimator's failure gate and pose chaining for m relative poses (m,7) in one launch.
    Returns (gated relative poses (m,7), absolute poses (m,7), ok (m,) int32)."""
    rel = _dev(rel.reshape(-1, 7), None, 'rel')
    init = _dev(init.reshape(7), rel.dtype, 'init') if init is not None else None
    rel_out, abs_out = torch.empty_like(rel), torch.empty_like(rel)
    ok = torch.empty(rel.shape[0], dtype=torch.int32, device=rel.device)
    check(lib().rpe_pose_gate_chain(ptr(rel), ptr(init), ptr(rel_out), ptr(abs_out), ptr(ok), rel.shape[0], float(scale), float(thr),
                                    _DT[rel.dtype], stream_ptr()), 'rpe_pose_gate_chain')
    return rel_out, abs_out, ok


def pose_gate_chain_rows(rel, init, scale, thr=0.1):
    """rpe_pose_gate_chain_rows: the gate and chain of ``pose_gate_chain`` for m independent sequences in one launch, row k of rel (m,7)
    onto row k of init (m,7).  Row k's bits are those of ``pose_gate_chain(rel[k], init[k], ...)``.  Returns (rel_out, abs_out, ok)."""
    rel = _dev(rel.reshape(-1, 7), None, 'rel')
    init = _dev(init.reshape(-1, 7), rel.dtype, 'init') if init is not None else None
    if init is not None and init.shape[0] != rel.shape[0]:
        raise _lib.RpeError(f'pose_gate_chain_rows: {rel.shape[0]} relative poses, {init.shape[0]} initial poses')
    rel_out, abs_out = torch.empty_like(rel), torch.empty_like(rel)
    ok = torch.empty(rel.shape[0], dtype=torch.int32, device=rel.device)
    check(lib().rpe_pose_gate_chain_rows(ptr(rel), ptr(init), ptr(rel_out), ptr(abs_out), ptr(ok), rel.shape[0], float(scale), float(thr),
                                         _DT[rel.dtype], stream_ptr()), 'rpe_pose_gate_chain_rows')
    return rel_out, abs_out, ok


# ------------------------------------------------------------------------------------------------- pose layer
def _pose_inputs(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight):
    f32 = torch.float32
    flow = _dev(flow, f32, 'flow')
    n, _, h, w = flow.shape
    pcl1, pcl2 = _dev(pcl1, f32, 'pcl1'), _dev(pcl2, f32, 'pcl2')
    w1, w2 = _dev(w1, f32, 'w1'), _dev(w2, f32, 'w2')
    mask1, mask2 = _mask(mask1, 'mask1'), _mask(mask2, 'mask2')
    K = _dev(K, f32, 'K')
    lw = _dev(loss_weight, f32, 'loss_weight')
    for t, c in ((pcl1, 3), (pcl2, 3), (w1, 1), (w2, 1), (mask1, 1), (mask2, 1)):
        if tuple(t.shape) != (n, c, h, w):
            raise _lib.RpeError(f'pose layer: shape {tuple(t.shape)} != {(n, c, h, w)}')
    if tuple(K.shape) != (n, 3, 3) or tuple(lw.shape) != (n, 2):
        raise _lib.RpeError('pose layer: K must be (n,3,3) and loss_weight (n,2)')
    return (flow, pcl1, pcl2, w1, w2, mask1, mask2, K, lw), n, h, w


def _workspace(n, h, w, device):
    return torch.empty(lib().rpe_pose_workspace_bytes(n, h, w), dtype=torch.uint8, device=device)


def pose_reduce(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight, T, need_hessian=False):
    """One objective evaluation at T (n,7) f64 -> dict(loss2d, loss3d, f, g (n,6), H (n,6,6))."""
    args, n, h, w = _pose_inputs(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight)
    T = _dev(T.reshape(n, 7), torch.float64, 'T')
    out = torch.empty(n, 32, dtype=torch.float64, device=T.device)
    ws = _workspace(n, h, w, T.device)
    check(lib().rpe_pose_reduce(*[ptr(a) for a in args], ptr(T), n, h, w, int(bool(need_hessian)), ptr(out), ptr(ws),
                                stream_ptr()), 'rpe_pose_reduce')
    res = dict(loss2d=out[:, 0], loss3d=out[:, 1], f=out[:, 2], g=out[:, 3:9])
    if need_hessian:
        iu = torch.triu_indices(6, 6, device=T.device)
        H = torch.zeros(n, 6, 6, dtype=torch.float64, device=T.device)
        H[:, iu[0], iu[1]] = out[:, 9:30]
        H = H + H.transpose(1, 2) - torch.diag_embed(torch.diagonal(H, dim1=1, dim2=2))
        res['H'] = H
    return res


def pose_solve(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight, iters, mode=SOLVER_LBFGS,
               tolerance_grad=1e-7, tolerance_change=1e-9, history_size=100, partition_rows=0, persistent=True):
    """Device-resident solve.  Returns (T f64 (n,7), vec7 f32 (n,7), log6 f32 (n,6), info int32 (n,4)).
    ``partition_rows=1``: every row's float64 sums are grouped as if it were solved alone (rpe_solve_opts), i.e. the result of a
    row does not depend on the batch it is in, bit for bit.  ``persistent=False`` (RPE_SOLVE_LAUNCH_PER_EVALUATION): one launch per
    evaluation instead of one for the whole solve -- the same bits, for A/B measurements, and for several solves at once whose grids
    together exceed the device (include/rpe.h, rpe_solve_opts: concurrent one-launch solves can starve each other)."""
    args, n, h, w = _pose_inputs(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight)
    dev = args[0].device
    T = torch.empty(n, 7, dtype=torch.float64, device=dev)
    vec7 = torch.empty(n, 7, dtype=torch.float32, device=dev)
    log6 = torch.empty(n, 6, dtype=torch.float32, device=dev)
    info = torch.empty(n, 4, dtype=torch.int32, device=dev)
    ws = _workspace(n, h, w, dev)
    o = _lib.SolveOpts(ctypes.sizeof(_lib.SolveOpts), int(history_size), float(tolerance_grad), float(tolerance_change), int(partition_rows),
                       0 if persistent else 1)
    check(lib().rpe_pose_solve_ex(*[ptr(a) for a in args], n, h, w, int(mode), int(iters), ctypes.byref(o), ptr(T), ptr(vec7), ptr(log6),
                                  ptr(info), ptr(ws), stream_ptr()), 'rpe_pose_solve_ex')
    return T, vec7, log6, info


QUALITY_SLOTS = 64


def pose_quality(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight, T):
    """rpe_pose_quality: the solve-quality report at T (n,7) f64 -> (n,64) f64 (slot table: include/rpe.h; ``quality_fields`` names
    them).  Two launches on the current stream, no host synchronisation; a row's slots do not depend on its batch, bit for bit."""
    args, n, h, w = _pose_inputs(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight)
    T = _dev(T.reshape(n, 7), torch.float64, 'T')
    out = torch.empty(n, QUALITY_SLOTS, dtype=torch.float64, device=T.device)
    ws = torch.empty(lib().rpe_pose_quality_workspace_bytes(n, h, w), dtype=torch.uint8, device=T.device)
    check(lib().rpe_pose_quality(*[ptr(a) for a in args], ptr(T), n, h, w, ptr(out), ptr(ws), stream_ptr()), 'rpe_pose_quality')
    return out


def quality_fields(out):
    """Named views of rpe_pose_quality's (n,64) rows: cov (n,6,6), pd, n2d, n3d, sum_w1, sum_w2, sse2d, sse3d, rms2d_px, rms3d, f,
    grad_max, g (n,6), m.  Views only: works on the device and on the host, copies nothing."""
    return dict(cov=out[:, 16:52].reshape(-1, 6, 6), pd=out[:, 52], n2d=out[:, 0], n3d=out[:, 1], sum_w1=out[:, 2], sum_w2=out[:, 3],
                sse2d=out[:, 4], sse3d=out[:, 5], rms2d_px=out[:, 6], rms3d=out[:, 7], f=out[:, 8], grad_max=out[:, 9], g=out[:, 10:16],
                m=out[:, 53])


def pose_backward_moments(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight, T):
    """At pose T (n,7) f64: (g2u (n,6), g3u (n,6), H (n,6,6)) -- unit-loss-weight tangent gradients of the two terms
    and the symmetrised fYY of the reference's backward (declerative_node_lie.py:40-51)."""
    args, n, h, w = _pose_inputs(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight)
    T = _dev(T.reshape(n, 7), torch.float64, 'T')
    out = torch.empty(n, 48, dtype=torch.float64, device=T.device)
    ws = torch.empty(lib().rpe_pose_backward_workspace_bytes(n, h, w), dtype=torch.uint8, device=T.device)
    check(lib().rpe_pose_backward_moments(*[ptr(a) for a in args], ptr(T), n, h, w, ptr(out), ptr(ws), stream_ptr()),
          'rpe_pose_backward_moments')
    return out[:, :6], out[:, 6:12], out[:, 12:].reshape(n, 6, 6)


def pose_backward_grads(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight, T, u, want):
    """fXY^T u for the inputs named in ``want`` (subset of flow, pcl1, pcl2, w1, w2) -> dict of float32 tensors."""
    args, n, h, w = _pose_inputs(flow, pcl1, pcl2, w1, w2, mask1, mask2, K, loss_weight)
    T = _dev(T.reshape(n, 7), torch.float64, 'T')
    u = _dev(u.reshape(n, 6), torch.float64, 'u')
    ch = dict(flow=2, pcl1=3, pcl2=3, w1=1, w2=1)
    outs = {k: (torch.empty(n, c, h, w, dtype=torch.float32, device=T.device) if k in want else None) for k, c in ch.items()}
    check(lib().rpe_pose_backward_grads(*[ptr(a) for a in args], ptr(T), ptr(u), n, h, w, ptr(outs['flow']), ptr(outs['pcl1']),
                                        ptr(outs['pcl2']), ptr(outs['w1']), ptr(outs['w2']), stream_ptr()), 'rpe_pose_backward_grads')
    return {k: v for k, v in outs.items() if v is not None}


# ------------------------------------------------------------------------------------------------- geometry
def depth_backproject_warp(stereo_flow2, time_flow, baseline, K, depth1, image1l, image2l, stereo_flow1, mask2,
                           want_pcl2=False):
    f32 = torch.float32
    sf2 = _dev(stereo_flow2, f32, 'stereo_flow2')
    n, _, h, w = sf2.shape
    tf, b, K = _dev(time_flow, f32, 'time_flow'), _dev(baseline, f32, 'baseline'), _dev(K, f32, 'K')
    d1, i1, i2 = _dev(depth1, f32, 'depth1'), _dev(image1l, f32, 'image1l'), _dev(image2l, f32, 'image2l')
    sf1, m2 = _dev(stereo_flow1, f32, 'stereo_flow1'), _mask(mask2, 'mask2')
    dev = sf2.device
    e = lambda *s, dt=f32: torch.empty(*s, dtype=dt, device=dev)
    depth2, pcl1, pcl2w = e(n, 1, h, w), e(n, 3, h, w), e(n, 3, h, w)
    m2v, m2w = e(n, 1, h, w, dt=torch.uint8), e(n, 1, h, w, dt=torch.uint8)
    inp1, inp2 = e(n, 8, h // 8, w // 8), e(n, 8, h // 8, w // 8)
    pcl2 = e(n, 3, h, w) if want_pcl2 else None
    check(lib().rpe_depth_backproject_warp(ptr(sf2), ptr(tf), ptr(b), ptr(K), ptr(d1), ptr(i1), ptr(i2), ptr(sf1), ptr(m2),
                                           n, h, w, ptr(depth2), ptr(m2v), ptr(pcl1), ptr(pcl2w), ptr(m2w), ptr(inp1),
                                           ptr(inp2), ptr(pcl2), stream_ptr()), 'rpe_depth_backproject_warp')
    return dict(depth2=depth2, mask2=m2v.view(torch.bool), pcl1=pcl1, pcl2w=pcl2w, mask2w=m2w.view(torch.bool),
                inp1=inp1, inp2=inp2, pcl2=pcl2)


def flow2depth(stereo_flow, baseline):
    sf = _dev(stereo_flow, torch.float32, 'stereo_flow')
    n, _, h, w = sf.shape
    b = _dev(baseline, torch.float32, 'baseline')
    depth = torch.empty(n, 1, h, w, dtype=torch.float32, device=sf.device)
    valid = torch.empty(n, 1, h, w, dtype=torch.uint8, device=sf.device)
    check(lib().rpe_flow2depth(ptr(sf), ptr(b), n, h, w, ptr(depth), ptr(valid), stream_ptr()), 'rpe_flow2depth')
    return depth, valid.view(torch.bool)


def warp_taps(flow):
    fl = _dev(flow, torch.float32, 'flow')
    n, _, h, w = fl.shape
    outs = [torch.empty(n, h, w, dtype=torch.int32, device=fl.device) for _ in range(4)]
    check(lib().rpe_warp_taps(ptr(fl), n, h, w, *[ptr(o) for o in outs], stream_ptr()), 'rpe_warp_taps')
    return dict(x0=outs[0], y0=outs[1], xn=outs[2], yn=outs[3])


GEOMETRY_GRADS = ('time_flow', 'stereo_flow2', 'stereo_flow1', 'depth1')


def depth_backproject_warp_backward(stereo_flow2, time_flow, baseline, K, depth1, image2l, stereo_flow1, mask2, grad_pcl1=None,
                                    grad_pcl2w=None, grad_inp1=None, grad_inp2=None, want=GEOMETRY_GRADS):
    """rpe_depth_backproject_warp_backward: the gradients named in ``want`` (subset of GEOMETRY_GRADS) of the stage whose forward is
    ``depth_backproject_warp``, from the incoming gradients of pcl1, pcl2w (n,3,h,w) and inp1, inp2 (n,8,h/8,w/8); None = zero.
    -> dict of float32 tensors.  Bit-identical from run to run, a row independent of its batch (no float atomics: include/rpe.h)."""
    f32 = torch.float32
    sf2 = _dev(stereo_flow2, f32, 'stereo_flow2')
    n, _, h, w = sf2.shape
    tf, b, K = _dev(time_flow, f32, 'time_flow'), _dev(baseline, f32, 'baseline'), _dev(K, f32, 'K')
    d1, i2 = _dev(depth1, f32, 'depth1'), _dev(image2l, f32, 'image2l')
    sf1, m2 = _dev(stereo_flow1, f32, 'stereo_flow1'), _mask(mask2, 'mask2')
    gin = [None if g is None else _dev(g, f32, nm) for g, nm in ((grad_pcl1, 'grad_pcl1'), (grad_pcl2w, 'grad_pcl2w'), (grad_inp1, 'grad_inp1'),
                                                                 (grad_inp2, 'grad_inp2'))]
    for g, shape in zip(gin, ((n, 3, h, w), (n, 3, h, w), (n, 8, h // 8, w // 8), (n, 8, h // 8, w // 8))):
        if g is not None and tuple(g.shape) != shape:
            raise _lib.RpeError(f'depth_backproject_warp_backward: an incoming gradient has shape {tuple(g.shape)}, expected {shape}')
    unknown = [k for k in want if k not in GEOMETRY_GRADS]
    if unknown:
        raise _lib.RpeError(f'depth_backproject_warp_backward: unknown gradients {unknown}')
    ch = dict(time_flow=2, stereo_flow2=2, stereo_flow1=2, depth1=1)
    outs = {k: (torch.empty(n, ch[k], h, w, dtype=f32, device=sf2.device) if k in want else None) for k in GEOMETRY_GRADS}
    ws = torch.empty(lib().rpe_depth_backproject_warp_backward_workspace_bytes(n, h, w), dtype=torch.uint8, device=sf2.device)
    check(lib().rpe_depth_backproject_warp_backward(ptr(sf2), ptr(tf), ptr(b), ptr(K), ptr(d1), ptr(i2), ptr(sf1), ptr(m2), n, h, w,
                                                    *[ptr(g) for g in gin], *[ptr(outs[k]) for k in GEOMETRY_GRADS], ptr(ws),
                                                    stream_ptr()), 'rpe_depth_backproject_warp_backward')
    return {k: v for k, v in outs.items() if v is not None}


def flow2depth_backward(stereo_flow, baseline, grad_depth):
    """rpe_flow2depth_backward: grad of ``flow2depth``'s depth with respect to the stereo flow (n,2,h,w); the y channel is zero."""
    sf = _dev(stereo_flow, torch.float32, 'stereo_flow')
    n, _, h, w = sf.shape
    b, gd = _dev(baseline, torch.float32, 'baseline'), _dev(grad_depth, torch.float32, 'grad_depth')
    out = torch.empty_like(sf)
    check(lib().rpe_flow2depth_backward(ptr(sf), ptr(b), ptr(gd), n, h, w, ptr(out), stream_ptr()), 'rpe_flow2depth_backward')
    return out


class _GeometryStageFn(torch.autograd.Function):
    """``depth_backproject_warp`` as one autograd node: forward = that call, backward = depth_backproject_warp_backward.  Differentiable
    inputs: stereo_flow2, time_flow, depth1, stereo_flow1; differentiable outputs: pcl1, pcl2w, inp1, inp2."""

    @staticmethod
    def forward(ctx, stereo_flow2, time_flow, baseline, K, depth1, image1l, image2l, stereo_flow1, mask2):
        g = depth_backproject_warp(stereo_flow2, time_flow, baseline, K, depth1, image1l, image2l, stereo_flow1, mask2)
        ctx.save_for_backward(stereo_flow2, time_flow, baseline, K, depth1, image2l, stereo_flow1, mask2)
        ctx.mark_non_differentiable(g['depth2'], g['mask2'], g['mask2w'])
        ctx.set_materialize_grads(False)                    # an output nothing differentiates arrives as None = the kernel's NULL
        return g['pcl1'], g['pcl2w'], g['inp1'], g['inp2'], g['depth2'], g['mask2'], g['mask2w']

    @staticmethod
    def backward(ctx, g_pcl1, g_pcl2w, g_inp1, g_inp2, *_):
        need = ctx.needs_input_grad
        names = {'stereo_flow2': need[0], 'time_flow': need[1], 'depth1': need[4], 'stereo_flow1': need[7]}
        want = [k for k in GEOMETRY_GRADS if names[k]]
        g = depth_backproject_warp_backward(*ctx.saved_tensors, g_pcl1, g_pcl2w, g_inp1, g_inp2, want=want) if want else {}
        return (g.get('stereo_flow2'), g.get('time_flow'), None, None, g.get('depth1'), None, None, g.get('stereo_flow1'), None)


def geometry_stage(stereo_flow2, time_flow, baseline, K, depth1, image1l, image2l, stereo_flow1, mask2):
    """``depth_backproject_warp`` (the same dict, bit for bit; 'pcl2' is None) with gradients: pcl1, pcl2w, inp1 and inp2 are
    differentiable with respect to stereo_flow2, time_flow, depth1 and stereo_flow1; depth2 and the masks carry none."""
    pcl1, pcl2w, inp1, inp2, depth2, m2v, m2w = _GeometryStageFn.apply(stereo_flow2, time_flow, baseline, K, depth1, image1l, image2l,
                                                                        stereo_flow1, mask2)
    return dict(depth2=depth2, mask2=m2v, pcl1=pcl1, pcl2w=pcl2w, mask2w=m2w, inp1=inp1, inp2=inp2, pcl2=None)


class _Flow2DepthFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stereo_flow, baseline):
        depth, valid = flow2depth(stereo_flow, baseline)
        ctx.save_for_backward(stereo_flow, baseline)
        ctx.mark_non_differentiable(valid)
        ctx.set_materialize_grads(False)
        return depth, valid

    @staticmethod
    def backward(ctx, g_depth, _):
        return (None if g_depth is None else flow2depth_backward(*ctx.saved_tensors, g_depth)), None


def flow2depth_grad(stereo_flow, baseline):
    """``flow2depth`` (the same depth and validity, bit for bit) with the depth differentiable with respect to the stereo flow."""
    return _Flow2DepthFn.apply(stereo_flow, baseline)


# ------------------------------------------------------------------------------------------------- correlation
class CorrPyramid:
    """Opaque device buffer holding the 4-level correlation pyramid of a batch of pairs."""

    def __init__(self, b, h8, w8, levels=4, radius=4, device='cuda', bf16x3=False):
        """``bf16x3``: size the scratch for the RPE_F32X3 experiment (1.5x the feature-map scratch); build(bf16x3=True) needs it."""
        self.b, self.h8, self.w8, self.levels, self.radius = b, h8, w8, levels, radius
        nbytes = lib().rpe_corr_pyramid_bytes_ex(b, h8, w8, levels, 3 if bf16x3 else 0)
        if nbytes == 0:
            raise _lib.RpeError('rpe_corr_pyramid_bytes: unsupported geometry')
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)

    def build(self, fmap1, fmap2, fp16_features=False, bf16x3=False):
        """``fp16_features``: BASELINE config 5 -- both maps are rounded to fp16 and correlated on the 16-bit matrix cores
        with f32 accumulation; the pyramid stays f32.  ``bf16x3``: f32 features, every f32 product evaluated as six bf16 products of
        an exact three-way split (RPE_F32X3: f32-equivalent results at 3/8 of the matrix time)."""
        f1, f2 = _dev(fmap1, torch.float32, 'fmap1'), _dev(fmap2, torch.float32, 'fmap2')
        b, c, h8, w8 = f1.shape
        if (b, h8, w8) != (self.b, self.h8, self.w8) or f2.shape != f1.shape:
            raise _lib.RpeError('corr build: shape mismatch')
        mode = 2 if fp16_features else 3 if bf16x3 else 0
        if self.buf.numel() < lib().rpe_corr_pyramid_bytes_ex(b, h8, w8, self.levels, mode):
            raise _lib.RpeError('corr build: this pyramid was not sized for the requested feature mode (CorrPyramid(..., bf16x3=True))')
        return _launch(_lib.OP_CORR_BUILD, (ptr(f1), ptr(f2), b, c, h8, w8, self.levels, mode, ptr(self.buf)), (f1, f2, self), self)

    def lookup(self, coords, out=None, prepare=False, map_size=None):
        """``prepare=True`` (needs ``out``): a zero-argument launcher on these buffers, with ``.op`` for an OpList.
        ``map_size`` = (mh, mw) (needs ``out``): coords (b,2,mh,mw) and out (b,ch,mh,mw) are larger maps whose top-left h8 x w8 is read /
        written (rpe_corr_lookup_ex: the padded workspace of RAFT's pad_maps route); the rest of ``out`` is left alone."""
        co = _dev(coords, torch.float32, 'coords')
        ch = self.levels * (2 * self.radius + 1) ** 2
        if map_size is not None:
            return _lookup_ex(self, _lib.OP_CORR_LOOKUP_EX, (ptr(self.buf), ptr(co), self.b, self.h8, self.w8, self.levels, self.radius), coords, co, out, ch,
                              map_size, prepare)
        if tuple(co.shape) != (self.b, 2, self.h8, self.w8):
            raise _lib.RpeError('corr lookup: coords shape mismatch')
        if out is None:
            out = torch.empty(self.b, ch, self.h8, self.w8, dtype=torch.float32, device=co.device)
        if prepare and (co is not coords or tuple(_nchw(out, 'out').shape) != (self.b, ch, self.h8, self.w8)):
            raise _lib.RpeError('corr lookup: a prepared launch needs contiguous coords and a (b, levels*(2r+1)^2, h8, w8) out buffer')
        return _launch(_lib.OP_CORR_LOOKUP, (ptr(self.buf), ptr(co), self.b, self.h8, self.w8, self.levels, self.radius, ptr(out)), (self, co, out), out,
                       prepare)

    def lookup_conv1x1(self, coords, packed, out, out2=None, relu=True, prepare=False):
        """rpe_corr_lookup_conv1x1: act(convc1(lookup(coords))) in one kernel (``packed`` = PackedLookupConv of convc1's weight), written to the
        channel slices ``out`` / ``out2`` (b, 256, h8, w8); bit-identical to lookup() + conv1x1.  ``prepare=True``: a launcher with ``.op``."""
        co = _dev(coords, torch.float32, 'coords')
        if co is not coords or tuple(co.shape) != (self.b, 2, self.h8, self.w8):
            raise _lib.RpeError('corr lookup_conv1x1: coords must be a contiguous (b,2,h8,w8) tensor')
        if not PackedLookupConv.supported(self.levels, self.radius, self.w8):
            raise _lib.RpeError('corr lookup_conv1x1: needs 4 levels, radius 4 and w8 % 8 == 0 (use lookup + conv1x1)')
        sl = _opt_slices('corr lookup_conv1x1', self.b, packed.cout, self.h8, self.w8, out=out, out2=out2)
        return _launch(_lib.OP_LOOKUP_CONV1X1, (ptr(self.buf), ptr(co), self.b, self.h8, self.w8, self.levels, self.radius, ptr(packed.packed),
                                                ptr(packed.bias), int(bool(relu)), *sl), (self, co, packed, out, out2), out, prepare)

    def taps(self, coords):
        co = _dev(coords, torch.float32, 'coords')
        win = 2 * self.radius + 1
        x0 = torch.empty(self.b, self.levels, win, self.h8 * self.w8, dtype=torch.int32, device=co.device)
        y0 = torch.empty_like(x0)
        check(lib().rpe_corr_lookup_taps(ptr(co), self.b, self.h8, self.w8, self.levels, ptr(x0), ptr(y0), stream_ptr()),
              'rpe_corr_lookup_taps')
        return x0, y0

    def rounds(self, coords):
        """Diagnostic (rpe_corr_lookup_rounds): staging rounds and requested 128-B lines per (batch item, level, group)."""
        co = _dev(coords, torch.float32, 'coords')
        ng = self.h8 * ((self.w8 + 7) // 8)
        rounds = torch.zeros(self.b, self.levels, ng, dtype=torch.int32, device=co.device)
        lines = torch.zeros_like(rounds)
        check(lib().rpe_corr_lookup_rounds(ptr(co), self.b, self.h8, self.w8, self.levels, ptr(rounds), ptr(lines), stream_ptr()),
              'rpe_corr_lookup_rounds')
        return rounds, lines

    def export_level(self, level):
        h, w = self.h8 >> level, self.w8 >> level
        dense = torch.empty(self.b * self.h8 * self.w8, h, w, dtype=torch.float32, device=self.buf.device)
        check(lib().rpe_corr_export_level(ptr(self.buf), self.b, self.h8, self.w8, self.levels, level, ptr(dense),
                                          stream_ptr()), 'rpe_corr_export_level')
        return dense


class AltCorr:
    """The correlation of a batch of pairs WITHOUT the all-pairs volume (upstream RAFT's ``alternate_corr``; csrc/corr_alt.hip): the
    device buffer holds fmap1 / sqrt(c) and fmap2 with its pooled copies, pixel-major, and every lookup recomputes its windows from
    them.  Same build / lookup interface as CorrPyramid (what RAFT's loop calls); ``nbytes`` = the size of the buffer.
    ``fp16=True`` (rpe_corr_alt_prepare_ex / rpe_corr_alt_lookup_dt with RPE_F16): the buffer holds half(fmap1) and half(fmap2), unscaled,
    with the pooled copies rounded to fp16 level after level -- half the bytes --, the window products run on the 16-bit matrix cores with
    f32 accumulation and 1 / sqrt(c) is applied in f32.  ``fp16=False`` makes exactly the f32 calls."""

    def __init__(self, b, c, h8, w8, levels=4, radius=4, device='cuda', fp16=False):
        self.b, self.c, self.h8, self.w8, self.levels, self.radius, self.fp16 = b, c, h8, w8, levels, radius, bool(fp16)
        self.nbytes = lib().rpe_corr_alt_bytes_ex(b, c, h8, w8, levels, _lib.F16 if self.fp16 else _lib.F32)
        if self.nbytes == 0 or radius != 4:
            raise _lib.RpeError('rpe_corr_alt_bytes: unsupported geometry')
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=device)

    def build(self, fmap1, fmap2):
        f1, f2 = _dev(fmap1, torch.float32, 'fmap1'), _dev(fmap2, torch.float32, 'fmap2')
        if tuple(f1.shape) != (self.b, self.c, self.h8, self.w8) or f2.shape != f1.shape:
            raise _lib.RpeError('corr alt build: shape mismatch')
        if self.fp16:
            return _launch(_lib.OP_CORR_ALT_PREPARE_EX, (ptr(f1), ptr(f2), self.b, self.c, self.h8, self.w8, self.levels, _lib.F16, ptr(self.buf)), (f1, f2, self),
                           self)
        return _launch(_lib.OP_CORR_ALT_PREPARE, (ptr(f1), ptr(f2), self.b, self.c, self.h8, self.w8, self.levels, ptr(self.buf)), (f1, f2, self), self)

    def lookup(self, coords, out=None, prepare=False, map_size=None):
        """``prepare=True`` (needs ``out``): a zero-argument launcher on these buffers, with ``.op`` for an OpList.  ``map_size``: as
        CorrPyramid.lookup (rpe_corr_alt_lookup_ex).  With ``fp16`` every form is rpe_corr_alt_lookup_dt (dense: map_size = (h8, w8))."""
        co = _dev(coords, torch.float32, 'coords')
        ch = self.levels * (2 * self.radius + 1) ** 2
        if map_size is not None:
            return _lookup_ex(self, _lib.OP_CORR_ALT_LOOKUP_DT if self.fp16 else _lib.OP_CORR_ALT_LOOKUP_EX,
                              (ptr(self.buf), ptr(co), self.b, self.c, self.h8, self.w8, self.levels, self.radius), coords, co, out, ch, map_size, prepare,
                              tail=(_lib.F16,) if self.fp16 else ())
        if tuple(co.shape) != (self.b, 2, self.h8, self.w8):
            raise _lib.RpeError('corr alt lookup: coords shape mismatch')
        if out is None:
            out = torch.empty(self.b, ch, self.h8, self.w8, dtype=torch.float32, device=co.device)
        if prepare and co is not coords:
            raise _lib.RpeError('corr alt lookup: a prepared launch needs contiguous coords and a (b, levels*(2r+1)^2, h8, w8) out buffer')
        if tuple(_nchw(out, 'out').shape) != (self.b, ch, self.h8, self.w8):
            raise _lib.RpeError('corr alt lookup: out must be a contiguous (b, levels*(2r+1)^2, h8, w8) buffer')
        if self.fp16:
            return _launch(_lib.OP_CORR_ALT_LOOKUP_DT, (ptr(self.buf), ptr(co), self.b, self.c, self.h8, self.w8, self.levels, self.radius, self.h8, self.w8,
                                                        _lib.F16, ptr(out)), (self, co, out), out, prepare)
        return _launch(_lib.OP_CORR_ALT_LOOKUP, (ptr(self.buf), ptr(co), self.b, self.c, self.h8, self.w8, self.levels, self.radius, ptr(out)),
                       (self, co, out), out, prepare)


def _lookup_ex(corr, kind, head, coords, co, out, ch, map_size, prepare, tail=()):
    """The pitched lookup of CorrPyramid / AltCorr: ``head`` = the entry point's arguments up to the radius, ``tail`` = those between the map
    size and ``out``."""
    mh, mw = map_size
    if mh < corr.h8 or mw < corr.w8 or co is not coords or tuple(co.shape) != (corr.b, 2, mh, mw):
        raise _lib.RpeError(f'corr lookup: with map_size coords must be a contiguous ({corr.b},2,{mh},{mw}) tensor, the map at least ({corr.h8},{corr.w8})')
    if out is None or tuple(_nchw(out, 'out').shape) != (corr.b, ch, mh, mw):
        raise _lib.RpeError(f'corr lookup: with map_size out must be a contiguous ({corr.b},{ch},{mh},{mw}) buffer')
    return _launch(kind, (*head, mh, mw, *tail, ptr(out)), (corr, co, out), out, prepare)


class _Packed:
    """A convolution's weight (and bias) re-laid once per weight version for the entry point ``entry`` that launches it.  A subclass states
    what differs: the kernel shapes it takes (``kernels``, or _fits) and the error text, its size query (``size``: floats, or bytes with
    ``in_bytes`` -- bf16 planes kept in float32 storage for the descriptor) and its pack entry point (``pack``)."""
    kernels, in_bytes = (), False

    def __init__(self, weight, bias=None):
        w = _nchw(weight.detach().contiguous(), 'weight')
        self.cout, self.cin, self.kh, self.kw = w.shape
        n = getattr(lib(), self.size)(*self._dims()) if self._fits() else 0
        if n == 0:
            raise _lib.RpeError(f'{type(self).__name__}: {self.error}')
        self.packed = torch.empty(n // 4 if self.in_bytes else n, dtype=torch.float32, device=w.device)
        check(getattr(lib(), self.pack)(ptr(w), *self._dims(), ptr(self.packed), stream_ptr()), self.pack)
        self.bias = None if bias is None else _nchw(bias.detach().contiguous(), 'bias')

    def _dims(self):
        return self.cout, self.cin

    def _fits(self):
        return (self.kh, self.kw) in self.kernels


class PackedLookupConv(_Packed):
    """convc1's (256, 324, 1, 1) weight in rpe_corr_lookup_conv1x1's layout (a lane's fragments of a 16-channel step as one 64-byte piece)."""
    kernels, error = ((1, 1),), 'needs the (256, 324, 1, 1) weight of BasicMotionEncoder.convc1'
    size, pack, entry = 'rpe_corr_lookup_conv1x1_packed_floats', 'rpe_corr_lookup_conv1x1_pack', 'rpe_corr_lookup_conv1x1'

    @staticmethod
    def supported(levels, radius, w8):
        return levels == 4 and radius == 4 and w8 % 8 == 0


# ------------------------------------------------------------------------------------------------- RAFT update
def _nchw(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise _lib.RpeError(f'{name}: expected a contiguous float32 NCHW tensor on the GPU')
    _on_current_device(t, name)
    return t


def gru_gates_zr(zr_pre, h_buf, c, z_out, rh_buf, bias=None, add=None):
    """z_out = sigmoid(zr_pre[:, :c] + add[:, :c] + bias[:c]); rh_buf[:, :c] = sigmoid(zr_pre[:, c:] + ...) * h_buf[:, :c]."""
    _nchw(zr_pre, 'zr_pre'); _nchw(h_buf, 'h_buf'); _nchw(z_out, 'z_out'); _nchw(rh_buf, 'rh_buf')
    if add is not None and _nchw(add, 'add').shape != zr_pre.shape:
        raise _lib.RpeError('gru_gates_zr: add must have the shape of zr_pre')
    b, c2, hh, ww = zr_pre.shape
    check(lib().rpe_gru_gates_zr(ptr(zr_pre), ptr(bias), ptr(add), ptr(h_buf), h_buf.shape[1], b, c, hh * ww, ptr(z_out),
                                 ptr(rh_buf), rh_buf.shape[1], stream_ptr()), 'rpe_gru_gates_zr')


def gru_gates_h(z, q_pre, h_buf, c, h_out, bias=None, add=None):
    """h_out[:, :c] = (1 - z) * h_buf[:, :c] + z * tanh(q_pre + add + bias)."""
    _nchw(z, 'z'); _nchw(q_pre, 'q_pre'); _nchw(h_buf, 'h_buf'); _nchw(h_out, 'h_out')
    if add is not None and _nchw(add, 'add').shape != q_pre.shape:
        raise _lib.RpeError('gru_gates_h: add must have the shape of q_pre')
    b, _, hh, ww = q_pre.shape
    check(lib().rpe_gru_gates_h(ptr(z), ptr(q_pre), ptr(bias), ptr(add), ptr(h_buf), h_buf.shape[1], b, c, hh * ww, ptr(h_out),
                                h_out.shape[1], stream_ptr()), 'rpe_gru_gates_h')


def bias_act(x, bias, relu=True, out=None, out_offset=0, out2=None, out2_offset=0):
    """act(x + bias[c]) -> channels [out_offset, out_offset + c) of ``out`` (default: in place on x) and optionally
    the same into ``out2``."""
    _nchw(x, 'x')
    b, c, hh, ww = x.shape
    out = x if out is None else _nchw(out, 'out')
    if out2 is not None:
        _nchw(out2, 'out2')
    check(lib().rpe_bias_act(ptr(x), ptr(bias), b, c, hh * ww, int(bool(relu)), ptr(out), out.shape[1], out_offset,
                             ptr(out2), out2.shape[1] if out2 is not None else 0, out2_offset, stream_ptr()), 'rpe_bias_act')
    return out


def instnorm_act(x, bias, eps=1e-5, relu=True, residual=None, out=None):
    """relu?(InstanceNorm(x + bias)), then optionally relu(residual + .) -- one pass per plane."""
    _nchw(x, 'x')
    if residual is not None:
        _nchw(residual, 'residual')
    b, c, hh, ww = x.shape
    out = x if out is None else _nchw(out, 'out')
    check(lib().rpe_instnorm_act(ptr(x), ptr(bias), b, c, hh * ww, float(eps), int(bool(relu)), ptr(residual), ptr(out),
                                 stream_ptr()), 'rpe_instnorm_act')
    return out


def affine_act(x, scale, shift, relu=True, residual=None, out=None):
    """relu?(x * scale[c] + shift[c]), then optionally relu(residual + .)."""
    _nchw(x, 'x')
    if residual is not None:
        _nchw(residual, 'residual')
    b, c, hh, ww = x.shape
    out = x if out is None else _nchw(out, 'out')
    check(lib().rpe_affine_act(ptr(x), ptr(scale), ptr(shift), b, c, hh * ww, int(bool(relu)), ptr(residual), ptr(out),
                               stream_ptr()), 'rpe_affine_act')
    return out


def conv3x3_to2(x, weight, bias, add=None, out=None):
    """out = conv3x3(x, weight (2,c,3,3), padding=1) + bias [+ add]; the flow head's last layer."""
    _nchw(x, 'x')
    b, c, hh, ww = x.shape
    weight = _nchw(weight.detach() if weight.requires_grad else weight, 'weight')
    if tuple(weight.shape) != (2, c, 3, 3):
        raise _lib.RpeError('conv3x3_to2: weight must be (2,c,3,3)')
    if add is not None:
        _nchw(add, 'add')
    if out is None:
        out = torch.empty(b, 2, hh, ww, dtype=torch.float32, device=x.device)
    check(lib().rpe_conv3x3_to2(ptr(x), ptr(weight), ptr(bias), b, c, hh, ww, ptr(add), ptr(out), stream_ptr()), 'rpe_conv3x3_to2')
    return out


def flow_update(x, weight, bias, coords, coords_out, flow_out=None, dst1=None, dst2=None, prepare=False, valid=None):
    """rpe_conv3x3_to2_flow: coords_out = conv3x3(x; weight (2,c,3,3)) + bias + coords, and flow = coords_out - pixel grid written to
    ``flow_out`` (b,2,h,w) and into the two-channel slices ``dst1`` / ``dst2`` (e.g. hx[:, 254:256]).  ``prepare=True`` returns a launcher.
    ``valid`` = (hv, wv): the maps are zero-padded and hold hv x wv of content (rpe_conv3x3_to2_flow_v): outside it coords_out is the pixel
    grid and the flow exactly zero."""
    _nchw(x, 'flow_update: x')
    b, c, hh, ww = x.shape
    weight = _nchw(weight.detach() if weight.requires_grad else weight, 'flow_update: weight')
    if tuple(weight.shape) != (2, c, 3, 3):
        raise _lib.RpeError('flow_update: weight must be (2,c,3,3)')
    for name, t in (('coords', coords), ('coords_out', coords_out), ('flow_out', flow_out)):
        if t is not None and tuple(_nchw(t, f'flow_update: {name}').shape) != (b, 2, hh, ww):
            raise _lib.RpeError(f'flow_update: {name} must be ({b},2,{hh},{ww})')
    sl = _opt_slices('flow_update', b, 2, hh, ww, dst1=dst1, dst2=dst2)
    args = (ptr(x), ptr(weight), ptr(bias), b, c, hh, ww, ptr(coords), ptr(coords_out), ptr(flow_out), *sl)
    keep = (x, weight, bias, coords, coords_out, flow_out, dst1, dst2)
    if valid is not None:
        return _launch(_lib.OP_FLOW_UPDATE_V, (*args, *_valid_extent('flow_update', valid, hh, ww)), keep, coords_out, prepare)
    return _launch(_lib.OP_FLOW_UPDATE, args, keep, coords_out, prepare)


def _valid_extent(who, valid, hh, ww):
    """(hv, wv) of a ``valid=`` argument, checked against the map: the library refuses an extent beyond it too (RPE_E_BADARG)."""
    hv, wv = (int(v) for v in valid)
    if not (0 < hv <= hh and 0 < wv <= ww):
        raise _lib.RpeError(f'{who}: valid extent ({hv},{wv}) does not lie inside the ({hh},{ww}) map')
    return hv, wv


def copy_rect(src, dst, hh, ww):
    """dst[:, :, :hh, :ww] = src[:, :, :hh, :ww] (rpe_copy_rect) for 4-D float32 tensors with unit stride along x and any row pitch, plane and
    batch stride -- contiguous maps, channel slices, and both against maps of another size: into and out of a padded workspace."""
    for name, t in (('src', src), ('dst', dst)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.stride(3) == 1):
            raise _lib.RpeError(f'copy_rect: {name} must be a float32 NCHW GPU tensor with unit stride along x')
        _on_current_device(t, f'copy_rect: {name}')
        if t.shape[2] < hh or t.shape[3] < ww:
            raise _lib.RpeError(f'copy_rect: {name} {tuple(t.shape)} is smaller than the ({hh},{ww}) rectangle')
    b, c = src.shape[:2]
    if tuple(dst.shape[:2]) != (b, c):
        raise _lib.RpeError('copy_rect: batch / channel mismatch')
    return _launch(_lib.OP_COPY_RECT, (ptr(src), src.stride(0), src.stride(1), src.stride(2), ptr(dst), dst.stride(0), dst.stride(1), dst.stride(2), b, c, hh, ww),
                   (src, dst), dst)


def copy_planes(src, dst):
    """dst[:, :c] = src for channel slices of NCHW buffers (rpe_copy_planes)."""
    sp, sbs = _chan_slice(src, 'src')
    dp, dbs = _chan_slice(dst, 'dst')
    b, c, hh, ww = src.shape
    if tuple(dst.shape) != (b, c, hh, ww):
        raise _lib.RpeError('copy_planes: shape mismatch')
    return _launch(_lib.OP_COPY_PLANES, (sp, sbs, dp, dbs, b, c, hh * ww), (src, dst), dst)


def forward_interpolate(flow, out=None):
    """Upstream RAFT's forward_interpolate (core/RAFT/core/utils/utils.py) of a 1/8 flow (N,2,h,w) f32, row by row on the GPU
    (rpe_flow_forward_interpolate): each pixel's flow is pushed forward along itself, and every grid point takes the flow of the nearest
    landing point strictly inside the map (ties to the lowest source index; a row with no such point gives zeros, where upstream's scipy
    raises).  Bit-exact copies of input values; ``out`` must not overlap ``flow``.  No allocation when ``out`` is given, no synchronisation."""
    fl = _dev(flow, torch.float32, 'flow')
    if fl.dim() != 4 or fl.shape[1] != 2:
        raise _lib.RpeError(f'forward_interpolate: flow must be (N,2,h,w), got {tuple(fl.shape)}')
    n, _, hh, ww = fl.shape
    if out is None:
        out = torch.empty_like(fl)
    elif tuple(out.shape) != tuple(fl.shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != fl.device:
        raise _lib.RpeError(f'forward_interpolate: out must be a contiguous float32 tensor of shape {tuple(fl.shape)} on {fl.device}')
    if _overlap_span(fl, out):
        raise _lib.RpeError('forward_interpolate: out must not overlap flow')
    check(lib().rpe_flow_forward_interpolate(ptr(fl), n, hh, ww, ptr(out), stream_ptr()), 'rpe_flow_forward_interpolate')
    return out


def _overlap_span(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def flow_seed(flow_init, coords_out=None, flow_out=None, dst1=None, dst2=None, prepare=False):
    """rpe_flow_seed, the front of a warm update loop: coords_out = pixel grid + flow_init, flow_out = flow_init, and flow_init into the
    two-channel slices ``dst1`` / ``dst2`` (e.g. hx[:, 254:256]); flow_init (b,2,h,w) contiguous.  ``prepare=True`` returns a launcher."""
    fi = _nchw(flow_init, 'flow_seed: flow_init')
    b, c, hh, ww = fi.shape
    if c != 2:
        raise _lib.RpeError(f'flow_seed: flow_init must be (b,2,h,w), got {tuple(fi.shape)}')
    for name, t in (('coords_out', coords_out), ('flow_out', flow_out)):
        if t is not None and tuple(_nchw(t, f'flow_seed: {name}').shape) != (b, 2, hh, ww):
            raise _lib.RpeError(f'flow_seed: {name} must be ({b},2,{hh},{ww})')
    sl = _opt_slices('flow_seed', b, 2, hh, ww, dst1=dst1, dst2=dst2)
    return _launch(_lib.OP_FLOW_SEED, (ptr(fi), b, hh, ww, ptr(coords_out), ptr(flow_out), *sl), (fi, coords_out, flow_out, dst1, dst2),
                   coords_out, prepare)


def upsample_convex(flow, mask, size=None):
    """``size`` = (h8, w8): flow and mask are larger (zero-padded) maps whose top-left h8 x w8 is up-sampled (rpe_upsample_convex_ex)."""
    fl, mk = _dev(flow, torch.float32, 'flow'), _dev(mask, torch.float32, 'mask')
    b, _, h8, w8 = fl.shape
    if size is not None:
        mh, mw, (h8, w8) = h8, w8, size
        if tuple(mk.shape) != (b, 576, mh, mw) or not (0 < h8 <= mh and 0 < w8 <= mw):
            raise _lib.RpeError('upsample_convex: mask must be (b,576,mh,mw) like the flow map, size within it')
        out = torch.empty(b, 2, 8 * h8, 8 * w8, dtype=torch.float32, device=fl.device)
        return _launch(_lib.OP_UPSAMPLE_CONVEX_EX, (ptr(fl), ptr(mk), b, h8, w8, mh, mw, ptr(out)), (fl, mk, out), out)
    if tuple(mk.shape) != (b, 576, h8, w8):
        raise _lib.RpeError('upsample_convex: mask must be (b,576,h/8,w/8)')
    out = torch.empty(b, 2, 8 * h8, 8 * w8, dtype=torch.float32, device=fl.device)
    return _launch(_lib.OP_UPSAMPLE_CONVEX, (ptr(fl), ptr(mk), b, h8, w8, ptr(out)), (fl, mk, out), out)


# ------------------------------------------------------------------------- fused update-block convolutions
CONV_LINEAR, CONV_RELU, CONV_GATE_ZR, CONV_GATE_H, CONV_TANH = 0, 1, 2, 3, 4


def _chan_slice(t, name):
    """(pointer, batch stride) of a float32 GPU tensor that is a channel slice ``buf[:, a:b]`` of a contiguous NCHW
    buffer (or such a buffer itself)."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
        raise _lib.RpeError(f'{name}: expected a float32 NCHW tensor on the GPU')
    _, _, hh, ww = t.shape
    if t.stride(3) != 1 or t.stride(2) != ww or t.stride(1) != hh * ww:
        raise _lib.RpeError(f'{name}: expected a channel slice of a contiguous NCHW buffer')
    _on_current_device(t, name)
    return ptr(t), t.stride(0)


def _opt_slices(who, b, c, hh, ww, **named):
    """The flat [pointer, batch stride, ...] of optional (b,c,hh,ww) channel slices; [None, 0] for one that is not given."""
    sl = []
    for name, t in named.items():
        if t is None:
            sl += [None, 0]
        elif tuple(t.shape) != (b, c, hh, ww):
            raise _lib.RpeError(f'{who}: {name} must be a ({b},{c},{hh},{ww}) channel slice')
        else:
            sl += _chan_slice(t, f'{who}: {name}')
    return sl


class PackedConv(_Packed):
    """Weights of one stride-1 'same' convolution re-laid for rpe_conv_fused (done once per weight version)."""
    error = 'needs a non-empty (cout, cin, kh, kw) weight'
    size, pack, entry = 'rpe_conv_packed_floats', 'rpe_conv_pack', 'rpe_conv_fused'

    def _dims(self):
        return self.cout, self.cin, self.kh, self.kw

    def _fits(self):
        return True

    @staticmethod
    def supported(weight, width):
        _, _, kh, kw = weight.shape
        return kh % 2 == 1 and kw in (1, 3, 5) and width % 4 == 0


class PackedConv1x1(_Packed):
    """Weights of a 1x1 stride-1 convolution in rpe_conv1x1's layout ([co tile][16-channel step][k][128 co]); same attributes as
    PackedConv, so conv_fused(..., entry='rpe_conv1x1') builds the descriptor."""
    kernels, error = ((1, 1),), 'weight must be (cout, cin, 1, 1)'
    size, pack, entry = 'rpe_conv1x1_packed_floats', 'rpe_conv1x1_pack', 'rpe_conv1x1'

    @staticmethod
    def supported(h, w):
        return (h * w) % 4 == 0 and h * w >= 4


class PackedConv1x1X3(_Packed):
    """Weights of a 1x1 stride-1 convolution split three ways into bf16 for rpe_conv1x1_x3 (the labelled bf16x3 variant of rpe_conv1x1;
    conv1x1 dispatches on the packing).  LINEAR / RELU only."""
    kernels, error, in_bytes = ((1, 1),), 'weight must be (cout, cin, 1, 1)', True
    size, pack, entry = 'rpe_conv1x1_x3_packed_bytes', 'rpe_conv1x1_x3_pack', 'rpe_conv1x1_x3'


class PackedConvF16(_Packed):
    """Weights of a stride-1 'same' convolution (1x1, 3x3, 1x5, 5x1; any cin, any cout) rounded to fp16 and laid out in matrix-fragment
    order for rpe_conv_f16: rpe_conv_fused's operation with fp16 OPERANDS (round to nearest even), f32 products, f32 sum in a fixed order,
    f32 epilogue -- the precision contract of RAFT's ``update_fp16`` (include/rpe.h).  conv_fused, conv_wino, conv_wino1d, conv1x1 and
    Conv1x1(..., f16=True) run rpe_conv_f16 when handed this packing; every epilogue mode of conv_fused, no scale / residual / stats /
    pre_norm / stride 2 / valid extent."""
    kernels, error, in_bytes = ((1, 1), (3, 3), (1, 5), (5, 1)), 'needs a (cout, cin, kh, kw) weight with (kh, kw) in 1x1, 3x3, 1x5, 5x1', True
    size, pack, entry = 'rpe_conv_f16_packed_bytes', 'rpe_conv_f16_pack', 'rpe_conv_f16'

    def _dims(self):
        return self.cout, self.cin, self.kh, self.kw

    @staticmethod
    def supported(weight, h, w):
        return tuple(weight.shape[2:]) in PackedConvF16.kernels and h > 0 and w > 0 and w % 4 == 0


def conv1x1(x, pc, mode, out, out2=None, prepare=False, valid=None):
    """rpe_conv1x1: out = act(W x + bias) for a PackedConv1x1 (LINEAR / RELU / TANH), channel-slice destinations like conv_fused
    (a PackedConv1x1X3 runs rpe_conv1x1_x3)."""
    return conv_fused(x, pc, mode, out, out2=out2, prepare=prepare, entry=pc.entry, valid=valid)


class Conv1x1:
    """A 1x1 layer with both packings, each made on first use: launches of at least 512 workgroups of 128 x 128 run on rpe_conv1x1
    (LDS-DMA GEMM: convc1 337 -> 260 us at batch 32), smaller ones on rpe_conv_fused, whose 64 x 64 tiles fill the chip better (batch 2:
    29 vs 32 us).  The two kernels sum the same products in the same order (bit-identical results), so the choice never shows."""

    def __init__(self, weight, bias=None):
        self._w = _nchw(weight.detach().contiguous(), 'weight')
        self._b = None if bias is None else _nchw(bias.detach().contiguous(), 'bias')
        self.cout, self.cin = self._w.shape[0], self._w.shape[1]
        self._packings = {}

    def _packing(self, cls):
        p = self._packings.get(cls)
        if p is None:
            p = self._packings[cls] = cls(self._w, self._b)
        return p

    fused = property(lambda self: self._packing(PackedConv))
    gemm = property(lambda self: self._packing(PackedConv1x1))
    gemm_x3 = property(lambda self: self._packing(PackedConv1x1X3))
    f16 = property(lambda self: self._packing(PackedConvF16))

    def __call__(self, x, mode, out, out2=None, prepare=False, x3=False, valid=None, f16=False):
        b, _, hh, ww = x.shape
        if f16:                                               # the fp16-operand contract (raft.UPDATE_FP16): rpe_conv_f16 at EVERY launch size, or an error
            if x3 or valid is not None:
                raise _lib.RpeError('Conv1x1: f16 runs on rpe_conv_f16 alone -- not with x3, and there is no valid-extent form of it')
            return conv_fused(x, self.f16, mode, out, out2=out2, prepare=prepare)
        # rpe_conv1x1's own preconditions (16-byte DMA pieces): plane size, base and batch stride of the input slice
        aligned = PackedConv1x1.supported(hh, ww) and x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0
        big = b * -(-(hh * ww) // 128) * -(-self.cout // 128) >= 512 and aligned
        if aligned and x3 and mode in (CONV_LINEAR, CONV_RELU):     # the labelled bf16x3 variant (raft.CONV_BF16X3): at EVERY launch size, so that a
            #                                                            row's bits do not depend on the batch it is launched in
            return conv1x1(x, self.gemm_x3, mode, out, out2=out2, prepare=prepare)
        if valid is not None:                                 # a valid extent inside a padded map: rpe_conv1x1_v at every launch size (same bits as either)
            if not aligned or x3:
                raise _lib.RpeError('Conv1x1: a valid extent needs the f32 GEMM route (16-byte aligned input slice, h * w % 4 == 0, no bf16x3)')
            return conv1x1(x, self.gemm, mode, out, out2=out2, prepare=prepare, valid=valid)
        if big:
            return conv1x1(x, self.gemm, mode, out, out2=out2, prepare=prepare)
        return conv_fused(x, self.fused, mode, out, out2=out2, prepare=prepare)


# The slice rules of an epilogue: descriptor field -> ('min' | 'exact', channels: 'cout' | 'gate' (gate_channels), required); a field
# without a rule is optional and may have any number of channels
_PLAIN_RULES = dict(add=('exact', 'cout', False), out=('min', 'cout', True), out2=('min', 'cout', False), residual=('exact', 'cout', False))
_FUSED_RULES = {CONV_GATE_ZR: dict(add=('exact', 'cout', False), out=('min', 'gate', True), out2=('min', 'gate', True), hidden=('min', 'gate', True)),
                CONV_GATE_H: dict(add=('exact', 'cout', False), out=('min', 'cout', True), hidden=('min', 'cout', True), zgate=('min', 'cout', True))}
_WINO_RULES = dict(out=('min', 'cout', True), out2=('min', 'cout', False), residual=('min', 'cout', False))
_FUSED_MODES = (CONV_LINEAR, CONV_RELU, CONV_GATE_ZR, CONV_GATE_H, CONV_TANH)


def conv_fused(x, pc, mode, out, out2=None, add=None, hidden=None, zgate=None, gate_channels=0, scale=None, bias='packed',
               residual=None, stats=None, stride=1, pre_norm=None, prepare=False, entry='rpe_conv_fused', valid=None, enc_valid=None):
    """rpe_conv_fused: out = epilogue(conv(x; pc) * scale + add + bias).  All tensors are channel slices of NCHW buffers.
    ``bias`` defaults to the one packed with the weights; ``stats`` (from conv_stats_buffer) collects the per-tile moments
    instnorm_apply needs.  ``prepare=True`` returns a zero-argument launcher instead of launching: the GRU loop runs the same
    nine convolutions on the same buffers twelve times, and at batch 1 the Python argument checking costs more than the kernels.
    ``valid`` = (hv, wv): the entry point's ``_v`` form (rpe_conv_wino1d_v, rpe_conv1x1_v): the map is zero-padded, the epilogue stores zero
    outside its hv x wv of content.  ``enc_valid`` = (hv, wv) of the OUTPUT map: the encoders' stride-2 form (rpe_enc_conv_s2_v / _m96_v), whose
    ``stats`` records also cover the content only."""
    if enc_valid is not None:
        if valid is not None or stride != 2:
            raise _lib.RpeError('conv_fused: enc_valid is the stride-2 encoder form (not with valid=)')
        valid = enc_valid
    if isinstance(pc, PackedConvF16):                         # the kernel that belongs to the packing (what it refuses is an error, never another route)
        entry = pc.entry
    d, bias, stats = _conv_desc('conv_fused', x, pc, mode, dict(add=add, out=out, out2=out2, hidden=hidden, zgate=zgate, residual=residual),
                                _FUSED_RULES.get(mode, _PLAIN_RULES), scale, bias, stats, pre_norm, modes=_FUSED_MODES, tile_major=False,
                                kernel=(pc.kh, pc.kw), stride=stride, gate_channels=gate_channels, valid=valid)
    return _launch(_kind(entry, valid, enc_valid is not None), d, (x, pc, out, out2, add, hidden, zgate, scale, bias, residual, stats, pre_norm), out, prepare)


def _kind(entry, valid, enc=False):
    """The launch-list kind of ``entry``, or of its valid-extent form ``entry + '_v'`` (an entry point without one raises)."""
    if valid is None:
        return _lib.KIND_OF_ENTRY[entry]
    if enc:                                                   # the encoders' forms: their own entry points, every encoder epilogue
        if entry not in _lib.ENC_FORM:
            raise _lib.RpeError(f'{entry} has no encoder valid-extent form')
        return _lib.KIND_OF_ENTRY[_lib.ENC_FORM[entry]]
    if entry + '_v' not in _lib.KIND_OF_ENTRY:
        raise _lib.RpeError(f'{entry} has no valid-extent form')
    return _lib.KIND_OF_ENTRY[entry + '_v']


def _conv_desc(who, x, pc, mode, slices, rules, scale, bias, stats, pre_norm, *, modes, tile_major, kernel, stride=1, gate_channels=0, valid=None):
    """The ConvDesc of conv_fused / conv_wino after the checks they share -> (descriptor, the bias and the stats tensor it points to).
    ``slices``: descriptor field -> channel slice on the output map or None, checked against ``rules`` (as _PLAIN_RULES); ``modes``: the epilogues the kernel has; ``tile_major``: the layout of ``stats`` (conv_wino's TileMajorStats, or
    conv_stats_buffer's channel-major tensor); ``kernel`` = (kh, kw)."""
    d = _lib.ConvDesc() if valid is None else _lib.ConvDescV()
    b, cin, hh, ww = x.shape
    if valid is not None:
        d.h_valid, d.w_valid = _valid_extent(who, valid, hh // stride, ww // stride)
    cout = pc.cout
    if cin != pc.cin:
        raise _lib.RpeError(f'{who}: input has {cin} channels, weights expect {pc.cin}')
    if mode not in modes:
        raise _lib.RpeError(f'{who}: mode {mode} is not an epilogue of this kernel' + (' (LINEAR / RELU only)' if len(modes) == 2 else ''))
    d.x, d.x_batch_stride = _chan_slice(x, f'{who}: x')
    bias = pc.bias if isinstance(bias, str) else bias
    for name, t in (('bias', bias), ('scale', scale)):
        if t is not None:
            _f32(t, f'{who}: {name}', numel=cout)
    d.packed, d.bias, d.scale = ptr(pc.packed), ptr(bias), ptr(scale)
    for name, t in slices.items():
        rule, kind, required = rules.get(name, ('min', None, False))
        channels = {'cout': cout, 'gate': gate_channels, None: 0}[kind]
        if t is None:
            if required:
                raise _lib.RpeError(f'{who}: this epilogue needs {name}')
            continue                                          # (a fresh descriptor holds NULL and stride 0)
        if t.shape[0] != b or tuple(t.shape[2:]) != (hh // stride, ww // stride) or (rule == 'exact' and t.shape[1] != channels):
            raise _lib.RpeError(f'{who}: {name} has shape {tuple(t.shape)}')
        if t.shape[1] < channels:
            raise _lib.RpeError(f'{who}: {name} has too few channels ({t.shape[1]}, the epilogue writes or reads {channels})')
        p, s = _chan_slice(t, f'{who}: {name}')
        setattr(d, name, p); setattr(d, name + '_batch_stride', s)
    if stats is not None:
        if isinstance(stats, TileMajorStats) != tile_major:
            raise _lib.RpeError(f'{who}: stats must come from ' + ('conv_wino_stats_buffer (tile-major records)' if tile_major else
                                                                  'conv_stats_buffer (a channel-major tensor)'))
        if tile_major:
            stats = _f32(stats.tensor, f'{who}: stats', (b, lib().rpe_conv_wino_stats_tiles(hh, ww), cout, 3))
        else:
            d.stats_tiles = lib().rpe_conv_stats_tiles(cout, hh, ww, stride)
            _f32(stats, f'{who}: stats', (b, cout, d.stats_tiles, 3))
    if pre_norm is not None:
        _f32(pre_norm, f'{who}: pre_norm', (b, cin, 2))
    d.stats, d.pre_norm = ptr(stats), ptr(pre_norm)
    d.b, d.cin, d.cout, d.h, d.w, (d.kh, d.kw), d.mode, d.gate_channels, d.stride = b, cin, cout, hh, ww, kernel, mode, gate_channels, stride
    return d, bias, stats


def conv_direct(x, weight, bias=None, stride=1, padding=0, relu=False, out=None):
    """rpe_conv_direct: torch.nn.functional.conv2d(x, weight, bias, stride, padding) [+ ReLU] for ANY map size -- the route of the shapes
    the tuned kernels refuse (odd maps, rows that are not whole 16-byte quads).  x / out may be channel slices of NCHW buffers."""
    xp, xbs = _chan_slice(x, 'x')
    b, cin, hh, ww = x.shape
    w = _nchw(weight.detach().contiguous(), 'weight')
    cout, wcin, kh, kw = w.shape
    if wcin != cin:
        raise _lib.RpeError(f'conv_direct: input has {cin} channels, weight expects {wcin}')
    st = stride if isinstance(stride, int) else stride[0]
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    ho, wo = (hh + 2 * ph - kh) // st + 1, (ww + 2 * pw - kw) // st + 1
    if bias is not None:
        bias = bias.detach()
        _f32(bias, 'conv_direct: bias', numel=cout)
    if out is None:
        out = torch.empty(b, cout, ho, wo, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (b, cout, ho, wo):
        raise _lib.RpeError(f'conv_direct: out must be ({b},{cout},{ho},{wo})')
    op, obs = _chan_slice(out, 'out')
    check(lib().rpe_conv_direct(xp, xbs, ptr(w), ptr(bias), b, cin, cout, hh, ww, kh, kw, st, ph, pw, int(bool(relu)), op, obs, stream_ptr()),
          'rpe_conv_direct')
    return out


class PackedWino1d(_Packed):
    """Weights of a 1x5 / 5x1 stride-1 convolution transformed for rpe_conv_wino1d (U = G g along the taps, once per weight version)."""
    kernels, error = ((1, 5), (5, 1)), 'needs a (cout, cin % 4 == 0, 1, 5) or (.., 5, 1) weight'
    size, pack, entry = 'rpe_conv_wino1d_packed_floats', 'rpe_conv_wino1d_pack', 'rpe_conv_wino1d'

    @staticmethod
    def supported(weight, ww):
        return tuple(weight.shape[2:]) in ((1, 5), (5, 1)) and weight.shape[1] % 4 == 0 and ww % 4 == 0


def conv_wino1d(x, pw, mode, out, **kw):
    """rpe_conv_wino1d: conv_fused's operation (all four epilogue modes incl. the GRU gates) for 1x5 / 5x1 stride-1 convolutions
    by Winograd F(4,5) along the filter axis: 2.5x fewer matrix FLOPs.  Same keyword arguments as conv_fused (no scale /
    residual / stats / pre_norm)."""
    return conv_fused(x, pw, mode, out, entry=pw.entry, **kw)


class PackedWino1dX3(_Packed):
    """Weights of a 1x5 / 5x1 stride-1 convolution transformed and split three ways into bf16 for rpe_conv_wino1d_x3 (the labelled
    bf16x3 variant of rpe_conv_wino1d; conv_wino1d dispatches on the packing)."""
    kernels, error, in_bytes = ((1, 5), (5, 1)), 'needs a (cout, cin % 16 == 0, 1, 5) or (.., 5, 1) weight', True
    size, pack, entry = 'rpe_conv_wino1d_x3_packed_bytes', 'rpe_conv_wino1d_x3_pack', 'rpe_conv_wino1d_x3'

    @staticmethod
    def supported(weight, ww):
        return tuple(weight.shape[2:]) in ((1, 5), (5, 1)) and weight.shape[1] % 16 == 0 and ww % 4 == 0


class PackedWino(_Packed):
    """Weights of a 3x3 stride-1 convolution transformed for rpe_conv_wino (U = G g G^T, once per weight version)."""
    kernels, error = ((3, 3),), 'needs a (cout, cin % 4 == 0, 3, 3) weight'
    size, pack, entry = 'rpe_conv_wino_packed_floats', 'rpe_conv_wino_pack', 'rpe_conv_wino'

    @staticmethod
    def supported(weight, hh, ww):
        return tuple(weight.shape[2:]) == (3, 3) and weight.shape[1] % 4 == 0 and hh % 2 == 0 and ww % 2 == 0


class PackedWino24(_Packed):
    """Weights of a 3x3 stride-1 convolution for rpe_conv_wino24, Winograd F(2x4,3x3) (U = Gy g Gx^T in f64, rounded once).  conv_wino()
    runs the kernel that belongs to the packing; maps it refuses (``supported``) take PackedWino's F(2x2)."""
    kernels, error = ((3, 3),), 'needs a (cout, cin % 4 == 0, 3, 3) weight'
    size, pack, entry = 'rpe_conv_wino24_packed_floats', 'rpe_conv_wino24_pack', 'rpe_conv_wino24'

    @staticmethod
    def supported(weight, hh, ww):
        return tuple(weight.shape[2:]) == (3, 3) and weight.shape[1] % 4 == 0 and hh % 2 == 0 and ww % 4 == 0


class PackedWinoX3(_Packed):
    """Weights of a 3x3 stride-1 convolution for rpe_conv_wino_x3, the LABELLED bf16x3 variant of rpe_conv_wino: U = G g G^T in f32,
    then the exact three-way bf16 split.  conv_wino() takes either packing and runs the kernel that belongs to it."""
    kernels, error, in_bytes = ((3, 3),), 'needs a (cout, cin % 16 == 0, 3, 3) weight', True
    size, pack, entry = 'rpe_conv_wino_x3_packed_bytes', 'rpe_conv_wino_x3_pack', 'rpe_conv_wino_x3'

    @staticmethod
    def supported(weight, hh, ww):
        return tuple(weight.shape[2:]) == (3, 3) and weight.shape[1] % 16 == 0 and hh % 2 == 0 and ww % 4 == 0


def conv_wino(x, pw, mode, out, out2=None, scale=None, bias='packed', residual=None, stats=None, pre_norm=None, prepare=False, valid=None,
              enc_valid=None):
    """rpe_conv_wino: out = epilogue(conv3x3(x; pw) * scale + bias) by Winograd F(2x2,3x3) -- F(2x4,3x3) with a PackedWino24, the
    labelled bf16x3 variant with a PackedWinoX3; tensors are channel slices of NCHW buffers.  ``stats`` (conv_wino_stats_buffer) /
    ``pre_norm`` / ``residual`` / ``scale``: the encoders' epilogues, as conv_fused.  ``enc_valid`` = (hv, wv): the encoders' valid-extent
    form (rpe_enc_conv_wino_v / _wino24_v) -- ``valid``'s zero outside the content with every epilogue above, the records of ``stats`` over
    the content only, and ``pre_norm``'s normalised input zero outside it."""
    if enc_valid is not None:
        if valid is not None:
            raise _lib.RpeError('conv_wino: valid= and enc_valid= are two entry points')
        valid = enc_valid
    if (pw.kh, pw.kw) != (3, 3):                              # (a PackedConvF16 exists for other shapes too: those go through conv_fused)
        raise _lib.RpeError(f'conv_wino: needs the packing of a 3x3 weight, got {pw.kh}x{pw.kw}')
    d, bias, stats = _conv_desc('conv_wino', x, pw, mode, dict(out=out, out2=out2, residual=residual), _WINO_RULES, scale, bias, stats, pre_norm,
                                modes=(CONV_LINEAR, CONV_RELU), tile_major=True, kernel=(3, 3), valid=valid)
    return _launch(_kind(pw.entry, valid, enc_valid is not None), d, (x, pw, out, out2, scale, bias, residual, stats, pre_norm), out, prepare)


class TileMajorStats:
    """The (b, tiles, cout, 3) per-tile (count, mean, M2) records of rpe_conv_wino.  The layout is part of the TYPE, not an
    attribute a view or clone could drop: instnorm_finalize / instnorm_apply take either this (tile-major) or a plain
    (b, cout, tiles, 3) tensor (rpe_conv_fused's and rpe_stem_conv's channel-major records) and validate the shape for each."""

    def __init__(self, tensor):
        self.tensor = tensor

    @property
    def shape(self):
        return self.tensor.shape

    def cpu(self):
        return self.tensor.cpu()


def conv_wino_stats_buffer(b, cout, hh, ww, device):
    """Per-tile (count, mean, M2) records rpe_conv_wino fills when ``stats`` is given: TILE-MAJOR (b, tiles, cout, 3)."""
    return TileMajorStats(torch.empty(b, lib().rpe_conv_wino_stats_tiles(hh, ww), cout, 3, dtype=torch.float32, device=device))


def _stats_layout(stats, b, c, who):
    """(tensor, signed tile count for the C ABI: negative = tile-major) after validating the records' shape against (b, c)."""
    tile_major = isinstance(stats, TileMajorStats)
    t = stats.tensor if tile_major else stats
    if not (_is_f32(t) and t.dim() == 4 and t.shape[3] == 3):
        raise _lib.RpeError(f'{who}: stats must be a contiguous float32 4-D GPU tensor of (count, mean, M2) records')
    want = (b, t.shape[1], c) if tile_major else (b, c, t.shape[2])
    if tuple(t.shape[:3]) != want or t.shape[1 if tile_major else 2] < 1:
        raise _lib.RpeError(f'{who}: stats must be the (b,c,tiles,3) buffer of conv_fused / stem_conv or the TileMajorStats (b,tiles,c,3) of conv_wino; '
                            f'got {tuple(t.shape)} for b={b}, c={c}')
    return t, (-t.shape[1] if tile_major else t.shape[2])


def conv_stats_buffer(b, cout, hh, ww, device, stride=1):
    """Per-tile (count, mean, M2) records rpe_conv_fused fills when ``stats`` is given: (b, cout, tiles, 3); hh, ww = input map."""
    return torch.empty(b, cout, lib().rpe_conv_stats_tiles(cout, hh, ww, stride), 3, dtype=torch.float32, device=device)


def instnorm_finalize(stats, hw, eps=1e-5, channels=None):
    """(b,c,2) = (mean, 1/std) per plane from conv_fused's partial sums: the ``pre_norm`` argument of the next conv_fused.
    ``channels`` (optional) is checked against the records' channel axis."""
    b = stats.shape[0]
    c = stats.shape[2] if isinstance(stats, TileMajorStats) else stats.shape[1]
    if channels is not None and channels != c:
        raise _lib.RpeError(f'instnorm_finalize: records hold {c} channels, expected {channels}')
    t, tiles = _stats_layout(stats, b, c, 'instnorm_finalize')
    mi = torch.empty(b, c, 2, dtype=torch.float32, device=t.device)
    return _launch(_lib.OP_INSTNORM_FINALIZE, (ptr(t), tiles, b, c, hw, float(eps), ptr(mi)), (t, mi), mi)


def instnorm_apply(x, stats, eps=1e-5, relu=True, residual=None, out=None, residual_norm=None, residual_relu=True, valid=None):
    """Instance norm of x (b,c,h,w) from the partial sums of conv_fused(..., stats=stats): one read + one write pass.
    ``stats`` may also be the (b,c,2) result of instnorm_finalize on those sums (``eps`` is then already in it): the pass is then a
    pure stream with several workgroups per plane, the faster form behind large maps (the records are merged once, not per workgroup).
    ``residual_norm`` (b,c,2) from instnorm_finalize: the residual is a RAW convolution output, normalised (+ ReLU'd unless
    ``residual_relu=False``: a stride-2 block's shortcut has none) on the fly.
    ``valid`` = (hv, wv): x is a zero-padded map with hv x wv of content (rpe_instnorm_apply_v): the same bits inside, zero outside;
    ``stats`` are then the pairs of instnorm_finalize, or records, which are finalized first (over hv * wv pixels)."""
    _nchw(x, 'instnorm_apply: x')
    b, c, hh, ww = x.shape
    if isinstance(stats, torch.Tensor) and stats.dim() == 3:              # (mean, 1/std) pairs of instnorm_finalize: a pure streaming pass
        t, tiles = _f32(stats, 'instnorm_apply: stats (the moments of instnorm_finalize)', (b, c, 2)), 0
    else:
        t, tiles = _stats_layout(stats, b, c, 'instnorm_apply')
    if residual is not None and _nchw(residual, 'instnorm_apply: residual').shape != x.shape:
        raise _lib.RpeError('instnorm_apply: residual must have the shape of x')
    if residual_norm is not None:
        if residual is None:
            raise _lib.RpeError('instnorm_apply: residual_norm needs a residual')
        _f32(residual_norm, 'instnorm_apply: residual_norm', (b, c, 2))
    out = x if out is None else _nchw(out, 'instnorm_apply: out')
    flags = int(bool(relu)) | (0 if residual_relu or residual_norm is None else 2)
    if valid is not None:
        hv, wv = _valid_extent('instnorm_apply', valid, hh, ww)
        if tiles != 0:
            t = instnorm_finalize(stats, hv * wv, eps=eps, channels=c)
        return _launch(_lib.OP_INSTNORM_APPLY_V, (ptr(x), ptr(t), b, c, hh, ww, hv, wv, flags, ptr(residual), ptr(residual_norm), ptr(out)),
                       (x, t, residual, residual_norm, out), out)
    return _launch(_lib.OP_INSTNORM_APPLY, (ptr(x), ptr(t), tiles, b, c, hh * ww, float(eps), flags, ptr(residual), ptr(residual_norm), ptr(out)),
                   (x, t, residual, residual_norm, out), out)


class PackedStem(_Packed):
    """A (cout, cin, 7, 7) weight (cin 3: encoder stem, stride 2; cin 2: convf1, stride 1) in rpe_stem_conv's layout."""
    error = 'weight must be (64k, 2|3, 7, 7)'
    size, pack, entry = 'rpe_stem_packed_floats', 'rpe_stem_pack', 'rpe_stem_conv'

    def __init__(self, weight):
        super().__init__(weight)
        self.stride = 2 if self.cin == 3 else 1

    def _fits(self):
        return (self.kh, self.kw) == (7, 7) and self.cin in (2, 3) and self.cout % 64 == 0


def stem_conv(image, ps, bias=None, scale=None, relu=True, stats=False, div=255.0, mul=2.0, sub=1.0, out=None, prepare=False, valid=None):
    """conv7x7(mul * (image / div) - sub) * scale + bias [ReLU]; stride and channel counts come from ``ps``.
    Returns out, or (out, stats).  ``prepare=True`` (needs ``out``; stats = a caller-owned buffer or False): a launcher with ``.op``."""
    _nchw(image, 'stem_conv: image')
    b, c, hh, ww = image.shape
    if c != ps.cin:
        raise _lib.RpeError(f'stem_conv: image must have {ps.cin} channels')
    st_ = ps.stride
    if out is None:
        out = torch.empty(b, ps.cout, hh // st_, ww // st_, dtype=torch.float32, device=image.device)
    elif tuple(_nchw(out, 'stem_conv: out').shape) != (b, ps.cout, hh // st_, ww // st_):
        raise _lib.RpeError('stem_conv: out has the wrong shape')
    if isinstance(stats, torch.Tensor):             # a caller-owned (batch slice of a) statistics buffer
        st, stats = _f32(stats, 'stem_conv: stats', (b, ps.cout, lib().rpe_stem_tiles(hh, ww, st_), 3)), True
    else:
        st = torch.empty(b, ps.cout, lib().rpe_stem_tiles(hh, ww, st_), 3, dtype=torch.float32, device=image.device) if stats else None
    args = (ptr(image), b, c, hh, ww, st_, float(div), float(mul), float(sub), ptr(ps.packed), ps.cout, ptr(bias), ptr(scale), int(bool(relu)), ptr(out), ptr(st))
    if valid is not None:                           # (rpe_stem_conv_v: zero outside the valid extent of the output map)
        return _launch(_lib.OP_STEM_CONV_V, (*args, *_valid_extent('stem_conv', valid, hh // st_, ww // st_)), (image, ps, bias, scale, out, st), out, prepare)
    return _launch(_lib.OP_STEM_CONV, args, (image, ps, bias, scale, out, st),
                   (out, st) if stats and not prepare else out, prepare)


# ------------------------------------------------------------------------------------------------- weight heads
def unet_heads(inp1, inp2, hidden, context, params2d, params3d, out_size):
    """Both TinyUNet weight heads + resize + sigmoid (rpe_unet_heads).  hidden / context may be channel slices of (b,128,..)."""
    i1, i2 = _nchw(inp1, 'inp1'), _nchw(inp2, 'inp2')
    b, _, h8, w8 = i1.shape
    hp, hbs = _chan_slice(hidden, 'hidden')
    cp, cbs = _chan_slice(context, 'context')
    if tuple(i1.shape) != (b, 8, h8, w8) or tuple(i2.shape) != (b, 8, h8, w8) or tuple(hidden.shape) != (b, 128, h8, w8) or \
            tuple(context.shape) != (b, 128, h8, w8):
        raise _lib.RpeError('unet_heads: inp1, inp2 must be (b,8,h/8,w/8), hidden and context (b,128,h/8,w/8)')
    for name, t, cin in (('params2d', params2d, 264), ('params3d', params3d, 272)):
        _f32(t, f'unet_heads: {name} (the packed parameter blob of TinyUNet({cin}))', numel=lib().rpe_unet_params_floats(cin))
    nws = lib().rpe_unet_workspace_bytes(b, h8, w8)
    if nws == 0:
        raise _lib.RpeError('unet_heads: the 1/8 grid is too small for the valid convolutions (needs >= 44x44)')
    H, W = out_size
    ws = torch.empty(nws, dtype=torch.uint8, device=i1.device)
    o2, o3 = (torch.empty(b, 1, H, W, dtype=torch.float32, device=i1.device) for _ in range(2))
    check(lib().rpe_unet_heads(ptr(i1), ptr(i2), hp, cp, hbs, cbs, ptr(params2d), ptr(params3d), b, h8, w8, H, W, ptr(o2), ptr(o3), ptr(ws),
                               stream_ptr()), 'rpe_unet_heads')
    return o2, o3


# ------------------------------------------------------------------------------------------------- weight heads, training route
UNET_TRAIN_NPARAM, UNET_TRAIN_NNORM = 36, 5          # UT_NPARAM, UT_NNORM of csrc/unet_train_host.h


class UNetTrainCtx:
    """What unet_train_backward needs from unet_train_forward: the workspace with the saved activations, the argument arrays (and the
    tensors behind their pointers, kept alive) and the sizes."""
    __slots__ = ('ws', 'src', 'src_c', 'src_bs', 'nsrc', 'params', 'train_mask', 'n', 'cin', 'h8', 'w8', 'out_size', 'sigmoid', 'keep')


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def unet_train_forward(parts, params, norms, out_size, sigmoid=False):
    """One TinyUNet head in training form (rpe_unet_train_forward, csrc/unet_train.hip) -> (out (n,1,H,W), ctx for unet_train_backward).
    parts: 1..4 maps (n,c_k,h/8,w/8) whose channel concatenation is the head's input (each may be a channel slice of a wider buffer);
    params: the 36 parameter tensors in the order of csrc/unet_train_host.h; norms: 5 tuples (running_mean, running_var,
    num_batches_tracked or None, momentum, eps, training) -- encoder stages, then decoder stages.  Norms in training mode use the batch
    statistics and have their running statistics updated in place, as F.batch_norm(training=True) does."""
    if not 1 <= len(parts) <= 4 or len(params) != UNET_TRAIN_NPARAM or len(norms) != UNET_TRAIN_NNORM:
        raise _lib.RpeError('unet_train_forward: expected 1..4 input parts, 36 parameter tensors and 5 norms')
    sl = [_chan_slice(t, f'parts[{k}]') for k, t in enumerate(parts)]
    n, _, h8, w8 = parts[0].shape
    if any(tuple(t.shape[2:]) != (h8, w8) or t.shape[0] != n for t in parts):
        raise _lib.RpeError('unet_train_forward: the input parts must share batch and map size')
    cin = sum(t.shape[1] for t in parts)
    L = lib()
    for k, t in enumerate(params):
        _f32(t, f'unet_train_forward: params[{k}] (of TinyUNet({cin}), in the documented order)',
             numel=L.rpe_unet_train_grad_offset(cin, k + 1) - L.rpe_unet_train_grad_offset(cin, k))
    mask = 0
    for k, (rm, rv, nbt, momentum, eps, training) in enumerate(norms):
        if rm is None or rv is None or momentum is None:
            raise _lib.RpeError('unet_train_forward: the norms must track running statistics with a fixed momentum')
        for what, t in (('running_mean', rm), ('running_var', rv)):
            _f32(t, f'unet_train_forward: norms[{k}] {what}')
        if nbt is not None and not (nbt.is_cuda and nbt.dtype == torch.int64):
            raise _lib.RpeError(f'unet_train_forward: norms[{k}] num_batches_tracked must be an int64 GPU tensor')
        mask |= int(bool(training)) << k
    H, W = out_size
    nws = L.rpe_unet_train_workspace_bytes(n, cin, h8, w8, H, W)
    if nws == 0:
        raise _lib.RpeError('unet_train_forward: unsupported size (the 1/8 grid must be at least 44x44, the channel counts multiples of 8)')
    c = UNetTrainCtx()
    c.ws = torch.empty(nws, dtype=torch.uint8, device=parts[0].device)
    c.src = (ctypes.c_void_p * len(parts))(*[p.value for p, _ in sl])
    c.src_c = (ctypes.c_int * len(parts))(*[t.shape[1] for t in parts])
    c.src_bs = (ctypes.c_longlong * len(parts))(*[bs for _, bs in sl])
    c.nsrc, c.params, c.train_mask = len(parts), _ptr_array(params), mask
    c.n, c.cin, c.h8, c.w8, c.out_size, c.sigmoid = n, cin, h8, w8, (H, W), int(bool(sigmoid))
    c.keep = (tuple(parts), tuple(params))
    out = torch.empty(n, 1, H, W, dtype=torch.float32, device=parts[0].device)
    rms, rvs, nbts = (_ptr_array([nm[k] for nm in norms]) for k in range(3))
    mom = (ctypes.c_float * UNET_TRAIN_NNORM)(*[float(nm[3]) for nm in norms])
    eps = (ctypes.c_float * UNET_TRAIN_NNORM)(*[float(nm[4]) for nm in norms])
    check(L.rpe_unet_train_forward(c.src, c.src_c, c.src_bs, c.nsrc, c.params, rms, rvs, nbts, mom, eps, mask, n, h8, w8, H, W, c.sigmoid,
                                   ptr(out), ptr(c.ws), stream_ptr()), 'rpe_unet_train_forward')
    return out, c


def unet_train_backward(grad_out, out, ctx, input_grad=False):
    """Backward of unet_train_forward (rpe_unet_train_backward) -> (the parameter gradients as one blob in the params order: tensor k
    at ``unet_train_grad_offsets(cin)[k]``, gradient of the concatenated input (n,cin,h/8,w/8) or None)."""
    c = ctx
    H, W = c.out_size
    g = _nchw(grad_out, 'grad_out')
    if tuple(g.shape) != (c.n, 1, H, W) or tuple(_nchw(out, 'out').shape) != (c.n, 1, H, W):
        raise _lib.RpeError('unet_train_backward: grad_out and out must be (n,1,H,W)')
    L = lib()
    blob = torch.empty(L.rpe_unet_train_grad_floats(c.cin), dtype=torch.float32, device=g.device)
    gin = torch.empty(c.n, c.cin, c.h8, c.w8, dtype=torch.float32, device=g.device) if input_grad else None
    check(L.rpe_unet_train_backward(ptr(g), ptr(out), c.src, c.src_c, c.src_bs, c.nsrc, c.params, c.train_mask, c.n, c.h8, c.w8, H, W, c.sigmoid,
                                    ptr(blob), ptr(gin), ptr(c.ws), stream_ptr()), 'rpe_unet_train_backward')
    return blob, gin


def _unet_train_ws_names():
    names = []
    for i in range(3):
        names += [f'{k}.{i}' for k in ('a1', 'r1', 'g_r1', 'skip', 'g_skip') + (('pool', 'g_pool') if i < 2 else ())] + [f'mean.{i}', f'invstd.{i}']
    for j in range(2):
        names += [f'{k}.{j}' for k in ('up', 'g_up', 'r', 'nrm', 'g_nrm', 'dout', 'g_dout')] + [f'mean.{3 + j}', f'invstd.{3 + j}']
    return tuple(names + ['hm', 'g_hm', 'wpart'])


UNET_TRAIN_WS_NAMES = _unet_train_ws_names()         # the buffers of the workspace in index order (UT_NBUF of csrc/unet_train_host.h)


def unet_train_workspace_views(ctx):
    """The buffers of ``ctx.ws`` by name (UNET_TRAIN_WS_NAMES; '<field>.<stage>' of UtPlan, norms 0..4) as tensor views, located by
    rpe_unet_train_workspace_offset / _extent: maps (n,c,h,w) float32, mean / invstd (c,), 'wpart' (32, largest weight) float64.  The
    forward fills the saved activations, the backward the g_* buffers (some in place: see csrc/unet_train.hip)."""
    L = lib()
    base = (-ctx.ws.data_ptr()) % 256                 # the library rounds the pointer up to 256 bytes
    views, ext = {}, (ctypes.c_int * 4)()
    for k, name in enumerate(UNET_TRAIN_WS_NAMES):
        off = L.rpe_unet_train_workspace_offset(ctx.n, ctx.cin, ctx.h8, ctx.w8, k)
        check(L.rpe_unet_train_workspace_extent(ctx.n, ctx.cin, ctx.h8, ctx.w8, k, ext), 'rpe_unet_train_workspace_extent')
        rows, c, h, w = ext
        if name == 'wpart':
            views[name] = ctx.ws[base + 4 * off:base + 4 * off + 8 * rows * c].view(torch.float64).view(rows, c)
        else:
            v = ctx.ws[base + 4 * off:base + 4 * off + 4 * rows * c * h * w].view(torch.float32)
            views[name] = v.view(c) if name.startswith(('mean', 'invstd')) else v.view(rows, c, h, w)
    return views


def unet_train_grad_offsets(cin):
    """First float of each of the 36 parameter gradients in unet_train_backward's blob, and the blob's size as the 37th entry."""
    L = lib()
    return [L.rpe_unet_train_grad_offset(cin, k) for k in range(UNET_TRAIN_NPARAM + 1)]


# ------------------------------------------------------------------------------------------------- backward of RAFT's output heads
# (this and the next two sections: one kernel per wrapper; raft_grad.py composes them into the tail's, the update step's and the pass's backward)
def upsample_convex_backward(grad_up, flow, mask):
    """rpe_upsample_convex_backward: (d_flow (b,2,h8,w8), d_mask (b,576,h8,w8)) of ``upsample_convex(flow, mask)`` from grad_up
    (b,2,8 h8,8 w8); ``mask`` = the logits as the forward read them.  Bit-identical from run to run."""
    fl, mk, gu = _nchw(flow, 'flow'), _nchw(mask, 'mask'), _nchw(grad_up, 'grad_up')
    b, _, h8, w8 = fl.shape
    if tuple(fl.shape) != (b, 2, h8, w8) or tuple(mk.shape) != (b, 576, h8, w8) or tuple(gu.shape) != (b, 2, 8 * h8, 8 * w8):
        raise _lib.RpeError('upsample_convex_backward: flow (b,2,h8,w8), mask (b,576,h8,w8) and grad_up (b,2,8 h8,8 w8) expected')
    d_flow, d_mask = torch.empty_like(fl), torch.empty_like(mk)
    check(lib().rpe_upsample_convex_backward(ptr(gu), ptr(fl), ptr(mk), b, h8, w8, ptr(d_flow), ptr(d_mask), stream_ptr()),
          'rpe_upsample_convex_backward')
    return d_flow, d_mask


def conv_bwd_weight(x, dy, kernel, scale=1.0, bias=True):
    """rpe_conv_bwd_weight: (dW (cout,cin,kh,kw), db (cout) or None) of a stride-1 'same' convolution with ``kernel`` = (3,3), (1,1), (1,5), (5,1) or (7,7)
    from its input x (b,cin,h,w) and the gradient dy (b,cout,h,w) of its output, at any map size; both may be channel slices.  On the f32 matrix
    cores, K = b h w split by a rule of the shapes alone: bit-identical from run to run.  ``scale`` multiplies both results."""
    xp, xbs = _chan_slice(x, 'conv_bwd_weight: x')
    dp, dbs = _chan_slice(dy, 'conv_bwd_weight: dy')
    b, cin, hh, ww = x.shape
    cout = dy.shape[1]
    kh, kw = kernel
    if tuple(dy.shape) != (b, cout, hh, ww):
        raise _lib.RpeError(f'conv_bwd_weight: dy {tuple(dy.shape)} does not match x {tuple(x.shape)}')
    nws = lib().rpe_conv_bwd_weight_workspace_bytes(b, cin, cout, hh, ww, kh, kw)
    if nws == 0:
        raise _lib.RpeError(f'conv_bwd_weight: unsupported shape (kernel {kh}x{kw}; 3x3, 1x1, 1x5, 5x1 and 7x7, non-empty tensors)')
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    dw = torch.empty(cout, cin, kh, kw, dtype=torch.float32, device=x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if bias else None
    check(lib().rpe_conv_bwd_weight(xp, xbs, dp, dbs, b, cin, cout, hh, ww, kh, kw, float(scale), ptr(dw), ptr(db), ptr(ws), stream_ptr()),
          'rpe_conv_bwd_weight')
    return dw, db


def conv3x3_to2_bwd_data(dy, weight, act=None, out=None):
    """rpe_conv3x3_to2_bwd_data: the data gradient of ``conv3x3_to2`` (weight (2,c,3,3)) from dy (b,2,h,w), times [act > 0] when ``act``
    (b,c,h,w) -- the ReLU output that was the layer's input -- is given; ``out`` may be a channel slice."""
    dp, dbs = _chan_slice(dy, 'conv3x3_to2_bwd_data: dy')
    b, two, hh, ww = dy.shape
    w = _nchw(weight.detach() if weight.requires_grad else weight, 'conv3x3_to2_bwd_data: weight')
    c = w.shape[1]
    if two != 2 or tuple(w.shape) != (2, c, 3, 3):
        raise _lib.RpeError('conv3x3_to2_bwd_data: dy must be (b,2,h,w) and weight (2,c,3,3)')
    if out is None:
        out = torch.empty(b, c, hh, ww, dtype=torch.float32, device=dy.device)
    ap, abs_ = (None, 0) if act is None else _chan_slice(act, 'conv3x3_to2_bwd_data: act')
    for name, t in (('act', act), ('out', out)):
        if t is not None and tuple(t.shape) != (b, c, hh, ww):
            raise _lib.RpeError(f'conv3x3_to2_bwd_data: {name} must be ({b},{c},{hh},{ww})')
    op, obs = _chan_slice(out, 'conv3x3_to2_bwd_data: out')
    check(lib().rpe_conv3x3_to2_bwd_data(dp, dbs, ptr(w), ap, abs_, b, c, hh, ww, op, obs, stream_ptr()), 'rpe_conv3x3_to2_bwd_data')
    return out


def _same_slices(who, **named):
    """[pointer, batch stride, ...] of equally shaped channel slices -> (flat list, (b, c, h, w))."""
    shape, sl = None, []
    for name, t in named.items():
        sl += _chan_slice(t, f'{who}: {name}')
        if shape is None:
            shape = tuple(t.shape)
        elif tuple(t.shape) != shape:
            raise _lib.RpeError(f'{who}: {name} has shape {tuple(t.shape)}, expected {shape}')
    return sl, shape


def relu_backward(grad, act, out=None):
    """rpe_relu_backward: out = act > 0 ? grad : 0 on channel slices (default: in place on ``grad``)."""
    out = grad if out is None else out
    sl, (b, c, hh, ww) = _same_slices('relu_backward', grad=grad, act=act, out=out)
    check(lib().rpe_relu_backward(*sl[:4], b, c, hh * ww, *sl[4:], stream_ptr()), 'rpe_relu_backward')
    return out


def sum_groups(parts, bias=None, relu=False, out=None):
    """rpe_sum_groups: act(sum_g parts[g] + bias[c]) for parts (groups,b,c,h,w), added in group order in f64 -> (b,c,h,w) (``out`` may be a
    channel slice)."""
    if not (_is_f32(parts) and parts.dim() == 5):
        raise _lib.RpeError('sum_groups: parts must be a contiguous float32 (groups,b,c,h,w) GPU tensor')
    _on_current_device(parts, 'sum_groups: parts')
    groups, b, c, hh, ww = parts.shape
    if bias is not None:
        _f32(bias, 'sum_groups: bias', numel=c)
    if out is None:
        out = torch.empty(b, c, hh, ww, dtype=torch.float32, device=parts.device)
    elif tuple(out.shape) != (b, c, hh, ww):
        raise _lib.RpeError(f'sum_groups: out must be ({b},{c},{hh},{ww})')
    op, obs = _chan_slice(out, 'sum_groups: out')
    check(lib().rpe_sum_groups(ptr(parts), groups, b, c, hh * ww, ptr(bias), int(bool(relu)), op, obs, stream_ptr()), 'rpe_sum_groups')
    return out


# ------------------------------------------------------------------------------------------------- backward of RAFT's update block
def gru_gates_zr_recompute(zr_pre, h, z, r, rh):
    """rpe_gru_gates_zr_recompute: z = s(zr_pre[:, :c]), r = s(zr_pre[:, c:]), rh = r h from the pre-activations (b,2c,h,w; bias added) -- the
    gates with everything their adjoints read kept.  Channel slices."""
    zp, zbs = _chan_slice(zr_pre, 'gru_gates_zr_recompute: zr_pre')
    sl, (b, c, hh, ww) = _same_slices('gru_gates_zr_recompute', h=h, z=z, r=r, rh=rh)
    if tuple(zr_pre.shape) != (b, 2 * c, hh, ww):
        raise _lib.RpeError(f'gru_gates_zr_recompute: zr_pre must be ({b},{2 * c},{hh},{ww})')
    check(lib().rpe_gru_gates_zr_recompute(zp, zbs, *sl[:2], b, c, hh * ww, *sl[2:], stream_ptr()), 'rpe_gru_gates_zr_recompute')
    return z, r, rh


def gru_gates_h_recompute(q_pre, z, h, q, h_new):
    """rpe_gru_gates_h_recompute: q = tanh(q_pre), h_new = (1 - z) h + z q.  Channel slices."""
    sl, (b, c, hh, ww) = _same_slices('gru_gates_h_recompute', q_pre=q_pre, z=z, h=h, q=q, h_new=h_new)
    check(lib().rpe_gru_gates_h_recompute(*sl[:6], b, c, hh * ww, *sl[6:], stream_ptr()), 'rpe_gru_gates_h_recompute')
    return q, h_new


def gru_gates_zq_backward(d_h_new, h, z, q, d_z_pre, d_q_pre, d_h):
    """rpe_gru_gates_zq_backward, the adjoint of one GRU half's blend h' = (1 - z) h + z q from d_h_new and the post-activation z, q:
    d_z_pre = d (q - h) z (1 - z), d_q_pre = d z (1 - q^2), d_h = d (1 - z) (the direct term).  Channel slices (d_z_pre: e.g. the first half of
    the stacked z | r buffer); the outputs must not overlap the inputs."""
    sl, (b, c, hh, ww) = _same_slices('gru_gates_zq_backward', d_h_new=d_h_new, h=h, z=z, q=q, d_z_pre=d_z_pre, d_q_pre=d_q_pre, d_h=d_h)
    check(lib().rpe_gru_gates_zq_backward(*sl[:8], b, c, hh * ww, *sl[8:], stream_ptr()), 'rpe_gru_gates_zq_backward')
    return d_z_pre, d_q_pre, d_h


def gru_gates_r_backward(d_rh, h, r, d_h_in, d_r_pre, d_h_out):
    """rpe_gru_gates_r_backward, once convq's data gradient d_rh = d loss / d (r h) is known: d_r_pre = d_rh h r (1 - r), d_h_out = d_h_in +
    d_rh r.  d_h_out may be d_h_in or d_rh."""
    sl, (b, c, hh, ww) = _same_slices('gru_gates_r_backward', d_rh=d_rh, h=h, r=r, d_h_in=d_h_in, d_r_pre=d_r_pre, d_h_out=d_h_out)
    check(lib().rpe_gru_gates_r_backward(*sl[:8], b, c, hh * ww, *sl[8:], stream_ptr()), 'rpe_gru_gates_r_backward')
    return d_r_pre, d_h_out


# ------------------------------------------------------------------------------------------------- backward of the correlation
def corr_grad_levels(h8, w8, levels=4):
    """[(h_l, w_l)] of the pyramid's levels (h8 >> l, w8 >> l): a row of the gradient volume G holds them one after the other."""
    return [(h8 >> l, w8 >> l) for l in range(levels)]


def corr_grad_volume(b, h8, w8, levels=4, device='cuda'):
    """The zero-filled gradient volume G (b, h8 w8, S), S = sum_l h_l w_l, of ops.corr_lookup_backward / corr_build_backward: d loss / d pyramid,
    row p = the levels' maps of query p one after the other, each row-major.  S h8 w8 4 bytes per pair: 139 MB at 640 x 512, 2.2 GB at
    1280 x 1024."""
    n = lib().rpe_corr_grad_volume_floats(b, h8, w8, levels)
    if n == 0:
        raise _lib.RpeError(f'corr_grad_volume: unsupported geometry ({b} x {h8} x {w8}, {levels} levels: every level must be at least 2 x 2)')
    return torch.zeros(b, h8 * w8, n // (b * h8 * w8), dtype=torch.float32, device=device)


def _grad_volume(who, G, b, h8, w8, levels):
    n = lib().rpe_corr_grad_volume_floats(b, h8, w8, levels)
    if n == 0:
        raise _lib.RpeError(f'{who}: unsupported geometry ({b} x {h8} x {w8}, {levels} levels: every level must be at least 2 x 2)')
    if not (_is_f32(G) and tuple(G.shape) == (b, h8 * w8, n // (b * h8 * w8))):
        raise _lib.RpeError(f'{who}: G must be a contiguous float32 ({b},{h8 * w8},{n // (b * h8 * w8)}) GPU tensor (ops.corr_grad_volume)')
    _on_current_device(G, f'{who}: G')


def corr_lookup_backward(coords, d_corr, G, radius=4):
    """rpe_corr_lookup_backward: G += the adjoint of one window lookup at ``coords`` (b,2,h8,w8) from ``d_corr`` (b, levels 81, h8, w8), the
    gradient of the looked-up window (raft_grad.update_step_backward's ``ret_d_corr``).  G: ops.corr_grad_volume's layout, zero-filled by the caller
    before the first call; calls accumulate in stream order.  The forward's own taps and fractions, cells outside a level dropped; one wave
    owns a query's row, no atomics: bit-identical from run to run, a row's bits independent of the batch.  Nothing goes into the coordinates
    (upstream detaches them).  -> G."""
    who = 'corr_lookup_backward'
    co, dc = _nchw(coords, f'{who}: coords'), _nchw(d_corr, f'{who}: d_corr')
    b, two, h8, w8 = co.shape
    win2 = (2 * radius + 1) ** 2
    levels = dc.shape[1] // win2
    if two != 2 or radius != 4 or levels < 1 or tuple(dc.shape) != (b, levels * win2, h8, w8):
        raise _lib.RpeError(f'{who}: coords must be (b,2,h8,w8) and d_corr (b, levels 81, h8, w8) of the same maps (radius 4)')
    _grad_volume(who, G, b, h8, w8, levels)
    check(lib().rpe_corr_lookup_backward(ptr(co), ptr(dc), b, h8, w8, levels, radius, ptr(G), stream_ptr()), 'rpe_corr_lookup_backward')
    return G


def corr_build_backward(G, fmap1, fmap2, levels=4, ret_df2cat=False):
    """rpe_corr_build_backward: (d_fmap1, d_fmap2), each (b,c,h8,w8), of the pyramid build from the gradient volume G (ops.corr_grad_volume's
    layout) and the f32 feature maps the pass correlated.  Pooling is linear, so with F2cat (c x S) = fmap2 followed by its 2x2-pooled copies
    (floor): d_fmap1 = F2cat G^T / sqrt(c), dF2cat = fmap1 G / sqrt(c), and d_fmap2 = the pool adjoints of dF2cat's level blocks applied from
    level 3 down to 0.  GEMMs on the f32 matrix cores, the contraction split by the shape alone and added in f64 in a second pass; no float
    atomics, bit-identical from run to run, a row's bits independent of the batch.  c: a multiple of 4 up to 256.  ``ret_df2cat``: dF2cat
    (b,c,S) as a third result.  Memory: G itself is S h8 w8 4 bytes per pair (139 MB at 640 x 512, 2.2 GB at 1280 x 1024)."""
    who = 'corr_build_backward'
    f1, f2 = _nchw(fmap1, f'{who}: fmap1'), _nchw(fmap2, f'{who}: fmap2')
    b, c, h8, w8 = f1.shape
    if f2.shape != f1.shape:
        raise _lib.RpeError(f'{who}: fmap1 {tuple(f1.shape)} and fmap2 {tuple(f2.shape)} must have one shape')
    _grad_volume(who, G, b, h8, w8, levels)
    nws = lib().rpe_corr_build_backward_workspace_bytes(b, c, h8, w8, levels)
    if nws == 0:
        raise _lib.RpeError(f'{who}: unsupported shape (c = {c}: a multiple of 4 up to 256)')
    ws = torch.empty(nws, dtype=torch.uint8, device=f1.device)
    d1, d2 = torch.empty_like(f1), torch.empty_like(f2)
    dcat = torch.empty(b, c, G.shape[2], dtype=torch.float32, device=f1.device) if ret_df2cat else None
    check(lib().rpe_corr_build_backward(ptr(G), ptr(f1), ptr(f2), b, c, h8, w8, levels, ptr(d1), ptr(d2), ptr(dcat), ptr(ws), stream_ptr()),
          'rpe_corr_build_backward')
    return (d1, d2, dcat) if ret_df2cat else (d1, d2)


# ------------------------------------------------------------------------------------------------- backward of the encoders
# (one kernel per wrapper, csrc/encoder_backward.hip; raft_grad.py composes them into residual_block_backward and encoder_backward)
def _s2_out(hi, wi, k):
    return (hi + 2 * (k // 2) - k) // 2 + 1, (wi + 2 * (k // 2) - k) // 2 + 1


def conv_s2_bwd_weight(x, dy, k, scale=1.0, bias=True):
    """rpe_conv_s2_bwd_weight: (dW (cout,cin,k,k), db (cout) or None) of a STRIDE-2 convolution with kernel k = 3 (padding 1), 1 (padding 0)
    or 7 (padding 3) from its input x (b,cin,hi,wi) and the gradient dy (b,cout,ho,wo) of its output, at any map size; both may be channel
    slices.  conv_bwd_weight's GEMM and split of K = b ho wo: bit-identical from run to run.  ``scale`` multiplies both results."""
    xp, xbs = _chan_slice(x, 'conv_s2_bwd_weight: x')
    dp, dbs = _chan_slice(dy, 'conv_s2_bwd_weight: dy')
    b, cin, hi, wi = x.shape
    cout, ho, wo = dy.shape[1:]
    if k not in (1, 3, 7) or tuple(dy.shape) != (b, cout, *_s2_out(hi, wi, k)):
        raise _lib.RpeError(f'conv_s2_bwd_weight: kernel {k} (3, 1 or 7) and dy {tuple(dy.shape)} do not match x {tuple(x.shape)} at stride 2')
    nws = lib().rpe_conv_s2_bwd_weight_workspace_bytes(b, cin, cout, hi, wi, ho, wo, k)
    if nws == 0:
        raise _lib.RpeError('conv_s2_bwd_weight: unsupported shape (non-empty tensors)')
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    dw = torch.empty(cout, cin, k, k, dtype=torch.float32, device=x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if bias else None
    check(lib().rpe_conv_s2_bwd_weight(xp, xbs, dp, dbs, b, cin, cout, hi, wi, ho, wo, k, float(scale), ptr(dw), ptr(db), ptr(ws), stream_ptr()),
          'rpe_conv_s2_bwd_weight')
    return dw, db


def conv_s2_bwd_data(dy, weight, size, out=None):
    """rpe_conv_s2_bwd_data: dx (b,cin,hi,wi), ``size`` = (hi, wi), of a stride-2 convolution with weight (cout,cin,k,k), k = 3 (padding 1) or
    1 (padding 0), from dy (b,cout,ho,wo).  Gather form, summed in f64; exact zeros where no tap reaches; ``out`` may be a channel slice."""
    dp, dbs = _chan_slice(dy, 'conv_s2_bwd_data: dy')
    w = _nchw(weight.detach(), 'conv_s2_bwd_data: weight')
    b, cout, ho, wo = dy.shape
    cin, k = w.shape[1], w.shape[2]
    hi, wi = size
    if tuple(w.shape) != (cout, cin, k, k) or k not in (1, 3) or (ho, wo) != _s2_out(hi, wi, k):
        raise _lib.RpeError(f'conv_s2_bwd_data: weight {tuple(w.shape)} (3x3 or 1x1) and dy {tuple(dy.shape)} do not give a {hi} x {wi} input at stride 2')
    if out is None:
        out = torch.empty(b, cin, hi, wi, dtype=torch.float32, device=dy.device)
    elif tuple(out.shape) != (b, cin, hi, wi):
        raise _lib.RpeError(f'conv_s2_bwd_data: out must be ({b},{cin},{hi},{wi})')
    op, obs = _chan_slice(out, 'conv_s2_bwd_data: out')
    check(lib().rpe_conv_s2_bwd_data(dp, dbs, ptr(w), b, cin, cout, hi, wi, ho, wo, k, op, obs, stream_ptr()), 'rpe_conv_s2_bwd_data')
    return out


def bn_frozen_backward(dy, z, gamma, conv_bias, mean, var, eps, dz=None):
    """rpe_bn_frozen_backward: the adjoint of y = s (z + conv_bias - mean) + beta, s = gamma / sqrt(var + eps), on running statistics, from dy
    (behind the ReLU mask) and the raw convolution output z -> (dz = s dy, d_gamma, d_beta, d_conv_bias); ``dz`` may be given (dy itself: in
    place).  The per-channel sums run in f64 under a fixed tree."""
    who = 'bn_frozen_backward'
    dz = torch.empty(dy.shape, dtype=torch.float32, device=dy.device) if dz is None else dz
    sl, (b, c, hh, ww) = _same_slices(who, dy=dy, z=z, dz=dz)
    for name, t in (('gamma', gamma), ('mean', mean), ('var', var)) + ((('conv_bias', conv_bias),) if conv_bias is not None else ()):
        _f32(t, f'{who}: {name}', numel=c)
    nws = lib().rpe_bn_frozen_backward_workspace_bytes(b, c, hh * ww)
    if nws == 0:
        raise _lib.RpeError(f'{who}: empty tensors')
    ws = torch.empty(nws, dtype=torch.uint8, device=dy.device)
    dg, dbeta, dcb = (torch.empty(c, dtype=torch.float32, device=dy.device) for _ in range(3))
    check(lib().rpe_bn_frozen_backward(*sl[:4], ptr(gamma), ptr(conv_bias), ptr(mean), ptr(var), float(eps), b, c, hh * ww, ptr(dg),
                                       ptr(dbeta), ptr(dcb), *sl[4:], ptr(ws), stream_ptr()), 'rpe_bn_frozen_backward')
    return dz, dg, dbeta, dcb


def instnorm_backward(dy, z, eps=1e-5, dz=None):
    """rpe_instnorm_backward: dz = (dy - mean(dy) - xh mean(dy xh)) / sigma per plane of an instance norm without affine parameters, from dy
    (behind the ReLU mask) and the norm's input z; plane moments in f64.  ``dz`` defaults to a new tensor (dy itself: in place)."""
    dz = torch.empty(dy.shape, dtype=torch.float32, device=dy.device) if dz is None else dz
    sl, (b, c, hh, ww) = _same_slices('instnorm_backward', dy=dy, z=z, dz=dz)
    check(lib().rpe_instnorm_backward(*sl[:4], b, c, hh * ww, float(eps), *sl[4:], stream_ptr()), 'rpe_instnorm_backward')
    return dz


def split_act_backward(grad, act, half, out=None):
    """rpe_split_act_backward: grad (1 - act^2) on channels [0, half) and act > 0 ? grad : 0 on the rest, ``act`` = the activated output
    (tanh | ReLU: the context encoder's net | inp); default in place on ``grad``."""
    out = grad if out is None else out
    sl, (b, c, hh, ww) = _same_slices('split_act_backward', grad=grad, act=act, out=out)
    if not 0 <= half <= c:
        raise _lib.RpeError('split_act_backward: 0 <= half <= channels expected')
    check(lib().rpe_split_act_backward(*sl[:4], b, c, half, hh * ww, *sl[4:], stream_ptr()), 'rpe_split_act_backward')
    return out


# ------------------------------------------------------------------------------------------------ the training step's update (csrc/optim.hip)
def optim_chunk():
    """RPE_OPTIM_CHUNK of the loaded library: the elements of one chunk (one workgroup) of rpe_grad_norm / rpe_adamw_step."""
    return int(lib().rpe_optim_chunk_floats())


def optim_chunk_offsets(numels):
    """rpe_optim_chunk_offsets: the chunk list of tensors of ``numels`` elements as a ctypes array of _lib.OptimChunk (host memory); sizes
    below 1 or from 2^31 on are refused there."""
    n = len(numels)
    sizes = (ctypes.c_longlong * max(1, n))(*numels)
    count = lib().rpe_optim_chunk_offsets(sizes, n, None, 0)
    if count < 0:
        check(count, 'rpe_optim_chunk_offsets')
    out = (_lib.OptimChunk * max(1, count))()
    check(min(0, lib().rpe_optim_chunk_offsets(sizes, n, out, count)), 'rpe_optim_chunk_offsets')
    return out, count


class OptimTable:
    """The device-resident table and chunk list of rpe_grad_norm / rpe_adamw_step with their workspace.  ``set(rows)`` takes the step's
    (param, grad, exp_avg, exp_avg_sq) tensors -- float32, contiguous, on the current device -- and uploads table and chunk list only when a
    pointer or a size differs from what the device holds: from a pinned staging buffer of its own per upload, asynchronously on the current
    stream (torch's pinned allocator keeps a staging buffer from being handed out again before its copy has run, so the host never waits
    and never rewrites bytes in flight).  One table serves one stream."""

    def __init__(self):
        self.key, self.n_rows, self.n_chunks, self.numels = None, 0, 0, None
        self.buf = self.workspace = None
        self.chunks_at = 0
        self._host_chunks = None
        self.uploads = 0

    def set(self, rows):
        key = tuple((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()) for p, g, m, v in rows)
        if key == self.key:
            return self
        for p, g, m, v in rows:
            for t in (g, m, v):
                if not (_is_f32(t) and t.numel() == p.numel()):
                    raise _lib.RpeError('OptimTable: gradients and moments must be contiguous float32 GPU tensors of their parameter\'s size')
            if not _is_f32(p):
                raise _lib.RpeError('OptimTable: parameters must be contiguous float32 GPU tensors')
            _on_current_device(p, 'OptimTable: parameter')
        numels = tuple(k[4] for k in key)
        if numels != self.numels:
            self._host_chunks, self.n_chunks = optim_chunk_offsets(numels)
            self.numels = numels
        n = len(rows)
        table = (_lib.OptimRow * max(1, n))(*[_lib.OptimRow(*k) for k in key])
        row_bytes, chunk_bytes = n * ctypes.sizeof(_lib.OptimRow), self.n_chunks * ctypes.sizeof(_lib.OptimChunk)
        self.chunks_at = (row_bytes + 15) // 16 * 16
        total = self.chunks_at + chunk_bytes
        if n:
            device = rows[0][0].device
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            ctypes.memmove(host.data_ptr(), table, row_bytes)
            ctypes.memmove(host.data_ptr() + self.chunks_at, self._host_chunks, chunk_bytes)
            if self.buf is None or self.buf.numel() < total or self.buf.device != device:
                self.buf = torch.empty(total, dtype=torch.uint8, device=device)
            self.buf[:total].copy_(host, non_blocking=True)
            need = int(lib().rpe_optim_workspace_bytes(self.n_chunks))
            if self.workspace is None or self.workspace.numel() < need or self.workspace.device != device:
                self.workspace = torch.zeros(need, dtype=torch.uint8, device=device)      # (the tickets start at zero; the kernels count them back)
            self.uploads += 1
        self.key, self.n_rows = key, n
        return self

    def _args(self):
        return (ctypes.c_void_p(self.buf.data_ptr()), self.n_rows, ctypes.c_void_p(self.buf.data_ptr() + self.chunks_at), self.n_chunks,
                ptr(self.workspace))


def optim_record(device):
    """A zeroed struct rpe_optim_record as a (4,) float64 tensor: [0] is the norm; optim_record_fields names the rest."""
    return torch.zeros(4, dtype=torch.float64, device=device)


def optim_record_fields(record):
    """Views of a record: norm (1,) f64, norm_f32 (1,) f32, nonfinite (1,) int64."""
    return dict(norm=record[0:1], norm_f32=record.view(torch.float32)[2:3], nonfinite=record.view(torch.int64)[2:3])


def grad_norm(table, record):
    """rpe_grad_norm over an OptimTable: ``record`` (optim_record) <- the global L2 norm of the gradients (f64, f32) and the count of
    non-finite elements.  One launch, none for an empty table; no host synchronisation."""
    if table.n_rows == 0:
        return record
    if not (record.is_cuda and record.dtype == torch.float64 and record.numel() == 4 and record.is_contiguous()):
        raise _lib.RpeError('grad_norm: record must be ops.optim_record(device)')
    check(lib().rpe_grad_norm(*table._args(), ptr(record), stream_ptr()), 'rpe_grad_norm')
    return record


def adamw_step(table, record, state, lr, beta1, beta2, eps, weight_decay, max_norm=None, skip_nonfinite=True):
    """rpe_adamw_step over an OptimTable, behind grad_norm on the same stream: the clipped AdamW update of every row, or -- with a non-finite
    gradient and ``skip_nonfinite`` -- no write but ``state[1] += 1``.  ``state``: (2,) int64 on the device, [step counter, skipped steps].
    ``max_norm`` None or <= 0: no clipping.  One launch, none for an empty table; no host synchronisation."""
    if table.n_rows == 0:
        return
    if not (state.is_cuda and state.dtype == torch.int64 and state.numel() == 2 and state.is_contiguous()):
        raise _lib.RpeError('adamw_step: state must be a (2,) int64 GPU tensor')
    check(lib().rpe_adamw_step(*table._args(), ptr(record), ptr(state), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                               float(max_norm) if max_norm is not None else 0.0, int(bool(skip_nonfinite)), stream_ptr()), 'rpe_adamw_step')


# ------------------------------------------------------------------------------------------------- RAFT's sequence loss
FLOW_LOSS_FIELDS = dict(loss=0, epe=1, px1=2, px3=3, px5=4, count=5)       # RPE_FLOW_LOSS_* of include/rpe.h; the N terms follow at 6


def _flow_loss_check(flow_preds, flow_gt, valid, gamma, max_flow):
    """Every refusal of flow_sequence_loss, before any launch (shapes and types first, so they are raised without a GPU too) -> (the
    predictions, gt contiguous, valid as a contiguous uint8 (b,H,W))."""
    who = 'flow_sequence_loss'
    if not isinstance(flow_preds, (list, tuple)) or len(flow_preds) == 0:
        raise _lib.RpeError(f'{who}: flow_preds must be a non-empty list of (b,2,H,W) predictions')
    preds = list(flow_preds)
    if not isinstance(flow_gt, torch.Tensor) or flow_gt.dim() != 4 or flow_gt.shape[1] != 2 or flow_gt.dtype != torch.float32:
        raise _lib.RpeError(f'{who}: flow_gt must be a float32 (b,2,H,W) tensor')
    b, _, hh, ww = flow_gt.shape
    for k, p in enumerate(preds):
        if not isinstance(p, torch.Tensor) or p.dtype != torch.float32:
            raise _lib.RpeError(f'{who}: prediction {k} must be a float32 tensor')
        if tuple(p.shape) != (b, 2, hh, ww):
            raise _lib.RpeError(f'{who}: prediction {k} has shape {tuple(p.shape)}, flow_gt {tuple(flow_gt.shape)}')
        if not p.is_contiguous():
            raise _lib.RpeError(f'{who}: prediction {k} must be contiguous (the kernel reads it where it lies)')
    if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) not in ((b, hh, ww), (b, 1, hh, ww)):
        raise _lib.RpeError(f'{who}: valid must be a bool or uint8 ({b},{hh},{ww}) or ({b},1,{hh},{ww}) tensor')
    if not (0.0 < float(gamma) and float(max_flow) > 0.0):
        raise _lib.RpeError(f'{who}: gamma and max_flow must be positive, got {gamma} and {max_flow}')
    for name, t in [(f'prediction {k}', p) for k, p in enumerate(preds)] + [('flow_gt', flow_gt), ('valid', valid)]:
        if not t.is_cuda:
            raise _lib.RpeError(f'{who}: {name}: expected a tensor on the GPU (the HIP path has no CPU fallback)')
        _on_current_device(t, f'{who}: {name}')
    v = valid.reshape(b, hh, ww).contiguous()
    return preds, flow_gt.contiguous(), v.view(torch.uint8) if v.dtype == torch.bool else v


def _device_table(pointers, device):
    """Device pointers as a device int64 tensor, uploaded from pinned memory on the current stream without a host synchronisation
    (OptimTable's way)."""
    return torch.tensor(pointers, dtype=torch.int64).pin_memory().to(device, non_blocking=True)


class _FlowSequenceLossFn(torch.autograd.Function):
    """(gt, valid, weights table, max_flow, the N predictions) -> (loss 0-d f32, the record); the record is not differentiable."""

    @staticmethod
    def forward(ctx, gt, valid, weights, max_flow, *preds):
        n, (b, _, hh, ww), dev = len(preds), gt.shape, gt.device
        table = _device_table([p.data_ptr() for p in preds], dev)
        ws = torch.empty(int(lib().rpe_flow_sequence_loss_workspace_bytes(n, b, hh, ww)) // 8, dtype=torch.float64, device=dev)
        record = torch.empty(FLOW_LOSS_FIELDS['count'] + 1 + n, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        check(lib().rpe_flow_sequence_loss(ptr(table), n, ptr(gt), ptr(valid), ptr(weights), b, hh, ww, float(max_flow), ptr(ws), ptr(record),
                                           ptr(loss), stream_ptr()), 'rpe_flow_sequence_loss')
        ctx.save_for_backward(gt, valid, weights, table, *preds)
        ctx.max_flow = float(max_flow)
        ctx.mark_non_differentiable(record)
        return loss, record

    @staticmethod
    def backward(ctx, g, _g_record):
        gt, valid, weights, table, *preds = ctx.saved_tensors
        n, (b, _, hh, ww) = len(preds), gt.shape
        g = _f32(g.contiguous(), 'flow_sequence_loss: the gradient of the loss', numel=1)
        grads = [torch.empty_like(p) for p in preds]
        out = _device_table([t.data_ptr() for t in grads], gt.device)
        check(lib().rpe_flow_sequence_loss_backward(ptr(table), n, ptr(gt), ptr(valid), ptr(weights), ptr(g), b, hh, ww, ctx.max_flow, ptr(out),
                                                    stream_ptr()), 'rpe_flow_sequence_loss_backward')
        return (None, None, None, None, *grads)


def flow_sequence_loss(flow_preds, flow_gt, valid, gamma=0.8, max_flow=400.0):
    """RAFT's sequence loss on ground-truth flow (csrc/flow_loss.hip), from its published definition:
        mask = valid & (|flow_gt| < max_flow), |.| the per-pixel Euclidean norm;   w_k = gamma^(N-1-k), k = 0 .. N-1;
        loss = sum_k w_k (1/M) sum_{b,c,y,x} mask |pred_k - flow_gt|,   M = b 2 H W: the mean runs over all elements, not the valid ones.
    flow_preds: the N predictions, each a contiguous f32 (b,2,H,W) GPU tensor (RAFT.forward(all_flows=True, grad_all_flows=True) returns
    such a list); flow_gt f32 (b,2,H,W); valid bool or uint8 (b,H,W) or (b,1,H,W).
    -> (loss, metrics): ``loss`` a 0-d f32 tensor, the output of one autograd node over the N predictions, whose backward writes
    d pred_k = float32(w_k g / M) sign(pred_k - flow_gt) on mask pixels and exact 0 on masked pixels and where pred_k == flow_gt, in one
    launch from a g read on the device; ``metrics`` a dict of device tensors without gradient: 'epe', '1px', '3px', '5px' (the last
    prediction's mean end-point error over mask pixels and the fractions below 1, 3, 5 px; NaN when the mask is empty), 'count' (mask
    pixels, int64), 'loss_f64', 'terms' ((N,) f64, the unweighted per-iteration means).  Differences and sums in f64, partials per
    workgroup added in a fixed order: bit-identical from run to run.  Two launches forward, one backward, no host synchronisation.
    One deliberate departure from upstream RAFT: a masked pixel contributes EXACTLY ZERO to the loss and to the gradient, whatever the
    prediction or flow_gt hold there, NaN and inf included (upstream's ``valid * i_loss`` gives NaN).  A NaN in flow_gt under a valid pixel
    is not masked: it makes the loss and that pixel's gradient NaN, which optim.ClippedAdamW answers by skipping the step.
    Refused before any launch: an empty list, predictions that are not f32, not contiguous or not of flow_gt's shape, a ``valid`` of
    another shape or type."""
    preds, gt, v = _flow_loss_check(flow_preds, flow_gt, valid, gamma, max_flow)
    n = len(preds)
    weights = torch.tensor([float(gamma) ** (n - 1 - k) for k in range(n)], dtype=torch.float64).pin_memory().to(gt.device, non_blocking=True)
    loss, record = _FlowSequenceLossFn.apply(gt, v, weights, float(max_flow), *preds)
    F = FLOW_LOSS_FIELDS
    metrics = {'epe': record[F['epe']], '1px': record[F['px1']], '3px': record[F['px3']], '5px': record[F['px5']],
               'count': record.view(torch.int64)[F['count']], 'loss_f64': record[F['loss']], 'terms': record[F['count'] + 1:]}
    return loss, metrics
