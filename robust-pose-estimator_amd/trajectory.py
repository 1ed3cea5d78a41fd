"""Trajectory bookkeeping around the tracker: the per-frame loop of
scripts/infer_trajectory.py:71-97, Freiburg I/O of core/utils/trajectory.py:17-23,38-61 and the ATE / RPE
evaluation of core/metrics/trajectory_metrics.py:7-105 + evaluation/evaluate_ate_freiburg.py:6-31 (incl. its
time-stamp ``offset``; infer_trajectory.py:106 uses -4).  Host-side numpy: this is bookkeeping over a few
hundred 7-vectors, not part of the GPU hot path."""
import os

import numpy as np
import torch


def pose_matrices(vec7):
    """(m,7) [t, q(xyzw)] -> (m,4,4) homogeneous matrices (numpy, float64)."""
    v = np.asarray(vec7, dtype=np.float64).reshape(-1, 7)
    x, y, z, w = v[:, 3], v[:, 4], v[:, 5], v[:, 6]
    M = np.zeros((v.shape[0], 4, 4))
    M[:, 0, 0] = 1 - 2 * (y * y + z * z); M[:, 0, 1] = 2 * (x * y - z * w); M[:, 0, 2] = 2 * (x * z + y * w)
    M[:, 1, 0] = 2 * (x * y + z * w); M[:, 1, 1] = 1 - 2 * (x * x + z * z); M[:, 1, 2] = 2 * (y * z - x * w)
    M[:, 2, 0] = 2 * (x * z - y * w); M[:, 2, 1] = 2 * (y * z + x * w); M[:, 2, 2] = 1 - 2 * (x * x + y * y)
    M[:, :3, 3] = v[:, :3]
    M[:, 3, 3] = 1.0
    return M


class _QualityLog:
    """The ``quality=True`` side of the tracking loops: keeps each call's ``estimator.last_quality`` (device tensors, nothing waits) and
    attaches one row per trajectory item in ONE copy to the host at the end of the run.  The initial pose, which no frame produced,
    gets the report of a frame without a solve (NaN covariance, pd = 0), like a sequence's first frame."""

    def __init__(self, estimator, quality):
        self.on = bool(quality)
        if self.on and not getattr(estimator, 'report_quality', False):
            raise ValueError("quality=True needs an estimator built with report_quality: True in its config")
        self.estimator, self.parts, self.owners = estimator, [], []

    def start(self, items):
        """``items``: the trajectory items of the initial poses."""
        if self.on:
            from .pose_estimator import blank_quality
            self.add(items, blank_quality(len(items), self.estimator.device))

    def add(self, items, q=None):
        """``items``: the trajectory items the estimator's last call produced, in the row order of its ``last_quality``."""
        if self.on:
            self.parts.append(self.estimator.last_quality if q is None else q)
            self.owners.extend(items)

    def finish(self):
        if not self.on or not self.parts:
            return
        import torch
        host = {k: torch.cat([p[k] for p in self.parts]).cpu() for k in self.parts[0]}
        for j, item in enumerate(self.owners):
            item['quality'] = {k: v[j] for k, v in host.items()}


def track_sequence(estimator, frames, start_stamp=0, chunk=1, quality=False):
    """The loop of infer_trajectory.py:70-91.  ``frames`` yields (limg, rimg, mask, stamp) already on the device.
    Returns [{'camera-pose': (7,) tensor (mm), 'timestamp': stamp}], starting with the initial pose.
    ``chunk`` > 1: frames are handed to ``estimator.forward_chunk`` in groups of ``chunk`` (one RAFT pass per group; the same
    trajectory bit for bit, about twice the frames per second at 16); the sequence's first frame always goes through ``forward``.
    An estimator with ``warm_start`` needs ``chunk`` = 1 (a chunk's temporal flows come from one pass).
    ``quality`` (an estimator with ``report_quality: True``): every item gains 'quality', the frame's row of ``estimator.last_quality``
    as host tensors (cov (6,6) of the relative pose's left tangent in mm / rad, pd, n2d, n3d, rms2d_px, rms3d in mm, f, grad_max, n_iter,
    func_evals, stop_reason), copied to the host once, after the last frame; ``save_quality`` writes them."""
    import torch
    if chunk > 1 and getattr(estimator, 'warm_start', False):
        raise ValueError('track_sequence: warm_start starts frame t from frame t-1\'s flow, which a chunked pass cannot: use chunk=1')
    qlog = _QualityLog(estimator, quality)
    traj = [{'camera-pose': estimator.last_pose.vec().reshape(7).detach().cpu(), 'timestamp': start_stamp}]
    qlog.start(traj)
    pending = []

    def flush():
        if not pending:
            return
        if len(pending) == 1:
            limg, rimg, mask, stamp = pending[0]
            poses = estimator(limg, rimg, mask)[0].vec().reshape(1, 7)
        else:
            poses = estimator.forward_chunk(torch.cat([p[0] for p in pending]), torch.cat([p[1] for p in pending]),
                                            torch.cat([p[2] for p in pending]))[0]
        for row, (_, _, _, stamp) in zip(poses.detach().cpu(), pending):
            traj.append({'camera-pose': row.reshape(7), 'timestamp': stamp})
        qlog.add(traj[-len(pending):])
        pending.clear()
    for item in frames:
        pending.append(item)
        if chunk <= 1 or estimator.frame is None or len(pending) >= chunk:
            flush()
    flush()
    qlog.finish()
    return traj


def track_host_frames(estimator, source, ingest, start_stamp=0, pipelined=True, quality=False):
    """``track_sequence`` from frames on the host.  ``source`` yields (frame, stamp) or (frame, user_mask, stamp) with ``frame`` a decoded
    uint8 host frame, ``ingest`` is a preprocess.HostFrameIngest: its stream copies and prepares frame t+1 (and t+2, with depth 2) while
    the tracker works on frame t.  ``pipelined``: the frames go through ``estimator.submit`` / ``result``, so frame t+1's encoders too
    run beside frame t's update loop; an estimator that refuses ``submit`` (the surfel trackers: frame t+1 is tracked against the map
    frame t fused) is driven through ``forward`` as with pipelined=False -- copy and ingest still overlap.  Same kernels on the same
    inputs: the trajectory is that of ``track_sequence`` on the prepared frames, bit for bit.  ``quality``: as ``track_sequence``."""
    qlog = _QualityLog(estimator, quality)
    traj = [{'camera-pose': estimator.last_pose.vec().reshape(7).detach().cpu(), 'timestamp': start_stamp}]
    qlog.start(traj)
    waiting = []                                                   # stamps of the submitted frames

    def collect(pose, stamp):
        traj.append({'camera-pose': pose.vec().reshape(7).detach().cpu(), 'timestamp': stamp})
        qlog.add(traj[-1:])
    for limg, rimg, mask, stamp in ingest.stream(source):
        if pipelined:
            try:
                estimator.submit(limg, rimg, mask)
            except RuntimeError:                                   # refused before anything was queued
                pipelined = False
        if not pipelined:
            collect(estimator(limg, rimg, mask)[0], stamp)
            continue
        waiting.append(stamp)
        if len(waiting) > 1:                                       # frame t+1 is queued: now frame t
            collect(estimator.result()[0], waiting.pop(0))
    while waiting:
        collect(estimator.result()[0], waiting.pop(0))
    qlog.finish()
    return traj


def track_sequences(estimator, sequences, start_stamps=None, quality=False):
    """``track_sequence`` for K sequences at once on a MultiSurfelPoseEstimator (frame to model) or a MultiPoseEstimator (frame to frame):
    ``sequences[k]`` yields (limg, rimg, mask, stamp) of sequence k (row k of the estimator).  Every lockstep step takes the next frame of
    each sequence that has one and advances those rows in one ``estimator.forward`` call; a sequence that ends leaves the batch.  With the
    estimator's init_poses the K runs can be the (start, end) scenarios of one recording (scripts/benchmark_test.py).  Returns the K
    trajectories in track_sequence's format, each bit for bit the one a SurfelPoseEstimator / PoseEstimator run of that sequence alone
    gives.  ``quality``: as ``track_sequence``."""
    import torch
    qlog = _QualityLog(estimator, quality)
    n = len(sequences)
    if n > estimator.n_seq:
        raise ValueError(f'track_sequences: {n} sequences for an estimator of {estimator.n_seq}')
    stamps = [0] * n if start_stamps is None else list(start_stamps)
    if len(stamps) != n:
        raise ValueError(f'track_sequences: {n} sequences, {len(stamps)} start stamps')
    trajs = [[{'camera-pose': estimator.last_pose[k].vec().reshape(7).detach().cpu(), 'timestamp': stamps[k]}] for k in range(n)]
    qlog.start([t[0] for t in trajs])
    its = [iter(s) for s in sequences]
    live = list(range(n))
    while live:
        items = []
        for k in live:
            item = next(its[k], None)
            if item is not None:
                items.append((k, item))
        live = [k for k, _ in items]
        if not live:
            break
        poses = estimator(torch.cat([it[0] for _, it in items]), torch.cat([it[1] for _, it in items]),
                          torch.cat([it[2] for _, it in items]), rows=live)[0].vec().reshape(-1, 7)
        for row, (k, it) in zip(poses.detach().cpu(), items):
            trajs[k].append({'camera-pose': row.reshape(7), 'timestamp': it[3]})
        qlog.add([trajs[k][-1] for k, _ in items])
    qlog.finish()
    return trajs


def save_trajectory(trajectory, path):
    """trajectory.py:17-23 -- ``stamp tx ty tz qx qy qz qw`` per line, translation mm -> m."""
    fn = os.path.join(path, 'trajectory.freiburg')
    with open(fn, 'w') as f:
        for tr in trajectory:
            v = np.asarray(tr['camera-pose'], dtype=np.float64).reshape(7)
            f.write(f"{tr['timestamp']} {v[0] / 1000.0} {v[1] / 1000.0} {v[2] / 1000.0} {v[3]} {v[4]} {v[5]} {v[6]}\n")
    return fn


_TRIU = [(i, j) for i in range(6) for j in range(i, 6)]
QUALITY_COLUMNS = ('stamp', 'pd', 'stop_reason', 'n_iter', 'n2d', 'n3d', 'rms2d_px', 'rms3d_mm') + tuple(f'cov{i}{j}' for i, j in _TRIU)


def save_quality(trajectory, path):
    """``trajectory.quality.txt`` beside ``trajectory.freiburg``: per item that carries 'quality' (track_sequence(..., quality=True)) one line
    ``stamp pd stop_reason n_iter n2d n3d rms2d_px rms3d_mm`` + the 21 upper-triangle entries of ``cov`` (row-major; left tangent
    (tau, phi) of the frame's relative pose, mm and rad).  Floats are written with repr, so ``read_quality`` returns them bit for bit."""
    fn = os.path.join(path, 'trajectory.quality.txt')
    with open(fn, 'w') as f:
        f.write('# ' + ' '.join(QUALITY_COLUMNS) + '\n')
        for tr in trajectory:
            q = tr.get('quality')
            if q is None:
                continue
            cov = np.asarray(q['cov'], dtype=np.float64).reshape(6, 6)
            ints = [int(q[k]) for k in ('pd', 'stop_reason', 'n_iter', 'n2d', 'n3d')]
            floats = [float(q['rms2d_px']), float(q['rms3d'])] + [float(cov[i, j]) for i, j in _TRIU]
            f.write(' '.join([str(tr['timestamp'])] + [str(v) for v in ints] + [repr(v) for v in floats]) + '\n')
    return fn


def read_quality(path):
    """Reads ``save_quality``'s file -> dict: 'timestamp' (list; int where the text is one, else float), pd, stop_reason, n_iter, n2d, n3d
    (int64 (m,)), rms2d_px, rms3d_mm (float64 (m,)) and cov (m,6,6) float64, symmetric."""
    with open(path) as f:
        rows = [ln.split() for ln in f.read().split('\n') if ln.strip() and not ln.startswith('#')]
    for r in rows:
        if len(r) != len(QUALITY_COLUMNS):
            raise ValueError(f'{path}: a line has {len(r)} fields, expected {len(QUALITY_COLUMNS)}')

    def stamp(t):
        try:
            return int(t)
        except ValueError:
            return float(t)
    m = len(rows)
    out = {'timestamp': [stamp(r[0]) for r in rows]}
    for c, k in enumerate(('pd', 'stop_reason', 'n_iter', 'n2d', 'n3d')):
        out[k] = np.asarray([int(r[1 + c]) for r in rows], dtype=np.int64).reshape(m)
    out['rms2d_px'] = np.asarray([float(r[6]) for r in rows], dtype=np.float64).reshape(m)
    out['rms3d_mm'] = np.asarray([float(r[7]) for r in rows], dtype=np.float64).reshape(m)
    cov = np.zeros((m, 6, 6))
    for c, (i, j) in enumerate(_TRIU):
        col = np.asarray([float(r[8 + c]) for r in rows], dtype=np.float64).reshape(m)
        cov[:, i, j] = col
        cov[:, j, i] = col
    out['cov'] = cov
    return out


def read_freiburg(path, ret_stamps=False, no_stamp=False):
    """trajectory.py:38-61 -- poses (m,7) with translation converted m -> mm (and integer time stamps)."""
    with open(path) as f:
        lines = f.read().replace(',', ' ').replace('\t', ' ').split('\n')
    rows = [[v.strip() for v in ln.split(' ') if v.strip() != ''] for ln in lines if len(ln) > 0 and ln[0] != '#']
    rows = [r for r in rows if len(r) > 0]
    if no_stamp:
        arr = np.asarray([r[0:7] for r in rows], dtype=float)
        arr[:, :3] *= 1000.0
        return arr
    stamps = [r[0] for r in rows]
    try:
        stamps = np.asarray([int(s.split('.')[0] + s.split('.')[1]) for s in stamps]) * 100
    except IndexError:
        stamps = np.asarray([int(s) for s in stamps])
    arr = np.asarray([r[1:8] for r in rows], dtype=float)
    arr[:, :3] *= 1000.0
    return (arr, stamps) if ret_stamps else arr


def _align(model, data):
    """Horn closed-form alignment (trajectory_metrics.py:7-35); model, data are 3xn."""
    mz = model - model.mean(1, keepdims=True)
    dz = data - data.mean(1, keepdims=True)
    Wm = np.zeros((3, 3))
    for c in range(model.shape[1]):
        Wm += np.outer(mz[:, c], dz[:, c])
    U, _, Vh = np.linalg.svd(Wm.T)
    S = np.identity(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    rot = U @ S @ Vh
    T = np.eye(4)
    T[:3, :3] = rot
    T[:3, 3] = (data.mean(1, keepdims=True) - rot @ model.mean(1, keepdims=True))[:, 0]
    return T


def absolute_trajectory_error(gt_poses, predicted_poses, prealign=True, ignore_failed_pos=False):
    """ATE-RMSE (trajectory_metrics.py:38-73) on (m,4,4) arrays; returns (rmse, per-pose translation error)."""
    gt, pred = np.asarray(gt_poses, dtype=np.float64), np.asarray(predicted_poses, dtype=np.float64)
    assert len(gt) == len(pred)
    valid = np.ones(len(pred), dtype=bool)
    if ignore_failed_pos:                     # identical consecutive predictions mark failed estimations
        for i in range(len(pred) - 1):
            valid[i + 1] = (pred[i] - pred[i + 1]).sum() != 0
    if prealign:
        pred = _align(pred[valid, :3, 3].T, gt[valid, :3, 3].T)[None] @ pred
    terr = np.sum((gt[valid, :3, 3] - pred[valid, :3, 3]) ** 2, axis=1)
    return float(np.sqrt(np.mean(terr))), np.sqrt(terr)


def relative_pose_error(gt_poses, predicted_poses, delta=1, ignore_failed_pos=False):
    """RPE (trajectory_metrics.py:76-105): per-pair translation norm and rotation angle of gt_rel^-1 pred_rel."""
    gt, pred = np.asarray(gt_poses, dtype=np.float64), np.asarray(predicted_poses, dtype=np.float64)
    te, re = [], []
    for i in range(len(gt) - delta):
        if ((pred[i] - pred[i + 1]).sum() != 0) or (not ignore_failed_pos):
            e = np.linalg.inv(np.linalg.inv(gt[i]) @ gt[i + delta]) @ (np.linalg.inv(pred[i]) @ pred[i + delta])
            te.append(np.sqrt(np.sum(e[:3, 3] ** 2)))
            re.append(np.arccos(max(min(0.5 * (np.trace(e[:3, :3]) - 1), 1.0), -1.0)))
    return np.asarray(te), np.asarray(re)


def evaluate(gt, pred, delta=1, offset=0, ignore_failed_pos=False):
    """evaluate_ate_freiburg.py:6-31.  gt / pred: freiburg file paths or {stamp: (7,) pose} dicts.
    A prediction with stamp k is compared with the ground truth at k + offset (kept if 0 < k+offset < max stamp)."""
    def load(x):
        if isinstance(x, dict):
            return x
        poses, stamps = read_freiburg(x, ret_stamps=True)
        return {int(k): p for k, p in zip(stamps, poses)}
    gt_d, pr_d = load(gt), load(pred)
    gmax = max(gt_d.keys())
    P, G = [], []
    for k in sorted(pr_d.keys()):
        if (k + offset > 0) and (k + offset < gmax):
            P.append(pr_d[k])
            G.append(gt_d[k + offset])
    Pm, Gm = pose_matrices(np.stack(P)), pose_matrices(np.stack(G))
    ate, terr = absolute_trajectory_error(Gm, Pm, ignore_failed_pos=ignore_failed_pos)
    rt, rr = relative_pose_error(Gm, Pm, delta=delta, ignore_failed_pos=ignore_failed_pos)
    return ate, float(np.mean(rt)), float(np.mean(rr)), terr, rt, rr
