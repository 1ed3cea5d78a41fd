"""Host restatement of rpe_flow_forward_interpolate (include/rpe.h) in numpy: the contract the GPU kernel is held to bit for bit.

Upstream RAFT's forward_interpolate (core/RAFT/core/utils/utils.py) pushes a 1/8 flow forward along itself and fills the grid with
scipy griddata(method='nearest') over the landing points strictly inside the map.  Restated exactly: landing points and squared
distances in f64 (two rounded squares, then their rounded sum), the nearest valid point per grid point, ties to the LOWEST source
index (griddata leaves them undefined), zeros for a row without a valid point (griddata raises)."""
import numpy as np


def forward_interpolate_row(flow, chunk=1024):
    """flow (2,h,w) float32 -> (2,h,w) float32."""
    dx, dy = flow[0].astype(np.float32).ravel(), flow[1].astype(np.float32).ravel()
    h, w = flow.shape[1:]
    y0, x0 = np.divmod(np.arange(h * w), w)
    x1 = x0.astype(np.float64) + dx.astype(np.float64)
    y1 = y0.astype(np.float64) + dy.astype(np.float64)
    valid = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    out = np.zeros((2, h * w), np.float32)
    idx = np.nonzero(valid)[0]                       # increasing source index: argmin's first minimum is the lowest index
    if idx.size == 0:
        return out.reshape(2, h, w)
    px, py = x1[idx], y1[idx]
    for lo in range(0, h * w, chunk):
        gy, gx = np.divmod(np.arange(lo, min(lo + chunk, h * w)), w)
        ex = gx.astype(np.float64)[:, None] - px[None, :]
        ey = gy.astype(np.float64)[:, None] - py[None, :]
        d = ex * ex + ey * ey
        pick = idx[np.argmin(d, axis=1)]
        out[0, lo:lo + len(gx)] = dx[pick]
        out[1, lo:lo + len(gx)] = dy[pick]
    return out.reshape(2, h, w)


def forward_interpolate(flow):
    """flow (N,2,h,w) -> (N,2,h,w), row by row."""
    return np.stack([forward_interpolate_row(f) for f in np.asarray(flow)])


def make_flows(kind, h, w, seed=0):
    """(1,2,h,w) float32 test flows: 'subpixel' random sub-pixel motion, 'outward' most points pushed out of the map, 'invalid' none
    left inside, 'zero', 'shift' integer shifts (landing exactly on grid points: ties everywhere)."""
    rng = np.random.default_rng(seed)
    if kind == 'subpixel':
        f = rng.uniform(-3.0, 3.0, (2, h, w))
    elif kind == 'outward':
        f = rng.uniform(-1.5, 1.5, (2, h, w)) * np.array([w, h]).reshape(2, 1, 1)
    elif kind == 'invalid':
        f = np.stack([np.full((h, w), float(w)), rng.uniform(-2, 2, (h, w))])
    elif kind == 'zero':
        f = np.zeros((2, h, w))
    elif kind == 'shift':
        f = np.stack([np.full((h, w), 3.0), np.full((h, w), -2.0)])
    else:
        raise ValueError(kind)
    return f.astype(np.float32)[None]
