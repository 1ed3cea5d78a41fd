"""Float64 restatements (torch on the CPU, no kernels) of the small RAFT operations of csrc/raft_ops.hip, one function per operation,
each saying what the kernel's header comment says.  Every input is converted to float64 first; every output is float64.
tests/test_raft_ops_ref_cpu.py pins them against torch's own operators; tests/test_gpu_raft_ops_edges.py holds the kernels to them.

Non-finite values follow IEEE arithmetic on the sums as written below, with two rules stated where they matter:
  * ReLU is ``y < 0 ? 0 : y``: NaN stays NaN (torch.relu does the same);
  * a tap of the 3x3 flow head or of the up-sampling's unfold that lies outside the map is ABSENT from the sum (conv3x3_to2) or an exact
    zero operand (upsample_convex, as F.unfold's zero padding is) -- never the product of a weight with a clamped in-map value."""
import torch
import torch.nn.functional as F


def f64(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double()


def relu(y):
    """max(y, 0) that keeps NaN."""
    return torch.where(y < 0, torch.zeros_like(y), y)


def _chan(v):
    return v[None, :, None, None]


# ------------------------------------------------------------------------------------------------------------------ gates
def gates_zr(zr, bias, add, h, c):
    """zr (b,2c,h,w) pre-activations, bias (2c) or None, add like zr or None, h (b,>=c,h,w): returns (z, r * h[:, :c]) with
    z = sigmoid(zr[:, :c] + add[:, :c] + bias[:c]) and r = sigmoid(zr[:, c:] + add[:, c:] + bias[c:])."""
    pre = f64(zr)
    if add is not None:
        pre = pre + f64(add)
    if bias is not None:
        pre = pre + _chan(f64(bias))
    z = 1.0 / (1.0 + torch.exp(-pre[:, :c]))
    r = 1.0 / (1.0 + torch.exp(-pre[:, c:2 * c]))
    return z, r * f64(h)[:, :c]


def gates_h(z, q, bias, add, h):
    """(1 - z) * h[:, :c] + z * tanh(q + add + bias), c = z's channel count."""
    z, pre = f64(z), f64(q)
    if add is not None:
        pre = pre + f64(add)
    if bias is not None:
        pre = pre + _chan(f64(bias))
    return (1.0 - z) * f64(h)[:, :z.shape[1]] + z * torch.tanh(pre)


# ------------------------------------------------------------------------------------------- bias / norm / affine epilogues
def bias_act(x, bias, relu_=True):
    y = f64(x)
    if bias is not None:
        y = y + _chan(f64(bias))
    return relu(y) if relu_ else y


def _residual(y, relu_, residual):
    if relu_:
        y = relu(y)
    if residual is not None:
        y = relu(f64(residual) + y)
    return y


def instnorm_act(x, bias, eps=1e-5, relu_=True, residual=None):
    """Per (b, c) plane of x + bias: (v - mean) / sqrt(biased variance + eps); then the optional ReLU; with a residual,
    max(residual + y, 0) after it."""
    v = f64(x)
    if bias is not None:
        v = v + _chan(f64(bias))
    mean = v.mean(dim=(2, 3), keepdim=True)
    var = ((v - mean) ** 2).mean(dim=(2, 3), keepdim=True)
    return _residual((v - mean) / torch.sqrt(var + float(eps)), relu_, residual)


def affine_act(x, scale, shift, relu_=True, residual=None):
    """x * scale[c] + shift[c]; then as instnorm_act."""
    return _residual(f64(x) * _chan(f64(scale)) + _chan(f64(shift)), relu_, residual)


# -------------------------------------------------------------------------------------------------------------- flow head
def conv3x3_to2(x, w, bias=None, add=None):
    """out[b, o, y, x] = bias[o] + add[b, o, y, x] + sum over c and the taps (dy, dx) of the 3x3 window THAT LIE INSIDE THE MAP of
    x[b, c, y + dy - 1, x + dx - 1] * w[o, c, dy, dx].  A tap outside the map is not in the sum (it is not a product with zero), so an
    Inf or NaN reaches exactly the outputs whose window holds it -- what F.conv2d(padding=1) gives."""
    x, w = f64(x), f64(w)
    b, c, hh, ww = x.shape
    out = torch.zeros(b, 2, hh, ww, dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            # outputs y in [y0, y1) read input rows y + dy - 1 in [0, hh)
            y0, y1 = max(0, 1 - dy), min(hh, hh + 1 - dy)
            x0, x1 = max(0, 1 - dx), min(ww, ww + 1 - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            src = x[:, :, y0 + dy - 1:y1 + dy - 1, x0 + dx - 1:x1 + dx - 1]
            out[:, :, y0:y1, x0:x1] += torch.einsum('bchw,oc->bohw', src, w[:, :, dy, dx])
    if bias is not None:
        out = out + _chan(f64(bias))
    if add is not None:
        out = out + f64(add)
    return out


def coords_grid(b, hh, ww):
    """coords0 of RAFT: channel 0 = x, channel 1 = y."""
    ys, xs = torch.meshgrid(torch.arange(hh, dtype=torch.float64), torch.arange(ww, dtype=torch.float64), indexing='ij')
    return torch.stack([xs, ys])[None].repeat(b, 1, 1, 1)


def flow_update(x, w, bias, coords):
    """rpe_conv3x3_to2_flow: (coords_out, flow) with coords_out = conv3x3_to2(x, w, bias, add=coords), flow = coords_out - pixel grid."""
    out = conv3x3_to2(x, w, bias, coords)
    return out, out - coords_grid(*out.shape[:1], *out.shape[2:])


# ------------------------------------------------------------------------------------------------------------ up-sampling
def upsample_convex(flow, mask):
    """flow (b,2,h8,w8), mask (b,576,h8,w8), channel = k*64 + i*8 + j: out[b, :, 8y+i, 8x+j] = sum_k softmax_k(mask[b, k, i, j, y, x])
    * 8 * flow[b, :, y + k//3 - 1, x + k%3 - 1], the flow zero outside the map (F.unfold's padding: an exact zero operand)."""
    flow, mask = f64(flow), f64(mask)
    b, _, hh, ww = flow.shape
    m = mask.reshape(b, 9, 8, 8, hh, ww)
    e = torch.exp(m - m.max(dim=1, keepdim=True).values)
    p = e / e.sum(dim=1, keepdim=True)
    pad = F.pad(8.0 * flow, (1, 1, 1, 1))
    out = torch.zeros(b, 2, 8, 8, hh, ww, dtype=torch.float64)
    for k in range(9):
        nb = pad[:, :, k // 3:k // 3 + hh, k % 3:k % 3 + ww]                 # (b, 2, hh, ww)
        out += p[:, k][:, None] * nb[:, :, None, None]
    return out.permute(0, 1, 4, 2, 5, 3).reshape(b, 2, 8 * hh, 8 * ww)


# ------------------------------------------------------------------------------------------------------------- comparisons
def compare(got, want, atol, what=''):
    """Every element of ``got`` against the float64 ``want``: NaN at the same positions, +-Inf at the same positions with the same sign,
    all remaining elements within ``atol`` (a number, or a tensor with one bar per element).  Returns the largest error of the finite elements."""
    got, want = f64(got), f64(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f'{what}: NaN at {int(gn.sum())} positions, the reference at {int(wn.sum())}; first differing ' \
                                f'{(gn != wn).nonzero()[:4].tolist()}'
    gi, wi = torch.isinf(got), torch.isinf(want)
    assert torch.equal(gi, wi), f'{what}: Inf positions differ; first {(gi != wi).nonzero()[:4].tolist()}'
    assert torch.equal(torch.sign(got[gi]), torch.sign(want[wi])), f'{what}: Inf signs differ'
    fin = ~(gn | gi)
    if not bool(fin.any()):
        return 0.0
    diff = (got - want).abs()
    bar = torch.as_tensor(atol, dtype=torch.float64).expand_as(diff) if isinstance(atol, torch.Tensor) else torch.full_like(diff, float(atol))
    over = fin & ~(diff <= bar)
    assert not bool(over.any()), f'{what}: {int(over.sum())} elements over the bar; worst {float(diff[over].max()):.3e}, first at ' \
                                 f'{over.nonzero()[:4].tolist()} (bar there {float(bar[over][0]):.3e})'
    return float(diff[fin].max())
