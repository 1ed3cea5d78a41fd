"""The TinyUNet inference forward in plain torch (no GPU), the truth the fused weight heads (csrc/unet.hip: rpe_unet_heads) are held to
in tests/test_gpu_unet_edges.py; its own properties are checked without a GPU in tests/test_unet_ref_cpu.py.

``forward_ref`` restates core/unet/unet.py:7-82 + the nn.Sigmoid of core/pose/pose_net.py:109-115 with one change: the skip is cropped
to the up-convolution's size from offset floor(d / 2), ``sk[dh:dh + uh, dw:dw + uw]``.  The reference (and oracle/unet.py, and
TinyUNet.forward_infer) slice ``dh:H - dh``, which fits only when the difference is even, i.e. on 1/8 grids that are multiples of 4;
elsewhere they raise in torch.cat, while rpe_unet_heads -- what PoseNet.infer calls -- computes, with this crop.  Where the reference
runs, the two are the same function (asserted bit for bit in test_unet_ref_cpu.py).  The same restatement, for the training twin, is
``forward_ref`` of tests/test_gpu_unet_train.py.

Tolerance rule of the tests built on this file (``bar``): the weight maps p = sigmoid(logits) are compared with the float64 forward;
the yardstick is the float32 CPU forward of the same function against the same truth; the kernels must stay within 4x of it (FACTOR of
test_gpu_unet_train.py: a different summation order over up to 272 x 9 terms per output), and the yardstick is never taken below
2^-23, the spacing of float32 on [0.5, 1), so that the rounding of the final expf and division cannot decide a test."""
import copy
import functools

import torch
import torch.nn.functional as F

FACTOR = 4.0
# (h8, w8, b) -> seed.  44x44: the smallest grid; 45x47: pools 41x43 maps (the last row and column are pooled by nothing); 46x52 and
# 47x44: skip crops over odd differences with dh != dw (46x52: 17 -> 8 rows against 20 -> 12 columns in the first decoder stage, 42 -> 8
# against 48 -> 16 in the second); 64x80: the 640x512 grid of the benchmark.  Only 44x44 and 64x80 are multiples of 4.
PARITY_CASES = {(44, 44, 2): 1, (45, 47, 2): 2, (46, 52, 2): 3, (47, 44, 1): 4, (64, 80, 1): 5}
NAN_GRID, NAN_AT = (46, 52, 2), ((0, 100, 2, 2), (0, 100, 23, 26))     # hidden[...]: outside both skip crops / inside them


def forward_ref(net, x, out_size=None, crop='floor', pool=None):
    """TinyUNet inference forward (frozen norms) in the dtype of ``net`` and ``x`` -> (logits, sigmoid(logits)) at ``out_size``
    (default: the net's).  ``crop='ceil'`` and ``pool`` exist only so that test_unet_ref_cpu.py can show what the cases can tell apart."""
    pool = pool or (lambda t: F.max_pool2d(t, 2))
    def bn(st, t):
        n = st.norm
        return F.batch_norm(t, n.running_mean, n.running_var, n.weight, n.bias, False, n.momentum, n.eps)
    with torch.no_grad():
        skips = []
        for st in net.encoder.enc_blocks:
            x = F.conv2d(torch.relu(bn(st, F.conv2d(x, st.conv1.weight, st.conv1.bias))), st.conv2.weight, st.conv2.bias)
            skips.append(x)
            x = pool(x)
        x = skips.pop()
        for upc, st in zip(net.decoder.upconvs, net.decoder.dec_blocks):
            x = F.conv_transpose2d(x, upc.weight, upc.bias, stride=2)
            sk = skips.pop()
            uh, uw = x.shape[-2:]
            dh, dw = sk.shape[-2] - uh, sk.shape[-1] - uw
            dh, dw = ((dh + 1) // 2, (dw + 1) // 2) if crop == 'ceil' else (dh // 2, dw // 2)
            x = torch.cat((x, sk[..., dh:dh + uh, dw:dw + uw]), dim=1)
            x = F.conv2d(bn(st, torch.relu(F.conv2d(x, st.conv1.weight, st.conv1.bias))), st.conv2.weight, st.conv2.bias)
        logits = F.interpolate(F.conv2d(x, net.head.weight, net.head.bias), out_size or net.out_sz, mode='bilinear')
        return logits, torch.sigmoid(logits)


def make_heads(h, w, seed, gain=2.0):
    """The two heads (264 and 272 input channels) for an (h, w) output as rpe_amd.unet.TinyUNet and oracle.unet.TinyUNet with one state
    dict (float32, CPU, eval): batch-norm statistics randomised as in tests/test_gpu_unet.py::_heads, every Conv2d and ConvTranspose2d
    weight multiplied by ``gain`` -- with the default initialisation the logits span about 0.1 and the maps are near-constant at 0.5."""
    from oracle import unet as ounet
    from rpe_amd import unet
    torch.manual_seed(seed)
    nets, onets = [], []
    for cin in (264, 272):
        n = unet.TinyUNet(cin, (h, w)).eval()
        for m in n.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5); m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_(0, 0.2)
            elif isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                m.weight.data.mul_(gain)
        o = ounet.TinyUNet(cin, (h, w)).eval()
        o.load_state_dict(n.state_dict())
        nets.append(n); onets.append(o)
    return nets, onets


def make_inputs(b, h8, w8, seed):
    """inp1, inp2 (b, 8, h8, w8) and hidden | context as the two halves of one (b, 256, h8, w8) buffer."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, 8, h8, w8, generator=g), torch.randn(b, 8, h8, w8, generator=g), torch.randn(b, 256, h8, w8, generator=g)


def head_inputs(inp1, inp2, hc):
    """The concatenated inputs of the two heads (core/pose/pose_net.py:109-115)."""
    return torch.cat((inp1, hc), 1), torch.cat((inp1, inp2, hc), 1)


def bar(truth_p, f32_p):
    return FACTOR * max(float((f32_p.double() - truth_p).abs().max()), 2.0 ** -23)


def run_cpu(nets, xs, dtype, **kw):
    """[(logits, p)] of both heads in ``dtype``."""
    return [forward_ref(copy.deepcopy(n).to(dtype), x.to(dtype), **kw) for n, x in zip(nets, xs)]


@functools.lru_cache(maxsize=None)
def case(h8, w8, b, nan_at=None):
    """Heads, inputs, the float64 truth and the float32 yardstick of one grid -- computed once per process, shared, never written to.
    ``nan_at``: an index into hidden that is set to NaN."""
    seed = PARITY_CASES.get((h8, w8, b), 100 + h8 + w8 + b)
    nets, onets = make_heads(8 * h8, 8 * w8, seed)
    inp1, inp2, hc = make_inputs(b, h8, w8, seed + 1000)
    if nan_at is not None:
        hc[:, :128][nan_at] = float('nan')
    xs = head_inputs(inp1, inp2, hc)
    return dict(nets=nets, onets=onets, inp1=inp1, inp2=inp2, hc=hc, xs=xs, f64=run_cpu(nets, xs, torch.float64), f32=run_cpu(nets, xs, torch.float32))
