"""Reference arithmetic of the fp16-operand convolution route (rpe_conv_f16, RAFT's ``update_fp16``); importable without a GPU.

The contract (include/rpe.h): every input activation and every weight of a covered layer is rounded to IEEE fp16, round to nearest even,
unscaled; products and sum are f32; everything after the sum is rpe_conv_fused's f32 epilogue.  So
  * a kernel is compared with the FLOAT64 convolution of the ROUNDED operands (conv_ref): the two differ by f32 accumulation only, and
    the bar is the direct f32 kernel's own (test_gpu_conv._tol on the rounded operands);
  * a model is compared with the CPU oracle whose covered modules round their input and weight (f16_update_oracle): oracle/ stays as
    it is, the modules of a deep copy get a wrapped ``forward``."""
import copy

import torch
import torch.nn.functional as F

LINEAR, RELU, GATE_ZR, GATE_H, TANH = 0, 1, 2, 3, 4
HIDDEN = 128                                                    # SepConvGRU's hidden and context widths

# the covered layers of BasicUpdateBlock, by their module names inside oracle.raft.RAFT (and rpe_amd.raft.RAFT)
PLAIN = ('update_block.encoder.convc1', 'update_block.encoder.convc2', 'update_block.encoder.convf2', 'update_block.encoder.conv',
         'update_block.flow_head.conv1', 'update_block.mask.0', 'update_block.mask.2')
GATES = tuple(f'update_block.gru.conv{g}{half}' for half in (1, 2) for g in 'zrq')
COVERED = PLAIN + GATES


def round_h(t):
    """IEEE fp16, round to nearest even, back in f32 (|x| >= 65520 -> +-Inf, NaN stays NaN)."""
    return t.half().float()


def conv_ref(x, w, bias=None, add=None, mode=LINEAR, hidden=None, zgate=None, gate_channels=0, rounded=True):
    """rpe_conv_fused's operation in float64 on fp16-rounded operands (``rounded=False``: on the operands as they are) -> (out, out2);
    out2 is r * hidden for GATE_ZR (out = z), else a copy of out."""
    xr, wr = (round_h(x), round_h(w)) if rounded else (x, w)
    v = F.conv2d(xr.double(), wr.double(), None, padding=(w.shape[2] // 2, w.shape[3] // 2))
    if add is not None:
        v = v + add.double()
    if bias is not None:
        v = v + bias.double()[None, :, None, None]
    if mode == GATE_ZR:
        s, c = torch.sigmoid(v), gate_channels
        return s[:, :c], s[:, c:] * hidden.double()[:, :c]
    if mode == GATE_H:
        z, c = zgate.double(), v.shape[1]
        out = (1 - z[:, :c]) * hidden.double()[:, :c] + z[:, :c] * torch.tanh(v)
        return out, out
    out = v.clamp_min(0) if mode == RELU else torch.tanh(v) if mode == TANH else v
    return out, out


def _plain_forward(m):
    def forward(x):
        return F.conv2d(round_h(x), round_h(m.weight), m.bias, m.stride, m.padding)
    return forward


def _gate_forward(m, c=HIDDEN):
    """A SepConvGRU convolution on cat[h | inp | motion]: the loop-varying columns (h and the motion features, 256 of the 384) take
    rounded operands, the 128 context channels' term (with the bias) is the f32 convolution it always was; the two are summed."""
    def forward(x):
        var = torch.cat((x[:, :c], x[:, 2 * c:]), 1), torch.cat((m.weight[:, :c], m.weight[:, 2 * c:]), 1)
        return F.conv2d(round_h(var[0]), round_h(var[1]), None, m.stride, m.padding) + F.conv2d(x[:, c:2 * c], m.weight[:, c:2 * c], m.bias, m.stride, m.padding)
    return forward


def f16_update_oracle(model):
    """A deep copy of an oracle.raft.RAFT whose covered modules (COVERED) compute with fp16-rounded input and weight; bias and output stay
    f32.  The wrap REPLACES a module's ``forward`` (an instance attribute bound to the copy's own module), so wrapping a wrapped model
    changes nothing; ``wrapped_f16`` lists what is wrapped."""
    model = copy.deepcopy(model)
    mods = dict(model.named_modules())
    for name in COVERED:
        mods[name].forward = (_gate_forward if name in GATES else _plain_forward)(mods[name])
    model.wrapped_f16 = tuple(sorted(COVERED))
    return model
