"""RAFT host mirror: same constructor / forward contract as the reference's RAFT fork
(``RAFT(config)(img1, img2, upsample=True) -> (flow_predictions, hidden, context)``, call sites
core/pose/pose_net.py:21-22,47,65,129) and the upstream parameter names, so ``raft-things.pth`` /
``poseNet_*.pth`` state dicts load unchanged.

What runs where (MI355X-first split), all hand-written HIP through the C ABI:
  * all-pairs correlation + pyramid and the per-iteration window lookup (csrc/corr.hip)
  * every convolution of the update block with its bias / ReLU / concat / GRU-gate epilogue, the encoders' residual
    blocks (3x3 stride 1 and 2, 1x1 stride-2 shortcut) with folded batch norm / instance-norm statistics, as f32-MFMA
    implicit GEMMs (csrc/conv.hip); the 7x7 stems and convf1 (csrc/stem.hip)
  * the update block's and the encoders' 3x3 stride-1 layers as Winograd F(2x2,3x3) (csrc/conv_wino.hip), the GRU's 1x5 / 5x1
    layers with their gate epilogues as Winograd F(4,5) (csrc/conv_wino1d.hip); the encoders' final 1x1 (cnet's with its
    tanh | ReLU split in the epilogue) and the mask head's 1x1 on the implicit GEMM
  * flow-head output layer with the coords / flow bookkeeping of the loop, convex up-sampling, norm / bias passes, slice copies
    (csrc/raft_ops.hip)
  * opt-in (config ``pad_maps``): at such map sizes the UPDATE LOOP on the tuned kernels over zero-padded maps (padded_size; the kernels' valid-extent
    entry points rpe_conv_*_v keep the padding zero); the encoders stay on the generic route below unless
  * opt-in (config ``pad_encoders``): at such sizes layer2, layer3 and the output layer of both ENCODERS on the tuned kernels over maps zero-padded
    to 4x / 2x / 1x padded_size (the encoder forms rpe_enc_conv_wino_v / _wino24_v / _s2_v / _s2_m96_v, rpe_instnorm_apply_v, rpe_conv1x1_v: zero
    stored outside the content, instance-norm moments and the loader-side normalisation over the content only); the stem and layer1 keep the
    true 1/2 map, the result leaves cropped
  * map sizes the tuned kernels refuse (odd maps, rows that are not whole 16-byte quads: image widths that are not a multiple of 32,
    heights not a multiple of 16): the same layers on the generic implicit GEMM (csrc/conv_direct.hip) with the stand-alone epilogue
    kernels -- robust, slower; no launch of a pass goes to a library at any size
Exact re-associations used (results identical up to float rounding):
  * convz/convr of each GRU half share their input, so their weights are stacked into one 256-channel conv
  * the GRU input is (h | inp | motion | flow) and the context `inp` is the same in all 12 iterations, so the
    inp-channel part of every GRU convolution (+ bias) is computed once per pass and added inside the gate kernels:
    the per-iteration convolutions read 256 instead of 384 channels (a third of the GRU's FLOPs hoisted out of the loop)
  * the (h | x) concatenations live in two persistent buffers; the gate kernels write r*h and the new h in place
  * the mask head + convex up-sampling only run for the predictions that are returned (``all_flows=False``
    returns just the final one, which is all the reference's PoseNet reads: ``[0][-1]``)
The RAFT architecture itself is restated from princeton-vl/RAFT (the reference's submodule is empty);
see oracle/raft.py for the CPU restatement these kernels are tested against.
"""
import operator
from types import SimpleNamespace
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import ops, raft_grad
from ._lib import RpeError
from .ops import bounded_put, wkey

# Module-level route constants (no environment switches in the product: tools/ and bench.py's labelled experiments set these attributes)
WINOGRAD = True          # 3x3 layers as F(2x2,3x3), the GRU's 1x5 / 5x1 as F(4,5); False = the direct implicit GEMM (A/B measurements)
WINO_2X4 = True          # under WINOGRAD, 3x3 layers on maps with w % 4 == 0 as F(2x4,3x3) (rpe_conv_wino24: a quarter fewer products);
                         # False = F(2x2) everywhere (A/B measurements)
S2_M96 = True            # the stride-2 3x3 layers of 96 output channels on 96-row tiles (rpe_conv_fused_m96: no idle wave; bit-identical);
                         # False = rpe_conv_fused's 128-row tiles (A/B measurements)
S2_M96_MIN_WGS = 512     # ... for launches of at least this many 128-pixel workgroups: below, rpe_conv_fused's 64 x 64 tiles fill the chip better
CORR_BF16X3 = False      # EXPERIMENT: correlation products as six bf16 products of an exact 3-way split (bench.py --corr-bf16x3)
CONV_BF16X3 = False      # LABELLED VARIANT (bench.py --conv-bf16x3; never the headline): the update block's 3x3 layers with >= 128 input
#                          channels (convc2, conv, FlowHead.conv1, the mask head's 3x3) through rpe_conv_wino_x3 -- Winograd products as six
#                          bf16 products of an exact 3-way split --, the 1x1 layers with LINEAR / RELU epilogues (convc1, fnet's output layer,
#                          the ReLU half of cnet's, the mask head's 1x1) through rpe_conv1x1_x3, and the correlation build through
#                          k_corr_build_x3.  The layers it does NOT cover (measured no faster) stay on the f32 matrix cores: the encoders'
#                          3x3 layers, convf2, the GRU's 1x5 / 5x1 layers (unless X3_GRU), the tanh half of cnet's output layer, the stems.
X3_MIN_CIN = 128         # rpe_conv_wino_x3 pays from 8 K steps of 16 channels on
X3_GRU = False           # under CONV_BF16X3, also the SepConvGRU's 1x5 / 5x1 layers on rpe_conv_wino1d_x3.  Off: in the bench step its launches
#                          take 449 / 410 us (z|r, 1x5 / 5x1) and 251 / 237 us (q) against rpe_conv_wino1d's 407 / 395 and 240 / 224 -- one
#                          workgroup per CU has nothing to run beside its memory-bound gate pass (csrc/conv_wino1d_x3.hip); kept, tested, opt-in.
# RAFT's ``update_fp16`` for models built without the config key (tools/bench_update_fp16.py): the update block's convolutions with fp16
# OPERANDS on the 16-bit matrix cores (rpe_conv_f16: operands rounded to nearest even, f32 products, sum and epilogue) -- what upstream
# RAFT's mixed_precision (autocast) does to the update block.  Covered: convc1, convc2, convf2, conv, the GRU convolutions' loop-varying 256
# input channels with their gates, FlowHead.conv1, the mask head.  Not covered (f32): the GRU's context terms, convf1, FlowHead.conv2, the
# encoders, the correlation.  A precision contract, uniform over the covered layers; opt-in, never the headline.  Refused with CONV_BF16X3,
# without WINOGRAD, with pad_maps / pad_encoders and on 1/8 maps with w % 4 != 0 (resolve_route).
UPDATE_FP16 = False
# The motion encoder's flow branch (convf1 -> convf2) on a side stream beside lookup -> convc1 -> convc2.  Measured (MI355X, 640x512):
# batch 1-2 (sequential tracking) 9.22 -> 9.08 ms per frame pair, 110.2 -> 111.9 frames/s; batch 32: 72.49 vs 72.41 ms per step (every
# launch fills the chip on its own), so it is used for small passes only.
SIDE_STREAM = True
# RAFT's ``pad_maps`` for models built without the config key (tools/bench_pad_maps.py, A/B runs): at 1/8 maps the tuned kernels refuse, the
# update loop runs on maps zero-padded to the next size they take (padded_size).  Opt-in; no effect on maps they take as they are.
PAD_MAPS = False
# RAFT's ``pad_encoders`` for models built without the config key: at image sizes whose 1/8 map the tuned kernels refuse, both encoders run
# layer2, layer3 and the output layer on zero-padded maps instead of on the generic convolution.  Opt-in; no effect at any other size.
PAD_ENCODERS = False
# The update loop as ONE call into the library (ops.OpList -> rpe_run_ops): the 12 iterations' ~130-180 launches and stream fork / joins are
# enqueued by a C loop over prepared argument blocks instead of one Python-dispatched ctypes call each (bit-identical: the same entry
# points with the same arguments).  False = launch by launch from Python (bench.py's per-convolution diagnostic pass, A/B runs).
LOOP_OPLIST = True
# bench.py's hook for timing the lookup INSIDE the timed region: a callable iters -> 2 * iters raw hipEvent_t handles (ints), recorded in
# front of and behind each iteration's lookup by the launch list itself; None = the list's timing cells stay empty (no-ops)
LOOKUP_EVENT_SINK = None
# Sequential tracking encodes 1-3 images and runs one or two flow pairs per frame: ~75 launches around the update loop whose Python dispatch
# (argument checks, descriptor construction, output allocation) costs more host time than the loop's list.  For such small passes an
# encoder pass and the two ends of RAFT.forward are RECORDED once (ops.Recorder: an ordinary pass that also logs its launches and keeps its
# intermediates as a private workspace) and replayed as launch lists with the input / output pointers rewritten.  Bit-identical (the same
# entry points with the same arguments); keyed on shapes, stream and the weights' versions.  Larger passes (batch mode) keep the
# call-by-call route: their host time is hidden behind 60 ms of kernels and their intermediates would pin gigabytes.
FRAME_OPLISTS = True
# The correlation lookup fused into convc1 (rpe_corr_lookup_conv1x1: the 324-channel lookup result never leaves LDS; bit-identical to the
# two kernels) in the update loop's launch list, for passes of at most this many workgroups (64 queries each): ONE round of workgroups on
# the chip.  Measured at 640x512 (tools/bench_lookup_conv.py; fused vs lookup + convc1 back to back): 1 pair 33 vs 33 us, 2 pairs (a tracker
# frame: 160 workgroups) 35 vs 45, 4 pairs 67 vs 66, 8 pairs 103 vs 106, 16 pairs 171 vs 169, 32 pairs 331 vs 313 -- a workgroup takes
# 33 us wherever it runs (20 us of matrix instructions behind a lookup phase that nothing overlaps: its 150 KB of LDS give it the CU to
# itself), so the fusion pays exactly where the two kernels leave most of the chip idle.
LOOKUP_FUSED = True
LOOKUP_FUSED_MAX_WGS = 256
FRAME_OPLISTS_MAX_IMAGES = 4                                      # images per encoder pass / flow pairs per RAFT pass up to which passes are recorded
ENC_STREAMS = True                                                 # RAFT.encode_both: the context encoder on the side stream beside the feature encoder
ENC_STREAMS_MIN = 8                                                # ... for at least this many context images (below: the fork / join costs more than it hides)
SIDE_STREAM_MAX = 8 * 5120                                     # queries per pass (batch * h/8 * w/8) up to which the side stream is used
# Every constant above that selects a packing, a kernel, a tile class or a stream: _switches() is part of every key of what is built or
# recorded under them, so a switch flipped on a live model (tests, bench.py's A/B runs) is honoured by all of it at the next pass.
# (LOOP_OPLIST, LOOKUP_EVENT_SINK, FRAME_OPLISTS and FRAME_OPLISTS_MAX_IMAGES choose how launches are dispatched, not what is cached.)
ROUTE_SWITCHES = ('WINOGRAD', 'WINO_2X4', 'S2_M96', 'S2_M96_MIN_WGS', 'CORR_BF16X3', 'CONV_BF16X3', 'X3_MIN_CIN', 'X3_GRU', 'SIDE_STREAM', 'SIDE_STREAM_MAX',
                  'LOOKUP_FUSED', 'LOOKUP_FUSED_MAX_WGS', 'ENC_STREAMS', 'ENC_STREAMS_MIN', 'PAD_MAPS', 'PAD_ENCODERS', 'UPDATE_FP16')
_switch_values = operator.itemgetter(*ROUTE_SWITCHES)


def _switches():
    """The current values of ROUTE_SWITCHES (read from the module at every call: they are plain attributes that callers assign)."""
    return _switch_values(globals())


def padded_size(h8, w8):
    """The map the update loop's tuned kernels run (h8, w8) on under ``pad_maps``: the next size they take -- rows rounded up to an even count
    (the 2-row tiles of rpe_conv_wino / rpe_conv_wino24), row length to a multiple of 4 (whole 16-byte quads; F(2x4,3x3) needs no more than
    that, so a multiple of 8 buys nothing).  The identity on sizes they take as they are: (11,13) -> (12,16), (45,44) -> (46,44),
    (135,240) -> (136,240), (64,80) -> (64,80)."""
    return h8 + (h8 & 1), (w8 + 3) // 4 * 4


class Route(NamedTuple):
    """What a pass runs on, resolved once (resolve_route) and handed down: the six options as they take effect -- the config key, or for
    the last three the module switch -- and, for a pass of known size, what follows from them.  Hashable: ``options`` is part of every key
    of what is packed or recorded under it (beside _switches() and the sizes), so no option can be left out of a key."""
    mixed_precision: bool = False
    alternate_corr: bool = False
    alt_corr_fp16: bool = False
    pad_maps: bool = False
    pad_encoders: bool = False
    update_fp16: bool = False
    loop_pad: Optional[Tuple[int, int]] = None                 # the zero-padded map the update loop runs on; None = the 1/8 map itself
    enc_pad: Optional[Tuple[int, int]] = None                  # likewise of the encoders' layer2 / layer3 / output layer (in 1/8 cells)
    fused: Optional[bool] = None                               # the loop's map has rows of whole quads: the tuned kernels, not the generic route

    @property
    def options(self):
        return Route(*self[:6])


def _fused(w8, update_fp16):
    """Do the update block's tuned kernels take a map of this width (Route.fused)?  update_fp16 has no other route: refused."""
    if w8 % 4 != 0 and update_fp16:
        raise RpeError(f'RAFT: update_fp16 needs a 1/8 map with w % 4 == 0 (rpe_conv_f16), got w8 = {w8}; it does not run in f32 instead')
    return w8 % 4 == 0


def resolve_route(mixed_precision=False, alternate_corr=False, alt_corr_fp16=False, pad_maps=False, pad_encoders=False, update_fp16=False,
                  map_size=None, image_size=None):
    """The Route of a pass with these instance flags under the current module switches, on a 1/8 map ``map_size`` or an image
    ``image_size`` where known.  Every refusal of a combination is raised here and nowhere else, in this order, before anything is built
    or launched: at construction, at the start of every pass and of every encoder call -- so a switch flipped or a flag assigned on a
    live model is refused, or honoured, at the next pass."""
    pad_maps, pad_encoders, update_fp16 = bool(pad_maps or PAD_MAPS), bool(pad_encoders or PAD_ENCODERS), bool(update_fp16 or UPDATE_FP16)
    # the on-the-fly correlation is f32, or fp16 by its own flag
    if alt_corr_fp16 and not alternate_corr:
        raise RpeError('RAFT: alt_corr_fp16 selects the feature precision of alternate_corr and needs alternate_corr: True')
    if alternate_corr and (mixed_precision or CORR_BF16X3 or CONV_BF16X3):
        raise RpeError('RAFT: alternate_corr is f32 only (fp16 features: alt_corr_fp16) -- not with mixed_precision, CORR_BF16X3 or CONV_BF16X3')
    # the valid-extent entry points exist for the f32 Winograd / GEMM kernels only
    if pad_maps and (CONV_BF16X3 or not WINOGRAD):
        raise RpeError('RAFT: pad_maps runs on the f32 Winograd kernels -- not with CONV_BF16X3 (X3_GRU), not without WINOGRAD')
    if pad_encoders and (CONV_BF16X3 or not WINOGRAD):
        raise RpeError('RAFT: pad_encoders runs on the f32 Winograd kernels -- not with CONV_BF16X3, not without WINOGRAD')
    # update_fp16 runs its covered layers on rpe_conv_f16 or not at all; the f32 layers beside it (the context terms) are the headline's
    if update_fp16 and CONV_BF16X3:
        raise RpeError('RAFT: update_fp16 and CONV_BF16X3 are two precisions for the same layers -- choose one')
    if update_fp16 and not WINOGRAD:
        raise RpeError('RAFT: update_fp16 keeps its f32 layers on the Winograd kernels -- not with WINOGRAD = False')
    if update_fp16 and (pad_maps or pad_encoders):
        raise RpeError('RAFT: update_fp16 has no valid-extent form yet -- not with pad_maps / pad_encoders')
    options = (bool(mixed_precision), bool(alternate_corr), bool(alt_corr_fp16), pad_maps, pad_encoders, update_fp16)
    if image_size is not None:
        map_size = image_size[0] // 8, image_size[1] // 8
    if map_size is None:
        return Route(*options)
    padded = padded_size(*map_size)
    padded = None if padded == tuple(map_size) else padded
    loop_pad = padded if pad_maps else None
    # (the encoders pad whole 8x8 cells only: any other image keeps their generic route)
    enc_pad = padded if pad_encoders and image_size is not None and image_size[0] % 8 == 0 and image_size[1] % 8 == 0 else None
    return Route(*options, loop_pad, enc_pad, _fused((loop_pad or map_size)[1], update_fp16))


def _norm(kind, ch):
    if kind == 'batch':
        return nn.BatchNorm2d(ch)
    if kind == 'instance':
        return nn.InstanceNorm2d(ch)
    if kind == 'none':
        return nn.Sequential()
    raise ValueError(kind)


class ResidualBlock(nn.Module):
    def __init__(self, in_planes, planes, norm_fn='batch', stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1 = _norm(norm_fn, planes)
        self.norm2 = _norm(norm_fn, planes)
        if stride == 1:
            self.downsample = None
        else:
            self.norm3 = _norm(norm_fn, planes)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride), self.norm3)

    def takes_raw_input(self, x):
        """Can this block read its input as the RAW output of an instance-normalised convolution (+ its (mean, 1/std)), i.e. run
        conv1 with the loader-side normalisation and normalise the shortcut inside the last pass?  (fnet's first block behind the stem.)"""
        return (isinstance(self.norm1, nn.InstanceNorm2d) and self.downsample is None and _fusable(self.conv1, x) and x.shape[-1] % 4 == 0
                and _wino(self.conv1, x) is not None)

    def forward(self, x, x_norm=None, valid=None):
        """relu(x' + relu(norm2(conv2(relu(norm1(conv1 x)))))), x' = x or norm3(conv1x1 x); every convolution with its
        (bias, norm, ReLU, residual) epilogue fused (conv_norm_act).  With instance norm (fnet) norm1 + ReLU never exist
        as a tensor: conv1 leaves its raw output and partial sums, and conv2 normalises that input while staging it.
        ``x_norm`` (b,c,2): x is a raw convolution output whose relu((x - mean) * inv) is this block's real input (takes_raw_input).
        ``valid`` = (hv, wv) (pad_encoders): x and every map of the block are zero-padded, the block's OUTPUT map holds hv x wv of content;
        every launch takes its encoder valid-extent form, which keeps the padding zero and the moments on the content."""
        fused_in = isinstance(self.norm1, nn.InstanceNorm2d) and _fusable(self.conv1, x) and x.shape[-1] // self.conv1.stride[0] % 4 == 0
        if x_norm is not None and not (fused_in and self.takes_raw_input(x)):
            raise RuntimeError('ResidualBlock: x_norm needs the fused stride-1 Winograd route')
        if fused_in:
            st = self.conv1.stride[0]
            hw = (x.shape[-2] // st) * (x.shape[-1] // st) if valid is None else valid[0] * valid[1]       # (the pixel count of the moments)
            raw1, stats1 = _encoder_conv(self.conv1, x, pre_norm=x_norm, moments=True, valid=valid)   # (stride 1: Winograd, moments per 16x8-pixel patch)
            mi = ops.instnorm_finalize(stats1, hw, eps=self.norm1.eps, channels=self.conv1.out_channels)
            res_relu = True
            if self.downsample is not None:
                sc = self.downsample[0]
                if _fusable(sc, x):
                    # the shortcut norm3(conv1x1 x) never exists as a tensor either: its raw convolution output and (mean, 1/std) go to
                    # the block's last pass, which normalises it on the fly (bit-identical to a pass of its own, tested)
                    x, stats_sc = _encoder_conv(sc, x, moments=True, valid=valid)
                    x_norm = ops.instnorm_finalize(stats_sc, hw, eps=self.norm3.eps, channels=sc.out_channels)
                    res_relu = False
                else:
                    x = conv_norm_act(sc, self.norm3, x, relu=False)
            raw2, stats2 = _encoder_conv(self.conv2, raw1, pre_norm=mi, moments=True, valid=valid)
            if isinstance(stats2, ops.TileMajorStats):            # merge the Winograd kernel's records once (a small launch), then stream
                stats2 = ops.instnorm_finalize(stats2, hw, eps=self.norm2.eps, channels=self.conv2.out_channels)
            return ops.instnorm_apply(raw2, stats2, eps=self.norm2.eps, relu=True, residual=x, residual_norm=x_norm, residual_relu=res_relu, valid=valid)
        y = conv_norm_act(self.conv1, self.norm1, x, relu=True, valid=valid)
        if self.downsample is not None:
            x = conv_norm_act(self.downsample[0], self.norm3, x, relu=False, valid=valid)
        return conv_norm_act(self.conv2, self.norm2, y, relu=True, residual=x, valid=valid)


def _cached(owner, attr, key, make, with_key=False):
    """``make()`` kept on ``owner`` -- a module (as attribute ``attr``) or a workspace dict (as entry ``attr``) -- until ``key`` changes.
    ``with_key``: returns (key, value), for a caller whose own cache depends on this one and therefore keys on its key."""
    d = owner if isinstance(owner, dict) else owner.__dict__
    cached = d.get(attr)
    if cached is None or cached[0] != key:
        d[attr] = cached = (key, make())
    return cached if with_key else cached[1]


def _bn_affine(conv, norm):
    """Eval-mode BatchNorm2d folded with the conv bias: y = conv_nobias(x) * scale + shift (cached per module)."""
    def fold():
        scale = (norm.weight / torch.sqrt(norm.running_var + norm.eps)).detach().float().contiguous()
        return scale, ((conv.bias - norm.running_mean) * scale + norm.bias).detach().float().contiguous()
    return _cached(norm, '_rpe_affine', wkey(conv.bias, norm.weight, norm.bias, norm.running_mean, norm.running_var), fold)


def _packed(conv):
    """PackedConv of a module's weight (no bias), cached on the module until the weight changes."""
    return _cached(conv, '_rpe_packed', wkey(conv.weight), lambda: ops.PackedConv(conv.weight, None))


def _wino(conv, x):
    """PackedWino24 / PackedWino of a 3x3 stride-1 convolution when rpe_conv_wino24 / rpe_conv_wino can run it on this input (cached on
    the module), else None."""
    if not WINOGRAD or conv.stride != (1, 1) or conv.kernel_size != (3, 3) or conv.padding != (1, 1):
        return None
    if not ops.PackedWino.supported(conv.weight, x.shape[-2], x.shape[-1]) or conv.in_channels > 128 or not x.is_contiguous():
        return None
    kind = ops.PackedWino24 if WINO_2X4 and ops.PackedWino24.supported(conv.weight, x.shape[-2], x.shape[-1]) else ops.PackedWino
    return _cached(conv, '_rpe_wino', (wkey(conv.weight), kind), lambda: kind(conv.weight, None))


def _fusable(conv, x):
    """Can rpe_conv_fused / rpe_conv_wino run this encoder convolution on this input?  (3x3 stride 1; 3x3 pad 1 / 1x1 stride 2 on even
    maps; rows of whole 16-byte quads.)  Every launch size takes this route: the kernels pick smaller tiles for small launches
    themselves, and their results do not depend on that choice (tests/test_gpu_conv.py::*_agree_bitwise)."""
    _, _, hh, ww = x.shape
    s1 = conv.stride == (1, 1) and conv.kernel_size == (3, 3) and conv.padding == (1, 1)
    s2 = conv.stride == (2, 2) and hh % 2 == 0 and ww % 2 == 0 and \
        ((conv.kernel_size == (3, 3) and conv.padding == (1, 1)) or (conv.kernel_size == (1, 1) and conv.padding == (0, 0)))
    stride = 2 if s2 else 1
    return (s1 or s2) and ww % 4 == 0 and ((hh // stride) * (ww // stride)) % 4 == 0 and x.is_contiguous()


def conv_norm_act(conv, norm, x, relu, residual=None, valid=None):
    """norm(conv(x) + bias) [ReLU] [+ residual, ReLU].  The residual blocks' convolutions -- 3x3 stride 1, 3x3 stride 2 and
    the 1x1 stride-2 shortcut -- run on the fused HIP implicit GEMM when the map width is a multiple of 4 (folded batch
    norm / ReLU / residual inside its epilogue; for instance norm the epilogue leaves per-tile partial sums and one more
    read+write pass normalises); shapes those kernels refuse run on the generic kernel (ops.conv_direct) + a stand-alone epilogue pass.
    ``valid`` (pad_encoders): the extent of the content of the zero-padded output map, as ResidualBlock.forward."""
    fused = _fusable(conv, x)
    if isinstance(norm, nn.BatchNorm2d):
        if norm.training:
            raise RuntimeError('the RAFT encoders run with frozen batch norm (RAFT.freeze_bn, pose_net.py:22)')
        scale, shift = _bn_affine(conv, norm)
        if fused:                                              # (cnet's stride-1 3x3 layers: Winograd with the folded batch norm in the epilogue)
            return _encoder_conv(conv, x, ops.CONV_RELU if relu else ops.CONV_LINEAR, affine=(scale, shift), residual=residual, valid=valid)[0]
        return ops.affine_act(ops.conv_direct(x, conv.weight, None, conv.stride, conv.padding), scale, shift, relu=relu, residual=residual)
    if isinstance(norm, nn.InstanceNorm2d):
        if fused:
            pre, stats = _encoder_conv(conv, x, moments=True, valid=valid)
            return ops.instnorm_apply(pre, stats, eps=norm.eps, relu=relu, residual=residual, valid=valid)
        return ops.instnorm_act(ops.conv_direct(x, conv.weight, None, conv.stride, conv.padding), conv.bias, eps=norm.eps, relu=relu, residual=residual)
    raise NotImplementedError(type(norm))


def _encoder_conv(conv, x, mode=ops.CONV_LINEAR, affine=None, residual=None, pre_norm=None, moments=False, valid=None):
    """An encoder convolution that _fusable accepts, on the route its input allows: Winograd (rpe_conv_wino*) when _wino has a packing for
    it, else the fused implicit GEMM (rpe_conv_fused, which also takes stride 2 and the 1x1 shortcut).  The epilogue adds the conv bias, or
    with ``affine`` = (scale, shift) applies the folded batch norm; ``mode`` (LINEAR / RELU), ``residual`` and ``pre_norm`` as ops.conv_fused.
    Returns (the output, the per-tile moments for instnorm_finalize / instnorm_apply in the layout of the kernel that ran -- TileMajorStats
    from Winograd, channel-major records from the implicit GEMM -- when ``moments``, else None).  ``valid`` (pad_encoders) = the content of
    the zero-padded OUTPUT map: the kernels' encoder valid-extent forms (ops.conv_wino / conv_fused with enc_valid=)."""
    b, _, hh, ww = x.shape
    st, cout = conv.stride[0], conv.out_channels
    scale, bias = affine if affine is not None else (None, conv.bias.detach())
    pw = _wino(conv, x)
    out = torch.empty(b, cout, hh // st, ww // st, device=x.device)
    if pw is not None:
        stats = ops.conv_wino_stats_buffer(b, cout, hh, ww, x.device) if moments else None
        ops.conv_wino(x, pw, mode, out, scale=scale, bias=bias, residual=residual, stats=stats, pre_norm=pre_norm, enc_valid=valid)
    else:
        stats = ops.conv_stats_buffer(b, cout, hh, ww, x.device, stride=st) if moments else None
        m96 = S2_M96 and st == 2 and conv.kernel_size == (3, 3) and cout == 96 and b * -(-(hh // 2) * (ww // 2) // 128) >= S2_M96_MIN_WGS
        ops.conv_fused(x, _packed(conv), mode, out, scale=scale, bias=bias, residual=residual, stats=stats, stride=st, pre_norm=pre_norm,
                       entry='rpe_conv_fused_m96' if m96 else 'rpe_conv_fused', enc_valid=valid)
    return out, stats


def _recording(owner, root):
    """The set-up of a module that records its small passes: (``owner``'s cache of recorded passes, the wkey of every parameter and
    buffer below ``root``).  The (dict, name) slots are collected once and read afresh for every key, so a Parameter object that is
    REPLACED shows up, not only one that is updated in place."""
    d = owner.__dict__
    if d.get('_recorded') is None:
        d['_recorded'] = _Recorded()
    if '_key_tensors' not in d:
        d['_key_tensors'] = [(slots, n) for m in root.modules() for slots in (m._parameters, m._buffers) for n in slots]
    return d['_recorded'], wkey(*[slots[n] for slots, n in d['_key_tensors']])


def _overlap(tensors):
    spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in tensors)
    return any(a[1] > b[0] for a, b in zip(spans, spans[1:]))


class _Recorded:
    """A small cache of recorded passes (ops.Recorder) keyed by the caller; a key whose recording came out incomplete three times (a launch
    the recorder cannot carry: a fallback route, a weight packing made on first use) is given up on and stays on the call-by-call route."""

    def __init__(self, keep=4):
        self._progs, self._failed, self._keep = {}, {}, keep

    def get(self, key):
        return self._progs.get(key)

    def wanted(self, key):
        return self._failed.get(key, 0) < 3

    def put(self, key, rec):
        if rec.complete:
            bounded_put(self._progs, key, rec, keep=self._keep)
        else:
            if len(self._failed) > 64:
                self._failed.clear()
            self._failed[key] = self._failed.get(key, 0) + 1

    def clear(self):
        self._progs.clear()
        self._failed.clear()


class BasicEncoder(nn.Module):
    def __init__(self, output_dim=128, norm_fn='batch', dropout=0.0, pad_encoders=False):
        super().__init__()
        self.norm_fn = norm_fn
        self.pad_encoders = pad_encoders                       # RAFT's config key ``pad_encoders``, for an encoder called on its own (_route)
        self.norm1 = _norm(norm_fn, 64)
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        self.in_planes = 64
        self.layer1 = self._make_layer(64, stride=1)
        self.layer2 = self._make_layer(96, stride=2)
        self.layer3 = self._make_layer(128, stride=2)
        self.conv2 = nn.Conv2d(128, output_dim, kernel_size=1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d)):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _make_layer(self, dim, stride=1):
        l1 = ResidualBlock(self.in_planes, dim, self.norm_fn, stride=stride)
        l2 = ResidualBlock(dim, dim, self.norm_fn, stride=1)
        self.in_planes = dim
        return nn.Sequential(l1, l2)

    def _stem_pack(self):
        """conv1 + norm1 + ReLU run on the RAW 0..255 image: the normalisation 2*(x/255)-1 happens while the kernel stages its
        input patch (rpe_stem_conv)."""
        w = self.conv1.weight
        return _cached(self, '_stem_packed', wkey(w), lambda: ops.PackedStem(w))

    def _stem_many(self, images):
        """The stem over several image batches, written into batch slices of ONE output (no torch.cat of the inputs)."""
        ps = self._stem_pack()
        n = sum(im.shape[0] for im in images)
        hh, ww = images[0].shape[-2:]
        out = torch.empty(n, 64, hh // 2, ww // 2, device=images[0].device)
        bn = isinstance(self.norm1, nn.BatchNorm2d)
        if bn:
            if self.norm1.training:
                raise RuntimeError('the RAFT encoders run with frozen batch norm (RAFT.freeze_bn, pose_net.py:22)')
            scale, shift = _bn_affine(self.conv1, self.norm1)
        stats = None if bn else torch.empty(n, 64, ops.lib().rpe_stem_tiles(hh, ww, 2), 3, device=out.device)
        i = 0
        for im in images:
            k = im.shape[0]
            if bn:
                ops.stem_conv(im.contiguous(), ps, bias=shift, scale=scale, relu=True, out=out[i:i + k])
            else:
                ops.stem_conv(im.contiguous(), ps, bias=self.conv1.bias.detach(), relu=False, stats=stats[i:i + k], out=out[i:i + k])
            i += k
        if bn:
            return out, None
        if self.layer1[0].takes_raw_input(out):               # norm1 + ReLU happen inside layer1's first block (its loader and its last pass)
            return out, ops.instnorm_finalize(stats, (hh // 2) * (ww // 2), eps=self.norm1.eps, channels=64)
        return ops.instnorm_apply(out, stats, eps=self.norm1.eps, relu=True), None

    def _final(self, x, split_act, valid=None):
        """conv2, the 1x1 output layer (128 -> output_dim), on the implicit GEMM.  ``split_act`` (the context encoder as RAFT uses
        it, core/RAFT/core/raft.py: net, inp = split(cnet); net = tanh(net); inp = relu(inp)): channels [0, 128) leave through
        tanh, the rest through ReLU, in the convolution's epilogue.  ``valid`` (pad_encoders): x is a zero-padded map with that much content;
        the layer runs on it (rpe_conv1x1_v) and the result leaves cropped and contiguous (rpe_copy_rect)."""
        m = self.conv2
        b, _, hh, ww = x.shape
        half = m.out_channels // 2
        if ww % 4 == 0 and x.is_contiguous():
            def pack():
                w, bv = m.weight.detach(), m.bias.detach()
                return ops.Conv1x1(w, bv), ops.Conv1x1(w[:half].contiguous(), bv[:half].contiguous()), ops.Conv1x1(w[half:].contiguous(), bv[half:].contiguous())
            whole, lo, hi = _cached(self, '_final_packed', wkey(m.weight, m.bias), pack)
            out = torch.empty(b, m.out_channels, hh, ww, device=x.device)
            if not split_act:
                whole(x, ops.CONV_LINEAR, out, x3=CONV_BF16X3, valid=valid)
            else:
                lo(x, ops.CONV_TANH, out[:, :half], valid=valid)
                hi(x, ops.CONV_RELU, out[:, half:], x3=CONV_BF16X3, valid=valid)
            if valid is not None:
                self._ws['out'] = out
                return ops.copy_rect(out, torch.empty(b, m.out_channels, *valid, device=x.device), *valid)
            return out
        y = ops.conv_direct(x, m.weight, m.bias, 1, 0)           # (maps whose rows are not whole 16-byte quads)
        if split_act:
            y[:, :half] = torch.tanh(y[:, :half])
            ops.bias_act(y[:, half:].contiguous(), None, relu=True, out=y, out_offset=half)
        return y

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self.__dict__.pop('_key_tensors', None)                # .to() / .float(): the recorded passes point at the old storage
        if getattr(self, '_recorded', None) is not None:
            self._recorded.clear()
        return r

    def forward(self, x, raw255=False, split_act=False, route=None):
        """``raw255``: x is the raw 0..255 image (RAFT.forward's normalisation is then done inside the first kernel), or a list of
        such image batches, encoded as one batch.  ``split_act``: see _final.  ``route``: the pass's Route (RAFT hands it down; an encoder
        called on its own resolves its own flag).
        Small inference passes (FRAME_OPLISTS) are recorded once per (shapes, stream, weights, route) and replayed as one launch list."""
        images = list(x) if isinstance(x, (list, tuple)) else [x]
        first = images[0]
        if route is None:
            route = resolve_route(pad_encoders=self.pad_encoders, image_size=first.shape[-2:])
        if FRAME_OPLISTS and raw255 and first.is_cuda and first.device.index == torch.cuda.current_device() and not torch.is_grad_enabled() \
                and sum(im.shape[0] for im in images) <= FRAME_OPLISTS_MAX_IMAGES \
                and all(im.is_contiguous() and im.dtype == torch.float32 and im.device == first.device for im in images) and not _overlap(images):
            recorded, wkey = _recording(self, self)
            key = (tuple(tuple(im.shape) for im in images), first.device.index, ops.raw_stream(), split_act, _switches(), self.training, wkey, route.options)
            rec = recorded.get(key)
            if rec is not None:
                out = torch.empty(rec.out_shape, device=first.device)
                rec.replay({**{i: im for i, im in enumerate(images)}, 'out': out})
                return out
            if recorded.wanted(key):
                rec = ops.Recorder()
                with rec:
                    out = self._forward(x, raw255, split_act, route.enc_pad)
                if rec.complete and out.is_contiguous():
                    for i, im in enumerate(images):
                        rec.complete = rec.complete and rec.bind(i, im) > 0
                    rec.complete = rec.complete and rec.bind('out', out) > 0
                    rec.out_shape = tuple(out.shape)
                recorded.put(key, rec)
                return out
        return self._forward(x, raw255, split_act, route.enc_pad)

    def _forward(self, x, raw255, split_act, padded):
        """``padded`` = Route.enc_pad: layer2, layer3 and the output layer on maps zero-padded to that many 1/8 cells (pad_encoders)."""
        many = isinstance(x, (list, tuple))
        first = x[0] if many else x
        hh, ww = first.shape[-2:]
        stem_ok = raw255 and hh % 2 == 0 and ww % 2 == 0 and ((hh // 2) * (ww // 2)) % 4 == 0 and isinstance(self.norm1, (nn.BatchNorm2d, nn.InstanceNorm2d))
        x_norm = None
        if stem_ok:
            x, x_norm = self._stem_many(list(x) if many else [x])
        else:
            x = (torch.cat(list(x), dim=0) if many else x).contiguous()
            x = conv_norm_act(self.conv1, self.norm1, 2 * (x / 255.0) - 1.0 if raw255 else x, relu=True)
        x = self.layer1[1](self.layer1[0](x, x_norm))
        if padded is None:
            x = self.layer3(self.layer2(x))
            return self._final(x, split_act)
        # pad_encoders: layer1's output enters the zero-padded pitch by one strided copy; from here every map is P2 / P4 / P8 with the true
        # 1/2, 1/4, 1/8 map as content, every stride-2 layer keeps input = 2 x output, and every launch stores zero outside the content
        (hp, wp), h8, w8 = padded, hh // 8, ww // 8
        ws = self._ws = dict(valid=(h8, w8), p2=self._p2(x.shape[0], 4 * hp, 4 * wp, (4 * h8, 4 * w8), x.device))
        x = ops.copy_rect(x, ws['p2'], 4 * h8, 4 * w8)
        for name, layer, v in (('l2', self.layer2, (2 * h8, 2 * w8)), ('l3', self.layer3, (h8, w8))):
            ws[name] = x = layer[1](layer[0](x, valid=v), valid=v)
        return self._final(x, split_act, valid=(h8, w8))

    def _padded(self, hh, ww):
        """Route.enc_pad of this encoder called on its own on an (hh, ww) image: its flag (or PAD_ENCODERS), nothing else set."""
        return resolve_route(pad_encoders=self.pad_encoders, image_size=(hh, ww)).enc_pad

    def _p2(self, n, h2, w2, content, device):
        """The zero-filled 64-channel map layer1's output is copied into: allocated and cleared once per (batch, size, content, device: two image sizes may share a padded size) -- the copy
        writes the content only and nothing else writes it, so its padding stays zero pass after pass (single-stream use, as RAFT._workspace).
        A recorded pass keeps the one it was recorded with."""
        cache = self.__dict__.setdefault('_p2_cache', {})
        key = (n, h2, w2, content, str(device))
        if key not in cache:
            bounded_put(cache, key, torch.zeros(n, 64, h2, w2, device=device), keep=2)
        return cache[key]


class FlowHead(nn.Module):
    def __init__(self, input_dim=128, hidden_dim=256):
        super().__init__()
        self.conv1 = nn.Conv2d(input_dim, hidden_dim, 3, padding=1)
        self.conv2 = nn.Conv2d(hidden_dim, 2, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.conv2(self.relu(self.conv1(x)))


class SepConvGRU(nn.Module):
    """Parameters as upstream; the forward lives in BasicUpdateBlock.step (fused with the HIP gate kernels)."""

    def __init__(self, hidden_dim=128, input_dim=192 + 128):
        super().__init__()
        c = hidden_dim + input_dim
        self.convz1 = nn.Conv2d(c, hidden_dim, (1, 5), padding=(0, 2))
        self.convr1 = nn.Conv2d(c, hidden_dim, (1, 5), padding=(0, 2))
        self.convq1 = nn.Conv2d(c, hidden_dim, (1, 5), padding=(0, 2))
        self.convz2 = nn.Conv2d(c, hidden_dim, (5, 1), padding=(2, 0))
        self.convr2 = nn.Conv2d(c, hidden_dim, (5, 1), padding=(2, 0))
        self.convq2 = nn.Conv2d(c, hidden_dim, (5, 1), padding=(2, 0))


class BasicMotionEncoder(nn.Module):
    def __init__(self, corr_levels=4, corr_radius=4):
        super().__init__()
        cor_planes = corr_levels * (2 * corr_radius + 1) ** 2
        self.convc1 = nn.Conv2d(cor_planes, 256, 1, padding=0)
        self.convc2 = nn.Conv2d(256, 192, 3, padding=1)
        self.convf1 = nn.Conv2d(2, 128, 7, padding=3)
        self.convf2 = nn.Conv2d(128, 64, 3, padding=1)
        self.conv = nn.Conv2d(64 + 192, 128 - 2, 3, padding=1)

    def flow_branch(self, flow, P, L):
        """convf1 -> convf2 of the fused route (``P`` = BasicUpdateBlock.packed_convs, ``L`` = its launchers): depends on the flow only, not
        on the correlation lookup, so it may run on a side stream beside lookup -> convc1 -> convc2."""
        ops.stem_conv(flow, P['convf1'], bias=self.convf1.bias.detach(), relu=True, div=1.0, mul=1.0, sub=0.0, out=L.flo, **L.vk)   # 7x7 on 2 channels
        L.f2()

    def forward(self, flow, corr, cat_buf, hx, rhx):
        """The generic route (no packed_convs): writes relu(conv(cat[cor, flo])) (126 ch) and flow (2 ch) into channels [128,256) of hx and
        rhx -- the generic convolution (ops.conv_direct) without bias, rpe_bias_act for the rest."""
        def cv(m, x):
            return ops.conv_direct(x, m.weight, None, m.stride, m.padding)
        cor = ops.bias_act(cv(self.convc1, corr), self.convc1.bias)
        ops.bias_act(cv(self.convc2, cor), self.convc2.bias, out=cat_buf, out_offset=0)
        flo = ops.bias_act(cv(self.convf1, flow), self.convf1.bias)
        ops.bias_act(cv(self.convf2, flo), self.convf2.bias, out=cat_buf, out_offset=192)
        ops.bias_act(cv(self.conv, cat_buf), self.conv.bias, out=hx, out_offset=128, out2=rhx, out2_offset=128)
        ops.bias_act(flow, None, relu=False, out=hx, out_offset=254, out2=rhx, out2_offset=254)


class BasicUpdateBlock(nn.Module):
    def __init__(self, corr_levels=4, corr_radius=4, hidden_dim=128):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.route = resolve_route()                           # the options of the pass's Route (RAFT._route sets them: at construction, at every pass)
        self.encoder = BasicMotionEncoder(corr_levels, corr_radius)
        self.gru = SepConvGRU(hidden_dim=hidden_dim, input_dim=128 + hidden_dim)
        self.flow_head = FlowHead(hidden_dim, hidden_dim=256)
        self.mask = nn.Sequential(nn.Conv2d(128, 256, 3, padding=1), nn.ReLU(inplace=True),
                                  nn.Conv2d(256, 64 * 9, 1, padding=0))

    def gate_weights(self, with_key=False):
        """GRU conv weights re-arranged once (cached until a parameter changes):
          * convz|convr stacked on the output-channel axis (they read the same input),
          * input channels split into the loop-varying part [h | motion | flow] (256 ch) and the context part
            `inp` (128 ch, identical in every GRU iteration).
        Returns dict name -> (w_var, w_ctx, bias) for 'zr1', 'q1', 'zr2', 'q2'."""
        g, c = self.gru, self.hidden_dim

        def split(w):                          # (out, 384, kh, kw) -> varying (out,256,..), context (out,128,..)
            return torch.cat((w[:, :c], w[:, 2 * c:]), 1).detach().contiguous(), w[:, c:2 * c].detach().contiguous()

        def stack():
            W = {}
            for name, convs in (('zr1', (g.convz1, g.convr1)), ('q1', (g.convq1,)), ('zr2', (g.convz2, g.convr2)), ('q2', (g.convq2,))):
                w = torch.cat([m.weight for m in convs], 0)
                bvec = torch.cat([m.bias for m in convs], 0).detach().contiguous()
                W[name] = (*split(w), bvec)
            return W
        key = wkey(*[t for m in (g.convz1, g.convr1, g.convq1, g.convz2, g.convr2, g.convq2) for t in (m.weight, m.bias)])
        return _cached(self, '_stacked', key, stack, with_key)

    def context_terms(self, inp, out=None):
        """conv(inp; context channels) + bias of the four GRU convolutions: loop-invariant, computed once per pass.
        ``out`` = dict of persistent destination buffers (RAFT._workspace): the fused HIP convolution writes into them, so
        the GRU loop's prepared launchers see the same addresses pass after pass."""
        W = self.gate_weights()
        P = self.packed_convs(inp.shape[-1]) if out is not None else None
        if P is not None:
            for k in W:
                (ops.conv_wino1d if isinstance(P['ctx_' + k], ops.PackedWino1d) else ops.conv_fused)(inp, P['ctx_' + k], ops.CONV_LINEAR, out[k])
            return out
        pads = {'zr1': (0, 2), 'q1': (0, 2), 'zr2': (2, 0), 'q2': (2, 0)}
        return {k: ops.conv_direct(inp, W[k][1], W[k][2], 1, pads[k]) for k in W}

    def fp16(self):
        """This pass runs the covered layers on rpe_conv_f16 (the config key, or the module switch)."""
        return self.route.update_fp16

    update_fp16 = property(fp16)

    def packed_convs(self, width, with_key=False):
        """Weights of the update block's convolutions in rpe_conv_fused's layout (cached until a parameter, the stacked gate weights or a
        route switch changes), or None when the fused kernels do not apply (map width not a multiple of 4)."""
        if not _fused(width, self.fp16()):                      # (a pass has this from its Route; a caller of its own asks here)
            return (None, None) if with_key else None
        e, fh = self.encoder, self.flow_head
        mods = (e.convc1, e.convc2, e.convf2, e.conv, fh.conv1)
        gate_key, W = self.gate_weights(with_key=True)
        # (the convolutions' own weight / bias attributes: walking module.parameters() costs ~100 us a call, and this runs 26 times a frame)
        key = (wkey(*[t for m in mods + (e.convf1,) for t in (m.weight, m.bias)]), gate_key, _switches(), self.route)
        return _cached(self, '_packed', key, lambda: self._pack_convs(mods, W), with_key)

    def _pack_convs(self, mods, W):
        """packed_convs' dict for the layers ``mods`` and the stacked gate weights ``W``, under the current route switches."""
        e = self.encoder
        P = {n: ops.PackedConv(m.weight, m.bias) for n, m in zip(('convc1', 'convc2', 'convf2', 'conv', 'fh1'), mods)}
        # the four 3x3 layers also in Winograd form (rpe_conv_wino: 2.25x fewer matrix FLOPs); used on even maps
        P['wino'] = {n: ops.PackedWino(m.weight, m.bias) for n, m in zip(('convc2', 'convf2', 'conv', 'fh1'), mods[1:])
                     if ops.PackedWino.supported(m.weight, 2, 2)} if WINOGRAD else {}
        # and as F(2x4,3x3) (rpe_conv_wino24: a quarter fewer products), used on maps with w % 4 == 0; not under the labelled variant
        P['wino24'] = {n: ops.PackedWino24(m.weight, m.bias) for n, m in zip(('convc2', 'convf2', 'conv', 'fh1'), mods[1:])
                       if ops.PackedWino24.supported(m.weight, 2, 4)} if (WINOGRAD and WINO_2X4 and not CONV_BF16X3) else {}
        # the labelled bf16x3 variant's packings of the same layers (used on maps rpe_conv_wino_x3 accepts: even h, w % 4 == 0)
        P['wino_x3'] = {n: ops.PackedWinoX3(m.weight, m.bias) for n, m in zip(('convc2', 'convf2', 'conv', 'fh1'), mods[1:])
                        if n != 'convf2' and m.in_channels >= X3_MIN_CIN and ops.PackedWinoX3.supported(m.weight, 2, 4)} if (WINOGRAD and CONV_BF16X3) else {}
        P['convf1'] = ops.PackedStem(e.convf1.weight)
        P['convc1_1x1'] = ops.Conv1x1(e.convc1.weight, e.convc1.bias)
        for n in ('zr1', 'q1', 'zr2', 'q2'):
            # the loop-varying 256 channels: Winograd F(4,5) along the filter axis (rpe_conv_wino1d: 2.5x fewer matrix FLOPs), else the
            # direct implicit GEMM; bias is part of the context term (context_terms)
            # (under CONV_BF16X3 with X3_GRU: the labelled variant's packing -- rpe_conv_wino1d_x3; packed_convs only runs for widths it accepts)
            P[n] = (ops.PackedWino1dX3 if CONV_BF16X3 and X3_GRU and ops.PackedWino1dX3.supported(W[n][0], 4) else ops.PackedWino1d)(W[n][0]) if WINOGRAD \
                else ops.PackedConv(W[n][0])
            P['ctx_' + n] = (ops.PackedWino1d if WINOGRAD else ops.PackedConv)(W[n][1], W[n][2])
        if self.fp16():
            # update_fp16: the covered layers' weights as fp16 matrix fragments (rpe_conv_f16); the gate convolutions' loop-varying 256
            # input channels only -- the context terms above stay f32 and enter as ``add``
            # (made when launchers are first built from this dict, like convc1's lookup-fused packing: kept as long as the dict)
            made = {}

            def f16():
                if not made:
                    made.update({n: ops.PackedConvF16(m.weight, m.bias) for n, m in zip(('convc1', 'convc2', 'convf2', 'conv', 'fh1'), mods)})
                    made.update({n: ops.PackedConvF16(W[n][0]) for n in ('zr1', 'q1', 'zr2', 'q2')})
                return made
            P['f16'] = f16
        scratch = {}

        def buf(name, like, c):                            # scratch for intermediate activations, one set per workspace (``like`` is one of
            k = (name, like.data_ptr(), like.shape[0], c, like.shape[2], like.shape[3], like.device)   # RAFT._workspace's buffers)
            if k not in scratch:
                bounded_put(scratch, k, torch.empty(like.shape[0], c, like.shape[2], like.shape[3], device=like.device), keep=12)
            return scratch[k]
        P['cor_buf'] = lambda like: buf('cor', like, 256)
        P['fh_buf'] = lambda like: buf('fh', like, 256)
        P['flo_buf'] = lambda like: buf('flo', like, 128)
        return P

    def launchers(self, ws, pyr=None, with_key=False):
        """Prepared launchers of the fused route's update on workspace ``ws`` (RAFT._workspace), built once and cached in ``ws`` until the
        packed weights change (every iteration of every pass on the workspace reuses them): c1, c2, f1, f2, cv (the motion encoder's convc1,
        convc2, convf1, convf2, conv; flo = convf1's output) and gru (the four GRU convolutions, FlowHead.conv1 and the flow head's output
        layer, which updates ws['coords1'] in place and writes flow = coords1 - grid into ws['flow'] and behind the motion features of hx /
        rhx).  With the pyramid ``pyr`` (the launch list's route) also lookup on coords1 and lookup_c1: lookup -> convc1 -> ReLU as one
        launch where that pays (LOOKUP_FUSED), else None."""
        packed_key, P = self.packed_convs(ws['hx'].shape[-1], with_key=True)
        alt = isinstance(pyr, ops.AltCorr)                  # (alternate_corr: lookup into the cor buffer, then convc1 -- LOOKUP_FUSED does not apply)
        key = (packed_key, None if pyr is None else (pyr.buf.data_ptr(), 'fp16' if alt and pyr.fp16 else alt), ws.get('valid'))
        return _cached(ws, '_launchers', key, lambda: self._make_launchers(ws, P, pyr, alt), with_key)

    def _make_launchers(self, ws, P, pyr, alt):
        hx, rhx, z_buf, cat_buf, corr, coords1, flow, ctx = (ws[k] for k in ('hx', 'rhx', 'z', 'cat', 'corr', 'coords1', 'flow', 'ctx'))
        c = self.hidden_dim
        e, fh = self.encoder, self.flow_head
        cor, flo, fh_buf = P['cor_buf'](corr), P['flo_buf'](corr), P['fh_buf'](hx)
        # pad_maps: the buffers are zero-padded maps with ``valid`` = (h8, w8) of content; every launch below then takes its entry point's
        # valid-extent form, whose epilogue stores zero in the padding (None = the maps are the content: the plain entry points)
        valid = ws.get('valid')
        # (stem_conv, flow_update and the lookup get the keyword only when set: bench.py --full and tests wrap them with the signatures of before this route)
        vk = {} if valid is None else dict(valid=valid)
        wino = dict(P['wino']) if hx.shape[-1] % 2 == 0 and hx.shape[-2] % 2 == 0 else {}
        if wino and hx.shape[-1] % 4 == 0:
            wino.update(P['wino24'])
            wino.update(P['wino_x3'])                      # (CONV_BF16X3: conv_wino runs the kernel that belongs to the packing)
        f16 = P['f16']() if 'f16' in P else None            # update_fp16: every covered layer on rpe_conv_f16 (never on padded maps: resolve_route)

        def c3(name, x, out, out2=None):                    # a 3x3 layer: Winograd when available, else the direct implicit GEMM
            if f16 is not None:
                return ops.conv_fused(x, f16[name], ops.CONV_RELU, out, out2=out2, prepare=True)
            if name in wino:
                return ops.conv_wino(x, wino[name], ops.CONV_RELU, out, out2=out2, prepare=True, valid=valid)
            return ops.conv_fused(x, P[name], ops.CONV_RELU, out, out2=out2, prepare=True)
        # each GRU half = two implicit-GEMM convolutions whose epilogues are the gates:
        #   z = s(convz hx + ctx), r*h -> rhx ;  h <- (1-z) h + z tanh(convq rhx + ctx)   (in place on hx[:, :c])
        gconv = ops.conv_wino1d if isinstance(P['zr1'], (ops.PackedWino1d, ops.PackedWino1dX3)) else ops.conv_fused
        if f16 is not None:
            P, gconv = dict(P, **{n: f16[n] for n in ('zr1', 'q1', 'zr2', 'q2')}), ops.conv_fused
        gru = []
        for zr, q in (('zr1', 'q1'), ('zr2', 'q2')):
            gru.append(gconv(hx, P[zr], ops.CONV_GATE_ZR, z_buf, out2=rhx[:, :c], add=ctx[zr], hidden=hx[:, :c], gate_channels=c, prepare=True, valid=valid))
            gru.append(gconv(rhx, P[q], ops.CONV_GATE_H, hx[:, :c], add=ctx[q], hidden=hx[:, :c], zgate=z_buf, prepare=True, valid=valid))
        gru.append(c3('fh1', hx[:, :c], fh_buf))
        gru.append(ops.flow_update(fh_buf, fh.conv2.weight, fh.conv2.bias.detach(), coords1, coords1, flow_out=flow, dst1=hx[:, 2 * c - 2:],
                                   dst2=rhx[:, 2 * c - 2:], prepare=True, **vk))
        L = SimpleNamespace(flo=flo, vk=vk, c1=P['convc1_1x1'](corr, ops.CONV_RELU, cor, prepare=True, x3=CONV_BF16X3, valid=valid) if f16 is None else
                            ops.conv_fused(corr, f16['convc1'], ops.CONV_RELU, cor, prepare=True), c2=c3('convc2', cor, cat_buf[:, :192]),
                            f1=ops.stem_conv(flow, P['convf1'], bias=e.convf1.bias.detach(), relu=True, div=1.0, mul=1.0, sub=0.0, out=flo, prepare=True, **vk),
                            f2=c3('convf2', flo, cat_buf[:, 192:]), cv=c3('conv', cat_buf, hx[:, 128:254], rhx[:, 128:254]), gru=gru)
        if pyr is not None:
            # (pad_maps: the pyramid and the taps keep the true (h8, w8); coords and the 324 channels live in the padded maps)
            L.lookup, L.lookup_c1 = pyr.lookup(coords1, out=corr, prepare=True, **({} if valid is None else dict(map_size=tuple(hx.shape[-2:])))), None
            n_wgs = hx.shape[0] * -(-(hx.shape[2] * -(-hx.shape[3] // 8)) // 8)
            if valid is None and not alt and LOOKUP_FUSED and not CONV_BF16X3 and f16 is None and n_wgs <= LOOKUP_FUSED_MAX_WGS and ops.PackedLookupConv.supported(pyr.levels, pyr.radius, pyr.w8):
                # (convc1 in the fused kernel's layout: made when a pass first takes this route, kept while convc1 stays as it is)
                pl = _cached(self, '_lookup_packed', wkey(e.convc1.weight, e.convc1.bias), lambda: ops.PackedLookupConv(e.convc1.weight, e.convc1.bias))
                L.lookup_c1 = pyr.lookup_conv1x1(coords1, pl, cor, relu=True, prepare=True)
        return L

    def step(self, ws, ctx, flow, coords1, h_buf, flow_branch_done=None):
        """One update on workspace ``ws``: hx = (h | motion | flow), rhx = (r*h | motion | flow), both (b,256,h,w); ctx = context_terms();
        the new hidden state is left in hx[:, :128].  Fused route (packed_convs): the workspace's launchers, ``coords1`` and ``flow`` are its
        persistent buffers and the flow head's output layer updates them in place (no subtract / copy launches); ``flow_branch_done``: an
        event recorded behind flow_branch() on another stream (it then is not run here).  Generic route: returns coords1 + delta_flow and
        writes h_buf (the fused flow head reads the slice directly)."""
        c = self.hidden_dim
        hx, rhx, z_buf, cat_buf, corr = (ws[k] for k in ('hx', 'rhx', 'z', 'cat', 'corr'))
        P = self.packed_convs(hx.shape[-1])
        if P is not None:
            L = self.launchers(ws)
            L.c1(); L.c2()
            if flow_branch_done is None:
                self.encoder.flow_branch(flow, P, L)
            else:
                torch.cuda.current_stream().wait_event(flow_branch_done)
            L.cv()
            for launch in L.gru:
                launch()
            return coords1
        self.encoder(flow, corr, cat_buf, hx, rhx)
        fh = self.flow_head
        W = self.gate_weights()
        # horizontal half: z = s(convz1 hx), r = s(convr1 hx), q = tanh(convq1 [r*h, x]), h = (1-z) h + z q
        zr = ops.conv_direct(hx, W['zr1'][0], None, 1, (0, 2))
        ops.gru_gates_zr(zr, hx, c, z_buf, rhx, add=ctx['zr1'])
        q = ops.conv_direct(rhx, W['q1'][0], None, 1, (0, 2))
        ops.gru_gates_h(z_buf, q, hx, c, hx, add=ctx['q1'])
        # vertical half
        zr = ops.conv_direct(hx, W['zr2'][0], None, 1, (2, 0))
        ops.gru_gates_zr(zr, hx, c, z_buf, rhx, add=ctx['zr2'])
        q = ops.conv_direct(rhx, W['q2'][0], None, 1, (2, 0))
        ops.gru_gates_h(z_buf, q, hx, c, hx, add=ctx['q2'])
        h_buf.copy_(hx[:, :c])                                            # contiguous h for the heads
        t = ops.conv_direct(h_buf, fh.conv1.weight, fh.conv1.bias, 1, 1, relu=True)
        return ops.conv3x3_to2(t, fh.conv2.weight, fh.conv2.bias, add=coords1)      # coords1 + delta_flow

    def up_mask(self, net):
        """.25 * mask(net) (upstream scales the mask to balance gradients).  The 3x3 layer + ReLU runs on the Winograd kernel, the
        factor is folded into the 1x1 layer's parameters (a power of two: bit-identical to scaling the result)."""
        c1, c2 = self.mask[0], self.mask[2]
        mp = (c1.weight, c1.bias, c2.weight, c2.bias)
        hh, ww = net.shape[-2:]
        x3 = CONV_BF16X3 and c1.in_channels >= X3_MIN_CIN and ops.PackedWinoX3.supported(c1.weight, hh, ww)
        w24 = WINO_2X4 and not CONV_BF16X3 and ops.PackedWino24.supported(c1.weight, hh, ww)
        if self.fp16() and c1.weight.is_cuda:
            # update_fp16: both layers on rpe_conv_f16, the x0.25 fold kept (a power of two: it commutes with the fp16 rounding of normal weights)
            p1, p2 = _cached(self, '_mask_packed', (wkey(*mp), 'f16', _switches()), lambda: (
                ops.PackedConvF16(c1.weight, c1.bias), ops.PackedConvF16((0.25 * c2.weight).detach(), (0.25 * c2.bias).detach())))
            t = ops.conv_fused(net, p1, ops.CONV_RELU, torch.empty(net.shape[0], c1.out_channels, hh, ww, device=net.device))
            return ops.conv_fused(t, p2, ops.CONV_LINEAR, torch.empty(net.shape[0], c2.out_channels, hh, ww, device=net.device))

        def pack():
            pw = (ops.PackedWinoX3 if x3 else ops.PackedWino24 if w24 else ops.PackedWino)(c1.weight, c1.bias) if WINOGRAD and c1.weight.is_cuda else None
            w2, b2 = (0.25 * c2.weight).detach(), (0.25 * c2.bias).detach()
            return pw, w2, b2, ops.Conv1x1(w2, b2) if c2.weight.is_cuda else None
        pw, w2, b2, p2 = _cached(self, '_mask_packed', (wkey(*mp), x3, w24, _switches()), pack)
        if pw is not None and not torch.is_grad_enabled() and hh % 2 == 0 and ww % 2 == 0:      # (net may be a channel slice: hx[:, :128]; pad_maps: of a padded map)
            t = ops.conv_wino(net, pw, ops.CONV_RELU, torch.empty(net.shape[0], c1.out_channels, hh, ww, device=net.device))
        else:
            t = ops.conv_direct(net, c1.weight, c1.bias, 1, 1, relu=True)
        if p2 is not None and ww % 4 == 0 and not torch.is_grad_enabled():
            return p2(t, ops.CONV_LINEAR, torch.empty(net.shape[0], c2.out_channels, hh, ww, device=net.device), x3=CONV_BF16X3)
        return ops.conv_direct(t, w2, b2, 1, 0)


def coords_grid(batch, ht, wd, device):
    ys, xs = torch.meshgrid(torch.arange(ht, device=device), torch.arange(wd, device=device), indexing='ij')
    return torch.stack((xs, ys), dim=0).float()[None].repeat(batch, 1, 1, 1)


class RAFT(nn.Module):
    def __init__(self, config):
        super().__init__()
        if config.get('small', False):
            raise NotImplementedError("RAFT-small is not on the reference's inference path (train.yaml:5 small: False)")
        self.config = config
        # upstream RAFT's ``mixed_precision`` runs the encoders under autocast, i.e. hands fp16 feature maps to the
        # correlation (BASELINE config 5 "fp16 features").  Here the encoders stay f32 and the feature maps are rounded to
        # fp16 where the correlation consumes them (16-bit matrix cores, f32 accumulation, f32 pyramid).
        self.mixed_precision = bool(config.get('mixed_precision', False))
        # upstream RAFT's ``alternate_corr``: no all-pairs volume; every iteration recomputes its correlation windows from the feature maps
        # (ops.AltCorr, csrc/corr_alt.hip).  Opt-in, f32 only -- or, with ``alt_corr_fp16`` (needs alternate_corr), BASELINE config 5 on this
        # route: the feature maps rounded to fp16 in the scratch (half its bytes), the window products on the 16-bit matrix cores, f32
        # accumulation and blend.  ``mixed_precision`` keeps meaning the pyramid route's fp16 build and stays refused with alternate_corr.
        self.alternate_corr = bool(config.get('alternate_corr', False))
        self.alt_corr_fp16 = bool(config.get('alt_corr_fp16', False))
        # ``pad_maps`` (opt-in): at 1/8 maps the tuned kernels refuse -- odd heights, rows that are not whole 16-byte quads -- the update loop runs
        # on maps zero-padded to padded_size(h8, w8) instead of on the generic convolution; the encoders keep the generic route there.
        self.pad_maps = bool(config.get('pad_maps', False))
        # ``pad_encoders`` (opt-in): at the same sizes both encoders run layer2, layer3 and the output layer on zero-padded maps (Route.enc_pad)
        self.pad_encoders = bool(config.get('pad_encoders', False))
        # ``update_fp16`` (opt-in): the update block's convolutions with fp16 operands on the 16-bit matrix cores (UPDATE_FP16 above names the
        # covered layers and the contract) -- what a user of upstream RAFT's mixed_precision expects of the update block.  Allowed together
        # with mixed_precision and with alternate_corr [+ alt_corr_fp16], which keep their own meaning (the correlation's feature maps).
        self.update_fp16 = bool(config.get('update_fp16', False))
        self.iters = int(config.get('iters', 12))
        self.hidden_dim = self.context_dim = 128
        self.corr_levels, self.corr_radius = 4, 4
        drop = config.get('dropout', 0.0)
        self.fnet = BasicEncoder(output_dim=256, norm_fn='instance', dropout=drop, pad_encoders=self.pad_encoders)
        self.cnet = BasicEncoder(output_dim=256, norm_fn='batch', dropout=drop, pad_encoders=self.pad_encoders)
        self.update_block = BasicUpdateBlock(self.corr_levels, self.corr_radius, hidden_dim=128)
        self._route()                                          # (refuses what does not go together)
        self._pyr = None
        self._ws = None

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    def _side_stream(self, device):
        s = getattr(self, '_side', None)
        if s is None or s[0].device != device:
            with torch.cuda.device(device):
                self._side = s = (torch.cuda.Stream(device=device), torch.cuda.Event(), torch.cuda.Event())
        return s

    def _route(self, map_size=None, image_size=None):
        """The Route of a pass of this model, as it is configured now, on that 1/8 map or image (resolve_route: refuses what does not go
        together); the update block runs on it from here on."""
        route = resolve_route(self.mixed_precision, self.alternate_corr, self.alt_corr_fp16, self.pad_maps, self.pad_encoders, self.update_fp16,
                              map_size, image_size)
        ub = self.update_block
        if ub.route[:6] != route[:6]:                          # (rarely: assigning a module attribute costs as much as resolving)
            ub.route = route.options
        return route

    def _padded(self, h8, w8):
        return self._route(map_size=(h8, w8)).loop_pad

    def _check_update_fp16(self, w8):
        self._route(map_size=(w8, w8))                         # (the refusals read the width only)

    def _pyramid(self, route, b, h8, w8, device):
        p = self._pyr
        if route.alternate_corr:
            c = self.fnet.conv2.out_channels
            if not isinstance(p, ops.AltCorr) or (p.b, p.c, p.h8, p.w8, p.fp16) != (b, c, h8, w8, route.alt_corr_fp16) or p.buf.device != device:
                self._pyr = p = ops.AltCorr(b, c, h8, w8, self.corr_levels, self.corr_radius, device=device, fp16=route.alt_corr_fp16)
            return p
        x3 = CORR_BF16X3 or CONV_BF16X3
        if p is None or (p.b, p.h8, p.w8) != (b, h8, w8) or p.buf.device != device or getattr(p, 'x3', False) != x3:
            self._pyr = ops.CorrPyramid(b, h8, w8, self.corr_levels, self.corr_radius, device=device, bf16x3=x3)
            self._pyr.x3 = x3
        return self._pyr

    def _workspace(self, n, h8, w8, device, padded=None):
        """Activation buffers that live INSIDE a forward pass -- (h | motion | flow), (r*h | motion | flow), z, the motion
        encoder's concat buffer, the lookup output and the four context terms -- allocated once per (batch, map, device):
        the prepared launch descriptors of the GRU loop are keyed on these addresses, so they are built once and hit on
        every later pass (and nothing from a previous pass stays pinned besides this one set).  Single-stream use, like
        the rest of the module; tensors handed back to the caller (flows, hidden, context) are always fresh.
        ``padded`` = (hp, wp) (pad_maps): every buffer is a ZERO-FILLED (hp, wp) map of which (h8, w8) is content (``valid``), plus padded
        copies of the context features and of a warm start's flow_init.  Invariant: whatever a tuned kernel reads as a convolution input is
        exactly zero outside the content at every launch -- the lookup and the copies in write the content only, every convolution of the
        loop stores zero outside it (the valid-extent entry points)."""
        key = (n, h8, w8, str(device), padded)
        if self._ws is None:
            self._ws = {}
        if key not in self._ws:
            if len(self._ws) >= 2:                             # a tracker alternates between two shapes at most (batch n / 2n)
                self._ws.pop(next(iter(self._ws)))
            c = self.hidden_dim
            mh, mw = (h8, w8) if padded is None else padded
            e = lambda ch: (torch.empty if padded is None else torch.zeros)(n, ch, mh, mw, device=device)
            self._ws[key] = dict(hx=e(2 * c), rhx=e(2 * c), z=e(c), cat=e(2 * c),
                                 corr=e(self.corr_levels * (2 * self.corr_radius + 1) ** 2),
                                 ctx=dict(zr1=e(2 * c), q1=e(c), zr2=e(2 * c), q2=e(c)),
                                 coords0=coords_grid(n, mh, mw, device), coords1=e(2), flow=e(2),
                                 zero2=torch.zeros(n, 2, mh, mw, device=device), valid=None if padded is None else (h8, w8))
            if padded is not None:
                self._ws[key].update(inp=e(c), finit=e(2))
        return self._ws[key]

    def _loop_program(self, pyr, ws, iters, side):
        """The update loop on workspace ``ws`` as a launch list (ops.OpList): per iteration [fork: convf1 -> convf2 on the side stream]
        lookup, convc1, convc2, [join | convf1, convf2], conv, the four GRU convolutions, FlowHead.conv1 and the flow update -- built once
        per (weights, pyramid, workspace, iters, streams) and replayed by one rpe_run_ops call per pass.  Cells 0 / 1: the fork / join
        events; cells 2 + 2k, 3 + 2k: timing events around iteration k's lookup (LOOKUP_EVENT_SINK; empty = skipped).
        Returns (list, marks) with marks[k] = first op of iteration k, marks[iters] = the end."""
        launchers_key, L = self.update_block.launchers(ws, pyr, with_key=True)
        key = (launchers_key, iters, None if side is None else side[0].cuda_stream)
        return _cached(ws, '_program', key, lambda: self._make_loop_program(L, iters, side))

    def _make_loop_program(self, L, iters, side):
        lk, c1 = (L.lookup, L.c1) if L.lookup_c1 is None else (L.lookup_c1, None)
        prog = ops.OpList(n_cells=2 + 2 * iters)
        if side is not None:
            for cell, ev in ((0, side[1]), (1, side[2])):
                ev.record()                                       # (torch creates the hipEvent_t at the first record)
                prog.cells[cell] = ev.cuda_event
        marks = []
        for itr in range(iters):
            marks.append(prog.mark())
            if side is not None:                                  # the flow branch needs only the flow: beside lookup -> convc1 -> convc2
                prog.record(0, 0).wait(0, 1).add(L.f1, 1).add(L.f2, 1).record(1, 1)
            prog.record(2 + 2 * itr, 0).add(lk).record(3 + 2 * itr, 0)
            if c1 is not None:
                prog.add(c1)
            prog.add(L.c2)
            if side is not None:
                prog.wait(1, 0)
            else:
                prog.add(L.f1).add(L.f2)
            prog.add(L.cv)
            for launch in L.gru:
                prog.add(launch)
        marks.append(prog.mark())
        prog.keep = side                                      # (the fork / join events of cells 0 / 1)
        prog.armed = False
        return prog, marks

    def _encode(self, net, images, route=None, **kw):
        """``net`` on raw 0..255 images under the pass's ``route``; a call from outside a pass resolves its own first, and is refused like a pass."""
        if route is None:
            first = images[0] if isinstance(images, (list, tuple)) else images
            route = self._route(image_size=None if first is None else first.shape[-2:])
        return net(images, raw255=True, route=route, **kw)

    @torch.no_grad()
    def encode_features(self, images):
        """fnet on raw 0..255 images (normalised like forward does); one batch or a list of batches encoded as one."""
        return self._encode(self.fnet, images).float()

    @torch.no_grad()
    def encode_context(self, images):
        """cnet on raw 0..255 images (one batch or a list of batches): (N,256,H/8,W/8) = (tanh(net) | relu(inp)), the initial
        hidden state and the context features of core/RAFT/core/raft.py, activated in the output layer's epilogue."""
        return self._encode(self.cnet, images, split_act=True)

    @torch.no_grad()
    def encode_both(self, feature_images, context_images):
        """(encode_features(feature_images), encode_context(context_images)).  The two encoders share nothing but their input images,
        so on a GPU the context encoder runs on the side stream beside the feature encoder (ENC_STREAMS): two independent chains of
        launches fill each other's tails and latencies -- at bench geometry 23.3 -> 23.0 ms for the pair (step 67.65 -> 67.24 ms); not for
        the one to three images of sequential tracking, where the fork / join costs what it hides (138 vs 136 frames/s with it).
        Same kernels on the same inputs: identical results."""
        many = isinstance(context_images, (list, tuple))
        first = context_images[0] if many else context_images
        count = sum(t.shape[0] for t in context_images) if many else first.shape[0]
        if not (ENC_STREAMS and first.is_cuda and count >= ENC_STREAMS_MIN):
            return self.encode_features(feature_images), self.encode_context(context_images)
        stream, ev_in, ev_done = self._side_stream(first.device)
        cur = torch.cuda.current_stream(first.device)
        ev_in.record(cur)
        with torch.cuda.stream(stream):
            stream.wait_event(ev_in)                          # the images (and the weights) are ready on the caller's stream
            cn = self.encode_context(context_images)
            ev_done.record(stream)
        f = self.encode_features(feature_images)
        cur.wait_event(ev_done)
        cn.record_stream(cur)                                 # allocated on the side stream, consumed (and freed) on the caller's
        return f, cn

    def _begin(self, route, pyr, ws, fmap1, fmap2, cnet, fused, flow_init=None):
        """Everything of a pass in front of the update loop: the correlation pyramid, h <- tanh half of the context encoder's output, the
        GRU's four loop-invariant context terms, and (fused route) coords1 <- grid, flow <- 0 in the workspace's persistent buffers,
        which the flow head's output layer then updates in place.  ``flow_init`` (warm start): coords1 <- grid + flow_init and flow_init
        as the flow the first iteration's motion encoder sees, in ONE launch (rpe_flow_seed) instead of the four plane copies."""
        c = self.hidden_dim
        if route.alternate_corr:
            pyr.build(fmap1.float(), fmap2.float())
        else:
            pyr.build(fmap1.float(), fmap2.float(), fp16_features=route.mixed_precision, bf16x3=(CORR_BF16X3 or CONV_BF16X3) and not route.mixed_precision)
        hx, rhx = ws['hx'], ws['rhx']
        if ws['valid'] is not None:
            # pad_maps: net, inp and flow_init go into the zero-padded maps by one strided copy each; the context terms are computed on the
            # padded inp (their padding holds the bias, which only the gate epilogues add -- and those store zero there)
            h8, w8 = ws['valid']
            ops.copy_rect(cnet[:, :c], hx[:, :c], h8, w8)
            ops.copy_rect(cnet[:, c:], ws['inp'], h8, w8)
            ctx = self.update_block.context_terms(ws['inp'], out=ws['ctx'])
            if flow_init is not None:
                flow_init = ops.copy_rect(flow_init, ws['finit'], h8, w8)       # (coords1's padding becomes the grid, the flow's stays zero)
        else:
            ops.copy_planes(cnet[:, :c], hx[:, :c])
            ctx = self.update_block.context_terms(cnet[:, c:], out=ws['ctx'] if fused else None)      # (fused: written into the persistent buffers)
        if fused and flow_init is not None:
            ops.flow_seed(flow_init, coords_out=ws['coords1'], flow_out=ws['flow'], dst1=hx[:, 2 * c - 2:], dst2=rhx[:, 2 * c - 2:])
        elif fused:
            ops.copy_planes(ws['coords0'], ws['coords1'])
            ops.copy_planes(ws['zero2'], ws['flow'])
            ops.copy_planes(ws['zero2'], hx[:, 2 * c - 2:])
            ops.copy_planes(ws['zero2'], rhx[:, 2 * c - 2:])
        return ctx

    def _prediction(self, flow, hx, upsample, valid=None):
        """What forward() returns for the 1/8 ``flow``: mask head on the hidden state + convex x8 up-sampling, or a copy of the flow.
        ``valid`` (pad_maps: the workspace's): the heads read the padded maps and write the true-size flow."""
        if upsample:
            return ops.upsample_convex(flow, self.update_block.up_mask(hx[:, :self.hidden_dim]), size=valid)
        if valid is not None:
            return ops.copy_rect(flow, torch.empty(flow.shape[0], 2, *valid, device=flow.device), *valid)
        return ops.copy_planes(flow, torch.empty_like(flow))

    def _finish(self, ws, upsample, ret_lowres=False):
        """Behind the loop of the fused route: the returned prediction (mask head + convex x8 up-sampling, or a copy of the 1/8 flow), the
        returned hidden state and (``ret_lowres``) a copy of the last 1/8 flow, all fresh tensors (the last one None when not asked for)."""
        c = self.hidden_dim
        hx, flow, valid = ws['hx'], ws['flow'], ws['valid']
        pred = self._prediction(flow, hx, upsample, valid)
        if valid is not None:                                     # pad_maps: hidden state and 1/8 flow come out cropped and contiguous
            fresh = lambda ch: torch.empty(hx.shape[0], ch, *valid, device=hx.device)
            return pred, ops.copy_rect(hx[:, :c], fresh(c), *valid), ops.copy_rect(flow, fresh(2), *valid) if ret_lowres else None
        h_buf = ops.copy_planes(hx[:, :c], torch.empty(hx.shape[0], c, hx.shape[2], hx.shape[3], device=hx.device))
        low = ops.copy_planes(flow, torch.empty_like(flow)) if ret_lowres else None
        return pred, h_buf, low

    def _run_loop(self, pyr, ws, iters, side):
        prog, marks = self._loop_program(pyr, ws, iters, side)
        if LOOKUP_EVENT_SINK is not None:
            for i, h in enumerate(LOOKUP_EVENT_SINK(iters)):
                prog.cells[2 + i] = h
            prog.armed = True
        elif prog.armed:
            for i in range(2 * iters):
                prog.cells[2 + i] = None
            prog.armed = False
        streams = (ops.raw_stream(),) if side is None else (ops.raw_stream(), side[0].cuda_stream)
        return prog, marks, streams

    def _forward_recorded(self, route, fmap1, fmap2, cnet, iters, upsample, flow_init=None, ret_lowres=False):
        """forward() for a small pass on given encoder outputs (sequential tracking: one or two flow pairs per frame) as THREE calls into
        the library: the recorded front (_begin; a warm pass's seeding launch included, flow_init bound like the encoder outputs), the
        loop's launch list, the recorded tail (_finish), whose result it returns.  None = this pass cannot be recorded (the caller goes on call by call)."""
        N, _, h8, w8 = fmap1.shape
        dev = fmap1.device
        c = self.hidden_dim
        ts = (fmap1, fmap2, cnet) + (() if flow_init is None else (flow_init,))
        if not all(ops._is_f32(t) and t.device == dev for t in ts) or _overlap(ts) \
                or tuple(cnet.shape) != (N, 2 * c, h8, w8) or dev.index != torch.cuda.current_device() \
                or (flow_init is not None and tuple(flow_init.shape) != (N, 2, h8, w8)):
            return None                                               # (the call-by-call route raises what needs raising)
        recorded, wkey = _recording(self, self.update_block)
        pyr = self._pyramid(route, N, h8, w8, dev)
        ws = self._workspace(N, h8, w8, dev, route.loop_pad)
        key = (N, h8, w8, dev.index, ops.raw_stream(), iters, upsample, flow_init is not None, ret_lowres, route.options, _switches(),
               pyr.buf.data_ptr(), ws['hx'].data_ptr(), wkey)
        ins = {'f1': fmap1, 'f2': fmap2, 'cnet': cnet}
        if flow_init is not None:
            ins['finit'] = flow_init
        side = self._side_stream(dev) if SIDE_STREAM and N * h8 * w8 <= SIDE_STREAM_MAX else None
        entry = recorded.get(key)
        if entry is not None:
            pre, post = entry.pre, entry
            pre.replay(ins)
            prog, _, streams = self._run_loop(pyr, ws, iters, side)
            prog.run(streams)
            pred, h_buf = torch.empty(post.pred_shape, device=dev), torch.empty(N, c, h8, w8, device=dev)
            low = torch.empty(N, 2, h8, w8, device=dev) if ret_lowres else None
            post.replay({'pred': pred, 'h': h_buf, **({'low': low} if ret_lowres else {})})
            return pred, h_buf, low
        if not recorded.wanted(key):
            return None
        prog, _, streams = self._run_loop(pyr, ws, iters, side)      # (built outside the recordings: its launchers must hold the real entry points)
        pre = ops.Recorder()
        with pre:
            self._begin(route, pyr, ws, fmap1, fmap2, cnet, True, flow_init)
        prog.run(streams)
        post = ops.Recorder()
        with post:
            pred, h_buf, low = self._finish(ws, upsample, ret_lowres)
        if pre.complete and post.complete:
            outs = {'pred': pred, 'h': h_buf, **({'low': low} if ret_lowres else {})}
            ok = all(pre.bind(k, t) > 0 for k, t in ins.items()) and all(post.bind(k, t) > 0 for k, t in outs.items())
            pre.complete = post.complete = ok
        post.complete = post.complete and pre.complete
        post.pre, post.pred_shape = pre, tuple(pred.shape)
        recorded.put(key, post)
        return pred, h_buf, low

    def head_params(self):
        """The eight parameters of the output heads in raft_grad.raft_tail_backward's order: (flow head, mask head)."""
        fh, mk = self.update_block.flow_head, self.update_block.mask
        return (fh.conv1.weight, fh.conv1.bias, fh.conv2.weight, fh.conv2.bias), (mk[0].weight, mk[0].bias, mk[2].weight, mk[2].bias)

    def update_params(self):
        """The 22 parameters of the SepConvGRU and the motion encoder in raft_grad.UPDATE_PARAMS' order (raft_grad.update_step_backward)."""
        return tuple(operator.attrgetter(name)(self.update_block) for name in raft_grad.UPDATE_PARAMS)

    def backward_encoders(self, image1, image2, fmap1, fmap2, net0, inp):
        """The encoders' backward behind a ``forward(image1, image2, ..., grad_corr=True)`` pass whose loss has been differentiated: the
        four leaves that pass returned carry d loss / d (fmap1, fmap2, net_0, inp) in their .grad; raft_grad.encoder_backward takes it
        through fnet (both images, one batch) and through cnet (image1, behind the tanh | ReLU of its output) and the results are ADDED
        into the .grad of the encoders' parameters, fnet's first, each in raft_grad.encoder_params' order.  With the node's own
        gradients (heads, update block) that is RAFT's whole gradient, in two calls.  Nothing else of the model is touched."""
        leaves = (fmap1, fmap2, net0, inp)
        if any(t.grad is None for t in leaves):
            raise RpeError('RAFT.backward_encoders: fmap1, fmap2, net0 and inp must be the leaves of a grad_corr pass after loss.backward() (a .grad is None)')
        route = self._route(image_size=tuple(image1.shape[-2:]))
        jobs = ((self.fnet, [image1, image2], torch.cat((fmap1.grad, fmap2.grad), dim=0), False),
                (self.cnet, image1, torch.cat((net0.grad, inp.grad), dim=1), True))
        for enc, images, d_out, split in jobs:
            grads = raft_grad.encoder_backward(enc, images, d_out, raw255=True, split_act=split, route=route)
            for p, g in zip(raft_grad.encoder_params(enc), grads):
                p.grad = g if p.grad is None else p.grad + g

    def _save_state(self, ws, states, flow=None, coords1=None):
        """``grad_update``: the entry state of the iteration about to run as dense tensors of their own -- (hx's 256 channels: h_{k-1} |
        motion slot | flow_k, and coords1_k, which the lookup is about to read), the content only when the workspace is padded: one copy
        of hx and one of the two coordinate planes.  ``flow`` / ``coords1``: the generic route's, which keeps them outside the workspace
        (and writes flow_k into hx inside the step)."""
        hx, valid = ws['hx'], ws['valid']
        co = ws['coords1'] if coords1 is None else coords1.contiguous()
        if valid is not None:
            new = lambda ch: torch.empty(hx.shape[0], ch, *valid, device=hx.device)
            states.append((ops.copy_rect(hx, new(hx.shape[1]), *valid), ops.copy_rect(co, new(2), *valid)))
            return
        st = ops.copy_planes(hx, torch.empty_like(hx))
        if flow is not None:
            ops.copy_planes(flow.contiguous(), st[:, hx.shape[1] - 2:])
        states.append((st, ops.copy_planes(co, torch.empty_like(co))))

    @torch.no_grad()
    def grad_pass(self, fmaps, cnet, *, stages, sources=None, grad_all_flows=False, **kw):
        """One gradient-free ``ret_lowres`` pass on given encoder outputs (``kw``: upsample, iters, all_flows, flow_init), run so that
        raft_grad can differentiate it as far as ``stages`` -- 'heads', 'update', 'corr' or 'encoders' (raft_grad's module docstring) ->
        (forward's result with the 1/8 flow as its 4th element, the raft_grad.GradPass of the whole batch; GradPass.rows makes its
        leaves).  ``sources`` (with 'encoders', and only then): where fmaps[0], fmaps[1] and cnet came from, an (images, lo, hi) each --
        one raw 0..255 image batch, or a tuple of batches that were encoded as one, and the rows of it.  The refusals are raised before
        any launch.  Below 'heads' the pass runs iteration by iteration and saves every iteration's entry state, and its pyramid is the
        record's from here on, no longer the model's.  ``grad_all_flows`` (needs all_flows=True): the record also carries the N - 1 earlier
        up-sampled predictions, which the node then differentiates too (raft_grad's module docstring); at 'heads' such a pass runs
        iteration by iteration as well and keeps every earlier iteration's (net_k, 1/8 flow_k), 130 h8 w8 4 bytes per pair each."""
        self.check_grad(stages, kw.get('upsample', True))
        if grad_all_flows:
            self.check_grad_all_flows(kw.get('all_flows', False), stages, kw.get('upsample', True))
        if (sources is None) != (stages != 'encoders'):
            raise RpeError("RAFT.grad_pass: sources goes with stages='encoders', and only with it")
        if sources is not None:
            for (_, lo, hi), t in zip(sources, (*fmaps, cnet)):
                if hi - lo != t.shape[0]:
                    raise RpeError(f'RAFT.grad_pass: a source names {hi - lo} images for {t.shape[0]} rows of encoder output')
        states = None if stages == 'heads' and not grad_all_flows else []
        r = self._forward_impl(self._route(map_size=tuple(fmaps[0].shape[-2:])), fmaps, cnet, ret_lowres=True, states=states, **kw)
        rec = raft_grad.GradPass(r[0][-1], r[1], r[3])
        c = self.hidden_dim
        if grad_all_flows:
            rec.earlier = list(r[0][:-1])
            if stages == 'heads':                              # (the states' h_k and flow_k alone: the 258-channel copies are dropped)
                fresh = lambda t: ops.copy_planes(t, torch.empty(t.shape, dtype=torch.float32, device=t.device))
                rec.tail_states = [(fresh(st[:, :c]), fresh(st[:, st.shape[1] - 2:])) for st, _ in states[1:]]
        if stages != 'heads':
            rec.net0, rec.inp, rec.states = cnet[:, :c], cnet[:, c:], states
            rec.pyr, self._pyr = self._pyr, None
        if stages in ('corr', 'encoders'):
            rec.fmap1, rec.fmap2 = fmaps                      # (what the pass correlated)
        if sources is not None:
            rec.sources = tuple((images, lo, hi) for images, lo, hi in sources)
        return r, rec

    def check_grad(self, stages, upsample=True):
        """Every refusal of a gradient pass as deep as ``stages``, before anything is launched."""
        if stages not in raft_grad.STAGES:
            raise ValueError(f'RAFT: stages must be one of {raft_grad.STAGES}, got {stages!r}')
        self.check_grad_heads(upsample)
        if stages in ('corr', 'encoders'):
            self.check_grad_corr()
        if stages == 'encoders':                               # (what raft_grad.encoder_backward refuses without a tensor in hand)
            for enc in (self.fnet, self.cnet):
                raft_grad._check_modes('RAFT: grad_encoders', enc)

    @staticmethod
    def check_grad_all_flows(all_flows, stages, upsample=True):
        """The refusals of ``grad_all_flows`` (raised before anything is launched): it differentiates the predictions all_flows returns,
        through a node of some depth, and those are the up-sampled ones."""
        if not all_flows:
            raise RpeError('RAFT: grad_all_flows differentiates every returned prediction: it needs all_flows=True')
        if stages is None:
            raise RpeError('RAFT: grad_all_flows needs a gradient stage: one of grad_heads, grad_update, grad_corr, grad_encoders')
        if not upsample:
            raise RpeError('RAFT: grad_all_flows attaches to the up-sampled predictions: it needs upsample=True')

    def check_grad_heads(self, upsample=True):
        """The refusals of ``grad_heads`` (raised before anything is launched): the tail's backward differentiates the f32 layers; a route
        that rounds their operands has no honest gradient here."""
        route = self._route()
        if route.update_fp16:
            raise RpeError('RAFT: grad_heads differentiates the f32 output heads -- not with update_fp16 (fp16 operands in the flow and mask heads)')
        if CONV_BF16X3:
            raise RpeError('RAFT: grad_heads differentiates the f32 output heads -- not with CONV_BF16X3 (bf16x3 products in the flow and mask heads)')
        if route.mixed_precision:
            raise RpeError('RAFT: grad_heads is f32 only -- not with mixed_precision')
        if not upsample:
            raise RpeError('RAFT: grad_heads attaches to the up-sampled prediction: it needs upsample=True')

    def check_grad_corr(self):
        """The refusals of ``grad_corr`` beyond check_grad_heads' (raised before anything is launched): the correlation's backward
        differentiates the f32 pyramid; ``alternate_corr`` has no pyramid, and CORR_BF16X3 does not form f32 products."""
        route = self._route()
        if route.alternate_corr:
            raise RpeError('RAFT: grad_corr differentiates the correlation pyramid -- not with alternate_corr (no pyramid is built)')
        if CORR_BF16X3:
            raise RpeError('RAFT: grad_corr is f32 only -- not with CORR_BF16X3')

    @torch.no_grad()
    def forward(self, image1, image2, upsample=True, iters=None, all_flows=False, fmaps=None, cnet=None, flow_init=None, ret_lowres=False,
                grad_heads=False, grad_update=False, grad_corr=False, grad_encoders=False, grad_all_flows=False):
        """image1, image2: (N,3,H,W) in 0..255.  Inference only (the reference freezes RAFT, train.yaml:51).
        ``fmaps`` / ``cnet`` accept encoder outputs computed elsewhere (both encoders normalise per sample -- instance
        norm / frozen batch norm -- so a caller may encode every distinct image once and reuse it); with both given the
        images may be None.  ``cnet`` is encode_context's output: (tanh(net) | relu(inp)).
        ``flow_init`` (N,2,H/8,W/8) f32: warm start as upstream RAFT's (coords1 = coords0 + flow_init; the first iteration's motion encoder
        sees flow = flow_init), e.g. ops.forward_interpolate of the previous frame's 1/8 flow; all zeros gives the cold pass bit for bit.
        ``ret_lowres``: a 4th return element, the last iteration's 1/8 flow as a fresh tensor.
        ``grad_heads`` / ``grad_update`` / ``grad_corr`` (each implies the one before): the pass runs as ever, gradient-free, as grad_pass
        runs it, and the returned LAST prediction is the output of one autograd node (raft_grad.attach) whose backward goes as far as
        the output heads / the whole update block through time / the correlation.  raft_grad's module docstring says what each stage
        saves, costs, differentiates and refuses.  ``hidden`` comes back as a leaf that requires grad (.grad = d loss / d net_N); behind
        the result grad_update appends the leaves ``net_0`` (N,128,h8,w8) and ``inp`` (a leaf copy of the context), grad_corr also
        ``fmap1`` and ``fmap2`` (leaf copies of the maps the pass correlated).
        ``grad_encoders`` (implies grad_corr): the node goes on through both encoders (raft_grad's depth 'encoders'), so after
        ``loss.backward()`` EVERY parameter of the model that requires grad has its gradient; no second call (backward_encoders) is
        needed.  It needs the images: with ``fmaps`` or ``cnet`` given it is refused before any launch -- an encoder output computed
        elsewhere cannot be differentiated here -- as are a batch norm in training mode and an active dropout.  It returns what a
        grad_corr call returns, with the same values, except that ``hidden`` and the context are the node's ``hidden_out`` and
        ``context_out``: whatever a consumer differentiates of them returns into the chain (the four leaves behind still get their .grad).
        ``grad_all_flows`` (with ``all_flows=True`` and one of the four stages): EVERY element of the returned ``flows`` is an output of
        the one node, so a loss over all N predictions -- RAFT's sequence loss, ops.flow_sequence_loss -- trains the model as far as the
        stage goes; values, launches of the forward and the other return elements are those of the call without it.  Refused before any
        launch without all_flows, without a stage, or with upsample=False."""
        stages = 'encoders' if grad_encoders else 'corr' if grad_corr else 'update' if grad_update else 'heads' if grad_heads else None
        if grad_all_flows:
            self.check_grad_all_flows(all_flows, stages, upsample)
        if stages is not None:
            self.check_grad(stages, upsample)                  # (before the encoders run: a refused pass launches nothing)
        sources = None
        if grad_encoders:
            if fmaps is not None or cnet is not None or image1 is None or image2 is None:
                raise RpeError('RAFT: grad_encoders differentiates the encoders on the images -- not with fmaps= or cnet= (an encoder output '
                               'computed elsewhere cannot be differentiated here)')
            N = image1.shape[0]
            sources = ((image1, 0, N), (image2, 0, N), (image1, 0, N))
        fmaps, cnet, route = self._encoded(image1, image2, fmaps, cnet)
        if stages is None:
            return self._forward_impl(route, fmaps, cnet, upsample, iters, all_flows, flow_init, ret_lowres)
        (flows, _, context, low), rec = self.grad_pass(fmaps, cnet, stages=stages, sources=sources, upsample=upsample, iters=iters, all_flows=all_flows,
                                                       flow_init=flow_init, grad_all_flows=grad_all_flows)
        rec = rec.rows(0, rec.hidden.shape[0])
        hidden = rec.hidden
        outs, earlier = raft_grad.attach([rec], self.head_params(), None if stages == 'heads' else self.update_params(),
                                         (self.fnet, self.cnet) if grad_encoders else None, ret_earlier=True)
        if grad_encoders:
            flows[-1], hidden, context = outs[0]
        else:
            flows[-1] = outs[0]
        flows[:-1] = earlier[0] if grad_all_flows else flows[:-1]
        leaves = tuple(t for t in (rec.net0, rec.inp, rec.fmap1, rec.fmap2) if t is not None)
        return (flows, hidden, context) + ((low,) if ret_lowres else ()) + leaves

    def _encoded(self, image1, image2, fmaps, cnet):
        """What forward's caller did not bring of the encoder outputs -> ((fmap1, fmap2), cnet, the pass's Route)."""
        if image1 is None:                                    # encoder outputs given: the images are not needed again
            route = self._route(map_size=tuple(fmaps[0].shape[-2:]))
        else:
            route = self._route(image_size=tuple(image1.shape[-2:]))       # (before the encoders run: a refused pass launches nothing)
        if fmaps is None:
            N = image1.shape[0]
            f = self._encode(self.fnet, (image1, image2), route).float()
            fmaps = f[:N], f[N:]                              # (else precomputed by encode_features: the caller de-duplicates)
        if cnet is None:
            cnet = self._encode(self.cnet, image1, route, split_act=True)       # (tanh(net) | relu(inp))
        return fmaps, cnet, route

    def _forward_impl(self, route, fmaps, cnet, upsample=True, iters=None, all_flows=False, flow_init=None, ret_lowres=False, states=None):
        """forward on the encoder outputs under ``route``.  ``states`` (grad_pass): a list that receives every iteration's entry state
        (_save_state); the copies sit between the iterations, so such a pass is neither recorded nor run as one launch list."""
        iters = self.iters if iters is None else iters
        fmap1, fmap2 = fmaps
        (N, _, h8, w8), dev = fmap1.shape, fmap1.device
        c = self.hidden_dim
        if flow_init is not None:
            if tuple(flow_init.shape) != (N, 2, h8, w8) or flow_init.dtype != torch.float32 or flow_init.device != dev:
                raise ValueError(f'RAFT.forward: flow_init must be a float32 ({N},2,{h8},{w8}) tensor on {dev}, got '
                                 f'{flow_init.dtype} {tuple(flow_init.shape)} on {flow_init.device}')
            flow_init = flow_init.contiguous()
        tail = lambda flows, hidden, low: (flows, hidden, cnet[:, c:]) + ((low,) if ret_lowres else ())      # (what forward returns)
        ub = self.update_block
        padded = route.loop_pad                                # pad_maps: the loop's maps, when the tuned kernels refuse (h8, w8)
        P = ub.packed_convs((padded or (h8, w8))[1])
        fused = P is not None
        if fused and FRAME_OPLISTS and LOOP_OPLIST and not all_flows and N <= FRAME_OPLISTS_MAX_IMAGES and LOOKUP_EVENT_SINK is None \
                and states is None:                           # (grad_update: the state copies sit between the iterations)
            r = self._forward_recorded(route, fmap1, fmap2, cnet, iters, upsample, flow_init, ret_lowres)
            if r is not None:
                return tail([r[0]], r[1], r[2])
        pyr = self._pyramid(route, N, h8, w8, dev)
        ws = self._workspace(N, h8, w8, dev, padded)
        ctx = self._begin(route, pyr, ws, fmap1, fmap2, cnet, fused, flow_init)
        hx, corr = ws['hx'], ws['corr']                     # hx = (h | motion | flow)
        flow_predictions = []
        side = self._side_stream(dev) if fused and SIDE_STREAM and N * h8 * w8 <= SIDE_STREAM_MAX else None
        if fused and LOOP_OPLIST:                             # the loop as a launch list: whole, or iteration by iteration for their flows
            prog, marks, streams = self._run_loop(pyr, ws, iters, side)
            if not all_flows and states is None:
                prog.run(streams)
            for itr in range(iters if all_flows or states is not None else 0):
                if states is not None:
                    self._save_state(ws, states)
                prog.run(streams, marks[itr], marks[itr + 1])
                if all_flows and itr < iters - 1:
                    flow_predictions.append(self._prediction(ws['flow'], hx, upsample, ws['valid']))
        elif fused:                                           # the same launches, one by one from Python
            for itr in range(iters):
                done = None
                if states is not None:
                    self._save_state(ws, states)
                if side is not None:
                    # the motion encoder's flow branch (convf1 -> convf2) needs only the flow: it runs on a side stream beside
                    # lookup -> convc1 -> convc2 and fills the partly idle last rounds of those launches
                    stream, ev_flow, done = side
                    ev_flow.record()
                    with torch.cuda.stream(stream):
                        stream.wait_event(ev_flow)
                        ub.encoder.flow_branch(ws['flow'], P, ub.launchers(ws))
                        done.record()
                pyr.lookup(ws['coords1'], out=corr, **({} if padded is None else dict(map_size=padded)))
                ub.step(ws, ctx, ws['flow'], ws['coords1'], None, flow_branch_done=done)
                if all_flows and itr < iters - 1:
                    flow_predictions.append(self._prediction(ws['flow'], hx, upsample, ws['valid']))
        if fused:
            pred, h_buf, low = self._finish(ws, upsample, ret_lowres)
            return tail(flow_predictions + [pred], h_buf, low)
        # the generic route: coords and flow are tensors of the pass, the heads run on a contiguous copy of h
        coords0 = ws['coords0']
        coords1 = coords0.clone() if flow_init is None else ops.flow_seed(flow_init, coords_out=torch.empty_like(coords0))     # coords0 + flow_init
        h_buf = torch.empty(N, c, h8, w8, device=dev)         # returned to the caller: fresh
        for itr in range(iters):
            pyr.lookup(coords1, out=corr)
            flow = flow_init if itr == 0 and flow_init is not None else coords1 - coords0
            if states is not None:
                self._save_state(ws, states, flow, coords1)
            coords1 = ub.step(ws, ctx, flow, coords1, h_buf)
            if all_flows or itr == iters - 1:
                lowres = coords1 - coords0
                flow_predictions.append(self._prediction(lowres, hx, upsample) if upsample else lowres)
        ops.copy_planes(hx[:, :c], h_buf)
        return tail(flow_predictions, h_buf, coords1 - coords0 if ret_lowres else None)
