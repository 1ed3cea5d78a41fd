"""RAFT's backward for training on the pose loss, composed on the host from the one-kernel wrappers of ops.py: the two stage functions
(raft_tail_backward, update_step_backward), the weight packings they run on, the record of what a pass saves (GradPass) and the ONE
autograd node over such records (attach).  The forward stays what it is -- a gradient-free pass, the launches and the bits of a
``ret_lowres`` pass --; RAFT.grad_pass runs it and fills the record, RAFT.forward(grad_heads= / grad_update= / grad_corr= / grad_encoders=) and
PoseNet.stages attach the node.

Upstream detaches coords1 at the top of every iteration.  The returned prediction therefore depends on the output heads through their
LAST application only, the correlation window and the flow that feed an iteration are constants of that iteration, and the only path
through time is the hidden state: the chain below is the exact gradient, nothing truncated.  A record's depth is which of its groups of
fields are present; each stage includes the ones above it:
  'heads'   (flow_up, hidden, flow_low).  Backward = raft_tail_backward (csrc/raft_backward.hip): the flow head's and the mask head's
            eight parameters and hidden.grad = d loss / d net_N.  The pass may be a recorded one.
  'update'  + (net0, inp, states, pyr).  The pass runs iteration by iteration and copies the entry state of every iteration -- hx's 256
            channels: h_{k-1}, the stale motion slot and flow_k, and the two planes of coords1_k -- into dense tensors of their own: 258
            h8 w8 4 bytes per pair and iteration, 5.3 MB at 640 x 512, 63 MB per pair for 12 iterations.  The correlation window is not
            saved: GradPass.corr looks it up again at the saved coordinates in the pass's pyramid, which the record takes over from the
            model (the forward's bits).  Backward = the tail, then update_step_backward (csrc/update_backward.hip) for k = N .. 1: all 30
            update-block parameters, net0.grad = d loss / d net_0 and inp.grad = d loss / d inp summed over the iterations, last first.
  'corr'    + (fmap1, fmap2), copies of the maps the pass correlated.  Every step also forms d corr_k (convc1's adjoint) and accumulates it
            at the saved coords1_k into the pass's gradient volume G = d loss / d pyramid (ops.corr_lookup_backward; S h8 w8 4 bytes per
            pair, S = the cells of the four levels: 139 MB at 640 x 512, 2.2 GB at 1280 x 1024, alive during that pass's backward only);
            after step 1 the build's adjoint runs once (ops.corr_build_backward, csrc/corr_backward.hip): fmap.grad = d loss / d fmap, the
            window being linear in the pyramid and the pyramid bilinear in the maps; nothing goes into the coordinates.  Every launch
            and every gradient of 'update' keeps its bits.
  'encoders' + (sources): where the pass's three encoder inputs came from -- for fmap1, for fmap2 and for the context a (raw 0..255 image
            batch or tuple of batches read as one, lo, hi) each; not a tensor field.  The node takes the encoders' 94 parameters behind the
            other 30 (attach(..., encoders=(fnet, cnet))) and gives every pass two more outputs, ``hidden_out`` (the values of hidden) and
            ``context_out`` (those of inp): what a consumer differentiates -- PoseNet's weight heads read both -- returns into the chain.  A
            gradient on hidden_out is added to the tail's d net_N once, before step N; one on context_out is added to d inp once, behind the
            steps' sum; the leaves' .grad hold these full gradients.  A pass runs its tail if its flow has a gradient and its steps if its
            flow or its hidden_out has one.  After the last pass the distinct images are collected by source identity (the same batch
            object and row; content is never compared) in the order of first appearance -- passes in the given order, fmap1's source
            before fmap2's, rows ascending -- and each image's d fmap is the sum of the contributing leaves' gradients in that walk order,
            added in f64 and rounded once (ops.sum_groups; a single contribution passes through unchanged); likewise cat(d net0, d inp) per
            distinct context image.  encoder_backward then runs ONCE per encoder, on the images something contributed to, and not at all
            for an encoder none of whose parameters requires grad; the 94 gradients leave the node as the gradients of its inputs.
            Every launch and every gradient of 'corr' keeps its bits.  This is what the reference's freeze_flow(False) trains.
A gradient per iteration (``grad_all_flows``, any depth): a record may carry ``earlier``, the N - 1 earlier up-sampled predictions, and the
node then has them as further outputs, behind the ones above (flows, hidden_out, context_out; then pass by pass the earlier predictions).
Prediction k depends on the parameters through net_k only -- coords1 is detached --, so the gradient of a loss over all predictions
(RAFT's sequence loss, ops.flow_sequence_loss) is the same walk with one more tail per iteration, on (net_k, flow_low_k, g_k) in front of
the step that takes d net_k on: _through_time, the one walk at every depth, says the rest.  A prediction without a gradient costs no
tail; with a gradient on the last prediction alone launches and bits are those of a record without ``earlier``.
Gradients added in f64 and rounded once go through _sum_f64; _split_bwd_weight forms a stride-1 weight gradient on pieces of a small map.
Refused before any launch (RAFT.check_grad_heads): update_fp16, CONV_BF16X3, mixed_precision -- a route that rounds the heads' operands
has no honest gradient here -- and upsample=False; for 'corr' also alternate_corr (no pyramid) and CORR_BF16X3 (RAFT.check_grad_corr); for
'encoders' also a batch norm in training mode and an active dropout in an encoder (_check_modes).

The encoders' backward is a stage function of its own (encoder_params, residual_block_backward, encoder_backward;
csrc/encoder_backward.hip).  Beside the depth above, RAFT.backward_encoders still hands it the .grad of a 'corr' pass's leaves (fmap1,
fmap2, net0, inp) by hand and adds the results into the encoders' parameters."""
import dataclasses
from typing import Any, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, ops
from .ops import (CONV_LINEAR, PackedConv, _nchw, affine_act, bn_frozen_backward, bounded_put, conv3x3_to2_bwd_data, conv_bwd_weight,
                  conv_direct, conv_fused, conv_s2_bwd_data, conv_s2_bwd_weight, copy_planes, gru_gates_h_recompute, gru_gates_r_backward,
                  gru_gates_zq_backward, gru_gates_zr_recompute, instnorm_act, instnorm_backward, relu_backward, split_act_backward,
                  sum_groups, upsample_convex_backward, wkey)

TAIL_GROUP_3X3_FWD, TAIL_GROUP_3X3_BWD, TAIL_GROUP_1X1 = 16, 32, 64      # input channels per launch of the tail's forward-kernel convolutions
# update_step_backward's parameter (and gradient) order: weight, bias of each -- 12 tensors of ``gru``, 10 of ``encoder``
UPDATE_PARAMS = tuple(f'{m}.{t}' for m in ('gru.convz1', 'gru.convr1', 'gru.convq1', 'gru.convz2', 'gru.convr2', 'gru.convq2', 'encoder.convc1',
                                           'encoder.convc2', 'encoder.convf1', 'encoder.convf2', 'encoder.conv') for t in ('weight', 'bias'))
# input channels per launch of the step's forward-kernel convolutions (forward recomputation and data gradients alike): 144 terms of a 3x3
# layer, 160 of a 5-tap layer, 64 of the 1x1 -- the k-ordered f32 chain of a launch stays below the tail's 288, the groups are added in f64
UPDATE_GROUP_3X3, UPDATE_GROUP_5TAP, UPDATE_GROUP_1X1 = 16, 32, 64
# the encoders' backward: input channels per launch of a 3x3 layer's forward recomputation (144 terms), of its data gradient (288) and of
# the 1x1 output layer (64); a stride-2 layer's recomputation runs ops.conv_direct on groups of at most ENC_CHAIN terms
ENC_GROUP_3X3_FWD, ENC_GROUP_3X3_BWD, ENC_GROUP_1X1, ENC_CHAIN = 16, 32, 64, 288
ENC_WGRAD_CHAIN = 1024                                                   # pixels rpe_conv_bwd_weight keeps in one chunk (include/rpe.h: its chunk rule)
# _split_bwd_weight's policies (its keywords; none: one launch).  Under ``wgrad_bands`` (a gradient per iteration) an update step's layers
# and an encoder's stride-1 layers; with or without it an encoder's run small batches one image each
UPDATE_WGRAD_BAND, ENC_WGRAD_BAND, ENC_BAND_CAP = 64, 256, 4096
_UPDATE_BANDS = dict(band=UPDATE_WGRAD_BAND, cap=ENC_WGRAD_CHAIN)
_ENCODER, _ENCODER_BANDS = dict(per_image=True), dict(per_image=True, band=ENC_WGRAD_BAND, over=ENC_WGRAD_CHAIN, cap=ENC_BAND_CAP)


# ------------------------------------------------------------------------------------------------- weight packings
class _SplitConvs:
    """What a stage function packs from its parameters: the stacked / transposed weights its subclass makes at construction, and each
    channel group's slice and PackedConv made on first use (get / conv_split)."""

    def __init__(self):
        self._made = {}

    def get(self, name, make):
        if name not in self._made:
            self._made[name] = make()
        return self._made[name]

    def conv_split(self, name, x, weight, bias, relu, group, out=None, extra=0, fill=None):
        """act(conv(x; weight) + bias), stride 1, 'same', 3x3, 1x1, 1x5 or 5x1, on the forward's kernels -- rpe_conv_fused where the map is one it takes
        (rows of whole 16-byte quads), ops.conv_direct at every other size -- run on ``group`` input channels at a time and the groups' results
        added in f64 (sum_groups).  Those kernels add their products in one k-ordered f32 chain: over all 1152 / 4608 terms of the tail's
        layers its error is 3-5 times that of a blocked float32 sum, over a group's 144-288 terms it is not."""
        b, cin, hh, ww = x.shape
        cout, kh, kw = weight.shape[0], weight.shape[2], weight.shape[3]
        bounds = [(lo, min(cin, lo + group)) for lo in range(0, cin, group)]
        # ``extra``: that many more (b,cout,h,w) terms of the f64 sum behind the groups' results; ``fill(terms)`` writes them (the update
        # block's backward adds the gradients that reach the same tensor by other paths there, instead of in f32 afterwards)
        allp = torch.empty(len(bounds) + extra, b, cout, hh, ww, dtype=torch.float32, device=x.device)
        parts = allp[:len(bounds)]
        if extra:
            fill(allp[len(bounds):])
        fused = ww % 4 == 0 and x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0
        for gi, (lo, hi) in enumerate(bounds):
            wg = self.get((name, gi, 'w'), lambda: weight[:, lo:hi].contiguous())
            if fused:
                conv_fused(x[:, lo:hi], self.get((name, gi, 'packed'), lambda: PackedConv(wg, None)), CONV_LINEAR, parts[gi])
            else:
                conv_direct(x[:, lo:hi], wg, None, 1, (kh // 2, kw // 2), out=parts[gi])
        return sum_groups(parts if extra == 0 else allp, bias, relu, out)


class _TailPacked(_SplitConvs):
    """What raft_tail_backward packs from the eight head parameters (flow head, then mask head).  Forward: the two 3x3 layers that read
    ``net`` stacked along their OUTPUT channels (one launch computes t_f and t_m) and the mask head's 1x1 (x 0.25, as RAFT's forward folds
    it).  Data gradients: the TRANSPOSED, FLIPPED weights -- dX = conv(dY; W^T flipped) is a forward convolution --, the two 256 -> 128 3x3
    layers stacked along their INPUT channels (the launches compute the sum of both data gradients) and the 576 -> 256 1x1 layer (x 0.25).
    Every one of them runs through conv_split: the forward kernels on groups of input channels, the groups added in f64."""

    def __init__(self, params):
        super().__init__()
        self.fh, self.mk = [t.detach() for t in params[:4]], [t.detach() for t in params[4:]]
        self.w3, self.b3 = torch.cat((self.fh[0], self.mk[0]), dim=0).contiguous(), torch.cat((self.fh[1], self.mk[1]), dim=0).contiguous()
        self.w3t = torch.cat((self.fh[0].transpose(0, 1).flip(2, 3), self.mk[0].transpose(0, 1).flip(2, 3)), dim=1).contiguous()
        self.w1, self.b1 = (0.25 * self.mk[2]).contiguous(), (0.25 * self.mk[3]).contiguous()
        self.w1t = (0.25 * self.mk[2]).transpose(0, 1).contiguous()


class _UpdatePacked(_SplitConvs):
    """What update_step_backward packs from the 22 parameters.  Forward: convz | convr of a half stacked along their OUTPUT channels, as
    the forward stacks them (gate_weights), in upstream's input order [h | inp | motion | flow].  Data gradients: the TRANSPOSED, FLIPPED
    weights, zr stacked along its INPUT channels."""

    def __init__(self, params):
        super().__init__()
        p = [t.detach() for t in params]
        self.w = {name: (p[2 * i], p[2 * i + 1]) for i, name in enumerate(('z1', 'r1', 'q1', 'z2', 'r2', 'q2', 'c1', 'c2', 'f1', 'f2', 'cv'))}
        tr = lambda w: w.transpose(0, 1).flip(2, 3)
        for hf in ('1', '2'):
            wz, bz = self.w['z' + hf]
            wr, br = self.w['r' + hf]
            self.w['zr' + hf] = (torch.cat((wz, wr), 0).contiguous(), torch.cat((bz, br), 0).contiguous())
            self.w['zr' + hf + 't'] = torch.cat((tr(wz), tr(wr)), 1).contiguous()
            self.w['q' + hf + 't'] = tr(self.w['q' + hf][0]).contiguous()
        for name in ('c1', 'c2', 'f2', 'cv'):
            self.w[name + 't'] = tr(self.w[name][0]).contiguous()


_PACKED = {}               # packing class -> {wkey of its parameters: the packing made from them} (the two newest weight sets of each)


def _packed(cls, params):
    cache, key = _PACKED.setdefault(cls, {}), wkey(*params)
    if key not in cache:
        bounded_put(cache, key, cls(params))
    return cache[key]


# ------------------------------------------------------------------------------------------------- the stage functions
def raft_tail_backward(net, flow_low, grad_up, fh_params, mask_params):
    """Backward of the tail of RAFT's last update iteration (csrc/raft_backward.hip):
        t_f = relu(conv3x3(net; fh.conv1)); delta = conv3x3(t_f; fh.conv2); t_m = relu(conv3x3(net; mask.0)); m = .25 conv1x1(t_m; mask.2)
        flow_up = upsample_convex(flow_prev + delta, m)
    net (b,128,h8,w8): the returned hidden state; flow_low (b,2,h8,w8) = flow_prev + delta, the pass's last 1/8 flow (``ret_lowres``; d / d delta
    = d / d flow_low, so flow_prev is not needed); grad_up (b,2,8 h8,8 w8); fh_params = (conv1.weight, conv1.bias, conv2.weight, conv2.bias)
    of the flow head, mask_params = (mask.0.weight, mask.0.bias, mask.2.weight, mask.2.bias).
    -> (d_net, (the eight parameter gradients in that order)).  t_f, t_m and m are recomputed from ``net`` with the forward's kernels
    (nothing is kept by the forward pass), which also compute the data gradients; each runs on groups of input channels whose results
    are added in f64 (_SplitConvs.conv_split).  f32 throughout, bit-identical from run to run."""
    net, fl, gu = _nchw(net, 'raft_tail_backward: net'), _nchw(flow_low, 'raft_tail_backward: flow_low'), _nchw(grad_up, 'raft_tail_backward: grad_up')
    fh, mk = tuple(fh_params), tuple(mask_params)
    b, c, hh, ww = net.shape
    for t in fh + mk:
        _nchw(t.detach(), 'raft_tail_backward: a head parameter')
    hid = fh[0].shape[0]
    if len(fh) != 4 or len(mk) != 4 or tuple(fh[0].shape) != (hid, c, 3, 3) or tuple(fh[2].shape) != (2, hid, 3, 3) \
            or tuple(mk[0].shape) != (hid, c, 3, 3) or tuple(mk[2].shape) != (576, hid, 1, 1):
        raise _lib.RpeError('raft_tail_backward: expected the flow head\'s (h,c,3,3), (2,h,3,3) and the mask head\'s (h,c,3,3), (576,h,1,1) weights')
    if tuple(fl.shape) != (b, 2, hh, ww) or tuple(gu.shape) != (b, 2, 8 * hh, 8 * ww):
        raise _lib.RpeError('raft_tail_backward: flow_low must be (b,2,h8,w8) and grad_up (b,2,8 h8,8 w8) for net (b,c,h8,w8)')
    P = _packed(_TailPacked, fh + mk)
    with torch.no_grad():
        # the forward, again
        t = P.conv_split('w3', net, P.w3, P.b3, True, TAIL_GROUP_3X3_FWD)              # (t_f | t_m): both layers read net
        t_f, t_m = t[:, :hid], t[:, hid:]
        m = P.conv_split('w1', t_m, P.w1, P.b1, False, TAIL_GROUP_1X1)
        # the adjoints, last layer first
        d_flow, d_m = upsample_convex_backward(gu, fl, m)
        g = torch.empty(b, 2 * hid, hh, ww, dtype=torch.float32, device=net.device)       # (d t_f | d t_m) in front of their ReLUs
        dw_fh2, db_fh2 = conv_bwd_weight(t_f, d_flow, (3, 3))
        conv3x3_to2_bwd_data(d_flow, P.fh[2], act=t_f, out=g[:, :hid])
        dw_m2, db_m2 = conv_bwd_weight(t_m, d_m, (1, 1), scale=0.25)
        P.conv_split('w1t', d_m, P.w1t, None, False, TAIL_GROUP_1X1, out=g[:, hid:])
        relu_backward(g[:, hid:], t_m)
        dw1, db1 = conv_bwd_weight(net, g, (3, 3))                      # both 3x3 layers read net: one GEMM of 2 * hid output channels
        d_net = P.conv_split('w3t', g, P.w3t, None, False, TAIL_GROUP_3X3_BWD)
    return d_net, (dw1[:hid], db1[:hid], dw_fh2, db_fh2, dw1[hid:], db1[hid:], dw_m2, db_m2)


def _sum_f64(terms):
    """The sum of a list of equally shaped gradients, added in list order in f64 and rounded once (sum_groups); of a list of tuples of
    gradients, the list of the sums position by position.  A single term passes through unchanged, and so does an absent (None) gradient.
    The view sum_groups gets: n terms of shape (c, ...) as (n, 1, c, rest, 1) -- a weight's output channels, a bias's elements."""
    if isinstance(terms[0], (tuple, list)):
        return [_sum_f64(ts) for ts in zip(*terms)]
    if len(terms) == 1 or terms[0] is None:
        return terms[0]
    return sum_groups(torch.stack(terms).view(len(terms), 1, terms[0].shape[0], -1, 1)).view_as(terms[0])


def _split_bwd_weight(x, dy, kernel, bias=True, band=0, over=0, cap=0, per_image=False):
    """ops.conv_bwd_weight on pieces of the map, their results added in f64 and rounded once (_sum_f64).  rpe_conv_bwd_weight splits
    K = b h w into chunks only above ENC_WGRAD_CHAIN pixels; below that an output element's products are ONE f32 chain over the map and
    across the images of the batch (at K = 512, two 16 x 16 maps, 2.6 times the error of a blocked float32 sum).  The pieces: with
    ``band``, on a map of over < b h w <= cap pixels, row bands of about ``band`` pixels -- dy zero outside the band, so the other
    pixels' products are exact zeros and add nothing to the chain; every band costs the whole map's GEMM, hence the cap --; else, with
    ``per_image``, one image each of a batch of several with at most ENC_WGRAD_CHAIN pixels in all; else the whole map, one launch."""
    b, _, hh, ww = dy.shape
    rows = max(1, band // (b * ww))
    if band and over < b * hh * ww <= cap and rows < hh:
        per = []
        for lo in range(0, hh, rows):
            part = torch.zeros(dy.shape, dtype=torch.float32, device=dy.device)
            part[:, :, lo:lo + rows] = dy[:, :, lo:lo + rows]
            per.append(conv_bwd_weight(x, part, kernel, bias=bias))
    elif per_image and b > 1 and b * hh * ww <= ENC_WGRAD_CHAIN:
        per = [conv_bwd_weight(x[i:i + 1], dy[i:i + 1], kernel, bias=bias) for i in range(b)]
    else:
        return conv_bwd_weight(x, dy, kernel, bias=bias)
    return tuple(_sum_f64(per))


def update_step_backward(hx, inp, corr, d_net, params, ret_d_corr=False, wgrad_bands=False):
    """Backward of ONE application of RAFT's update block without its heads (csrc/update_backward.hip):
        cor = relu(convc2(relu(convc1(corr)))); flo = relu(convf2(relu(convf1(flow)))); m = relu(conv([cor | flo])); x = [inp | m | flow]
        per half (1x5, then 5x1): z = s(convz([h | x])), r = s(convr([h | x])), q = tanh(convq([r h | x])), h <- (1 - z) h + z q
    hx (b,256,h8,w8): the step's entry state (h_{k-1} | motion slot | flow_k) in the workspace's layout -- the motion slot is not read;
    inp (b,128,h8,w8); corr (b,324,h8,w8): the looked-up window; d_net (b,128,h8,w8) = d loss / d net_k; params: the 22 tensors of
    UPDATE_PARAMS.  corr and flow are constants (upstream detaches coords1 at the top of the iteration): no gradient is formed into the flow,
    and none into corr unless asked for.
    -> (d_net_prev, d_inp, grads) with grads in UPDATE_PARAMS' order; with ``ret_d_corr`` additionally d_corr (b,324,h8,w8) = d loss / d corr,
    convc1's transposed 1x1 weight applied to the gradient in front of convc1's ReLU (conv_split, groups of UPDATE_GROUP_1X1 channels added
    in f64): what ops.corr_lookup_backward accumulates.  Without the flag the launches and the results are those of a call without it.  Every intermediate is recomputed here with the forward's kernels on
    groups of input channels added in f64 (conv_split), which also compute the data gradients; the gradients that reach a tensor by several
    paths are added in that same f64 sum.  ``wgrad_bands``: the eleven weight gradients under _split_bwd_weight's banded policy (small maps: row
    bands added in f64 instead of one f32 chain over the map); without it one launch each.  f32 throughout,
    bit-identical from run to run, a row's result independent of its batch."""
    who = 'update_step_backward'
    hx, inp, corr, d_net = _nchw(hx, f'{who}: hx'), _nchw(inp, f'{who}: inp'), _nchw(corr, f'{who}: corr'), _nchw(d_net, f'{who}: d_net')
    params = tuple(params)
    b, c2, hh, ww = hx.shape
    c = c2 // 2
    for t in params:
        _nchw(t.detach(), f'{who}: a parameter')
    want = [(c, 3 * c, 1, 5)] * 3 + [(c, 3 * c, 5, 1)] * 3 + [(256, corr.shape[1], 1, 1), (192, 256, 3, 3), (128, 2, 7, 7), (64, 128, 3, 3), (c - 2, 256, 3, 3)]
    if len(params) != 22 or c != 128 or any(tuple(params[2 * i].shape) != s or tuple(params[2 * i + 1].shape) != s[:1] for i, s in enumerate(want)):
        raise _lib.RpeError(f'{who}: expected the 22 tensors of UPDATE_PARAMS (SepConvGRU and BasicMotionEncoder of hidden size 128) and hx with 256 channels')
    if tuple(inp.shape) != (b, c, hh, ww) or tuple(d_net.shape) != (b, c, hh, ww) or tuple(corr.shape[::2]) != (b, hh) or corr.shape[3] != ww:
        raise _lib.RpeError(f'{who}: inp and d_net must be ({b},{c},{hh},{ww}) and corr (b,324,h8,w8) for hx {tuple(hx.shape)}')
    P = _packed(_UpdatePacked, params)
    wgrad = lambda x, dy, kernel: _split_bwd_weight(x, dy, kernel, **(_UPDATE_BANDS if wgrad_bands else {}))
    G3, G5, G1 = UPDATE_GROUP_3X3, UPDATE_GROUP_5TAP, UPDATE_GROUP_1X1
    new = lambda ch: torch.empty(b, ch, hh, ww, dtype=torch.float32, device=hx.device)
    with torch.no_grad():
        flow = hx[:, 2 * c - 2:]
        # the motion encoder, again
        c1 = P.conv_split('c1', corr, *P.w['c1'], True, G1)
        cat = new(256)                                                  # (cor | flo)
        P.conv_split('c2', c1, *P.w['c2'], True, G3, out=cat[:, :192])
        f1 = conv_direct(flow, *P.w['f1'], 1, 3, relu=True)              # 2 -> 128, 7x7: 98 terms
        P.conv_split('f2', f1, *P.w['f2'], True, G3, out=cat[:, 192:])
        # the GRU's two halves, again: A = [h | inp | m | flow] (upstream's order), R = [r h | inp | m | flow]
        A1, R1, A2, R2 = new(3 * c), new(3 * c), new(3 * c), new(3 * c)
        copy_planes(hx[:, :c], A1[:, :c])
        copy_planes(inp, A1[:, c:2 * c])
        P.conv_split('cv', cat, *P.w['cv'], True, G3, out=A1[:, 2 * c:3 * c - 2])
        copy_planes(flow, A1[:, 3 * c - 2:])
        z, r, q = (new(c), new(c)), (new(c), new(c)), (new(c), new(c))
        for i, (A, R, nxt) in enumerate(((A1, R1, A2), (A2, R2, None))):
            hf = '12'[i]
            copy_planes(A[:, c:], R[:, c:])
            if nxt is not None:
                copy_planes(A[:, c:], nxt[:, c:])
            zr_pre = P.conv_split('zr' + hf, A, *P.w['zr' + hf], False, G5)
            gru_gates_zr_recompute(zr_pre, A[:, :c], z[i], r[i], R[:, :c])
            q_pre = P.conv_split('q' + hf, R, *P.w['q' + hf], False, G5)
            gru_gates_h_recompute(q_pre, z[i], A[:, :c], q[i], nxt[:, :c] if nxt is not None else new(c))      # (net_k itself is not needed again)
        # the adjoints, second half first.  T = [d h_old | d x] of a half: first convq's data gradient ([d (r h) | d x]), then, with the
        # gates' terms written over its first c channels, one more term of the f64 sum behind convz | convr's data gradient
        grads, d, carry = {}, d_net, None
        for i, (A, R) in ((1, (A2, R2)), (0, (A1, R1))):
            hf = '12'[i]
            kernel = (1, 5) if i == 0 else (5, 1)
            dzr, dq, dh = new(2 * c), new(c), new(c)
            gru_gates_zq_backward(d, A[:, :c], z[i], q[i], dzr[:, :c], dq, dh)
            grads['q' + hf] = wgrad(R, dq, kernel)
            T = P.conv_split('q' + hf + 't', dq, P.w['q' + hf + 't'], None, False, G5)
            gru_gates_r_backward(T[:, :c], A[:, :c], r[i], dh, dzr[:, c:], T[:, :c])
            dw, db = wgrad(A, dzr, kernel)                     # convz | convr read the same input: one GEMM of 2 c output channels
            grads['z' + hf], grads['r' + hf] = (dw[:c], db[:c]), (dw[c:], db[c:])

            def fill(terms, T=T, carry=carry):
                copy_planes(T, terms[0])
                if carry is not None:                                   # the other half's d x (its d h_old went into this half as ``d``)
                    terms[1][:, :c].zero_()
                    copy_planes(carry[:, c:], terms[1][:, c:])
            carry = P.conv_split('zr' + hf + 't', dzr, P.w['zr' + hf + 't'], None, False, G5, extra=1 if carry is None else 2, fill=fill)
            d = carry[:, :c]
        d_net_prev, d_inp = new(c), new(c)
        copy_planes(carry[:, :c], d_net_prev)
        copy_planes(carry[:, c:2 * c], d_inp)
        # the motion encoder's adjoint (nothing into flow or corr)
        m = A1[:, 2 * c:3 * c - 2]
        dm = relu_backward(carry[:, 2 * c:3 * c - 2], m)
        grads['cv'] = wgrad(cat, dm, (3, 3))
        dcat = P.conv_split('cvt', dm, P.w['cvt'], None, False, G3)
        relu_backward(dcat, cat)
        grads['c2'] = wgrad(c1, dcat[:, :192], (3, 3))
        grads['f2'] = wgrad(f1, dcat[:, 192:], (3, 3))
        dc1 = P.conv_split('c2t', dcat[:, :192], P.w['c2t'], None, False, G3)
        relu_backward(dc1, c1)
        grads['c1'] = wgrad(corr, dc1, (1, 1))
        df1 = P.conv_split('f2t', dcat[:, 192:], P.w['f2t'], None, False, G3)
        relu_backward(df1, f1)
        grads['f1'] = wgrad(flow, df1, (7, 7))
        d_corr = P.conv_split('c1t', dc1, P.w['c1t'], None, False, G1) if ret_d_corr else None
    order = ('z1', 'r1', 'q1', 'z2', 'r2', 'q2', 'c1', 'c2', 'f1', 'f2', 'cv')
    out = (d_net_prev, d_inp, tuple(t for name in order for t in grads[name]))
    return out + (d_corr,) if ret_d_corr else out


# ------------------------------------------------------------------------------------------------- the encoders
class _EncoderPacked(_SplitConvs):
    """What the encoders' backward packs from an encoder's (or one block's) parameters: nothing at construction; the transposed, flipped
    weight of every stride-1 layer (``tr``) and each channel group's slice and PackedConv on first use, under the layer's name."""

    def __init__(self, params):
        super().__init__()

    def tr(self, name, weight):
        return self.get((name, 'tr'), lambda: weight.detach().transpose(0, 1).flip(2, 3).contiguous())


def _encoder_units(enc):
    """(name, conv, norm or None) of an encoder's convolutions in encoder_params' order."""
    units = [('conv1', enc.conv1, enc.norm1)]
    for ln in ('layer1', 'layer2', 'layer3'):
        for bi, blk in enumerate(getattr(enc, ln)):
            units += _block_units(blk, f'{ln}.{bi}')
    return units + [('conv2', enc.conv2, None)]


def _block_units(blk, name):
    units = [(f'{name}.conv1', blk.conv1, blk.norm1), (f'{name}.conv2', blk.conv2, blk.norm2)]
    if blk.downsample is not None:
        units.append((f'{name}.downsample', blk.downsample[0], blk.norm3))
    return units


def _unit_params(conv, norm):
    affine = norm is not None and getattr(norm, 'weight', None) is not None
    return [conv.weight, conv.bias] + ([norm.weight, norm.bias] if affine else [])


def encoder_params(enc):
    """A BasicEncoder's parameters in encoder_backward's order: the stem (conv1, norm1), then layer1[0], layer1[1], layer2[0], layer2[1],
    layer3[0], layer3[1] -- of each block conv1 / norm1, conv2 / norm2 and, where it has one, downsample[0] / norm3 --, then conv2.  Each
    convolution contributes (weight, bias), followed by its norm's (weight, bias) where the norm has them: 62 tensors with batch norm
    (cnet), 32 with instance norm (fnet, whose norms have no parameters)."""
    return [p for _, conv, norm in _encoder_units(enc) for p in _unit_params(conv, norm)]


def block_params(block):
    """One ResidualBlock's parameters in residual_block_backward's order (its part of encoder_params)."""
    return [p for _, conv, norm in _block_units(block, '') for p in _unit_params(conv, norm)]


def _conv_raw(P, name, conv, x):
    """conv(x) WITHOUT its bias, on the backward's unfused route: stride 1 through conv_split; stride 2 on ops.conv_direct, on groups of input
    channels of at most ENC_CHAIN terms added in f64 (one launch where the whole layer has no more: the 1x1 shortcuts, the stem)."""
    w = conv.weight.detach()
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    if conv.stride[0] == 1:
        return P.conv_split(name, x, w, None, False, ENC_GROUP_3X3_FWD if k == 3 else ENC_GROUP_1X1)
    group = max(1, ENC_CHAIN // (k * k))
    if cin <= group:
        return conv_direct(x, w, None, 2, k // 2)
    bounds = [(lo, min(cin, lo + group)) for lo in range(0, cin, group)]
    b, _, hi, wi = x.shape
    parts = torch.empty(len(bounds), b, cout, *ops._s2_out(hi, wi, k), dtype=torch.float32, device=x.device)
    for gi, (lo, hi_) in enumerate(bounds):
        conv_direct(x[:, lo:hi_], P.get((name, gi, 'w'), lambda: w[:, lo:hi_].contiguous()), None, 2, k // 2, out=parts[gi])
    return sum_groups(parts)


def _norm_act(P, name, conv, norm, z, relu, out=None):
    """relu?(norm(z + conv.bias)) into a new tensor (or ``out``); z, the raw convolution output, stays: the adjoint reads it."""
    out = torch.empty_like(z) if out is None else out
    if isinstance(norm, nn.BatchNorm2d):
        def fold():
            scale = (norm.weight / torch.sqrt(norm.running_var + norm.eps)).detach().float().contiguous()
            return scale, ((conv.bias - norm.running_mean) * scale + norm.bias).detach().float().contiguous()
        key = wkey(norm.running_mean, norm.running_var)
        scale, shift = P.get((name, 'affine', key), fold)
        return affine_act(z, scale, shift, relu=relu, out=out)
    return instnorm_act(z, conv.bias.detach(), eps=norm.eps, relu=relu, out=out)


def _norm_adjoint(conv, norm, dy, z):
    """The norm's adjoint in place on ``dy`` (behind the ReLU mask) -> (dz, the gradients of conv.bias and of the norm's parameters in
    encoder_params' order).  Instance norm: the bias cancels under the norm, its gradient is exact zeros."""
    if isinstance(norm, nn.BatchNorm2d):
        dz, dg, dbeta, dcb = bn_frozen_backward(dy, z, norm.weight.detach(), conv.bias.detach(), norm.running_mean, norm.running_var, norm.eps, dz=dy)
        return dz, [dcb, dg, dbeta]
    return instnorm_backward(dy, z, eps=norm.eps, dz=dy), [torch.zeros_like(conv.bias)]


def _block_forward(block, x, P, name):
    """One ResidualBlock again, every intermediate kept: out = relu(skip + relu(norm2(conv2(relu(norm1(conv1 x)))))), skip = x or
    norm3(conv1x1(x)) -> the record _block_backward reads."""
    r = {'x': x}
    r['z1'] = _conv_raw(P, f'{name}.conv1', block.conv1, x)
    r['a1'] = _norm_act(P, f'{name}.conv1', block.conv1, block.norm1, r['z1'], True)
    r['z2'] = _conv_raw(P, f'{name}.conv2', block.conv2, r['a1'])
    pair = torch.empty(2, *r['z2'].shape, dtype=torch.float32, device=x.device)          # (skip, y): the two terms of the residual add
    r['y'] = _norm_act(P, f'{name}.conv2', block.conv2, block.norm2, r['z2'], True, out=pair[1])
    if block.downsample is not None:
        r['zs'] = _conv_raw(P, f'{name}.downsample', block.downsample[0], x)
        _norm_act(P, f'{name}.downsample', block.downsample[0], block.norm3, r['zs'], False, out=pair[0])
    else:
        copy_planes(x, pair[0])
    r['out'] = sum_groups(pair, None, True)
    return r


def _block_backward(block, r, d_out, P, name, wgrad=_ENCODER):
    """-> (d_x, the block's gradients in block_params' order) from the record of _block_forward; ``wgrad``: _split_bwd_weight's keywords."""
    x, s2 = r['x'], block.downsample is not None
    g = relu_backward(d_out, r['out'], out=torch.empty_like(d_out))          # behind the block's last ReLU: ONE mask, the gradient of both paths
    gy = relu_backward(g, r['y'], out=torch.empty_like(g))
    dz2, gn2 = _norm_adjoint(block.conv2, block.norm2, gy, r['z2'])
    dw2 = _split_bwd_weight(r['a1'], dz2, (3, 3), False, **wgrad)[0]
    da1 = P.conv_split(f'{name}.conv2.t', dz2, P.tr(f'{name}.conv2', block.conv2.weight), None, False, ENC_GROUP_3X3_BWD)
    relu_backward(da1, r['a1'])
    dz1, gn1 = _norm_adjoint(block.conv1, block.norm1, da1, r['z1'])
    if not s2:
        dw1 = _split_bwd_weight(x, dz1, (3, 3), False, **wgrad)[0]
        # d x = conv1's data gradient + the shortcut's g, one more term of the same f64 sum
        d_x = P.conv_split(f'{name}.conv1.t', dz1, P.tr(f'{name}.conv1', block.conv1.weight), None, False, ENC_GROUP_3X3_BWD, extra=1,
                           fill=lambda terms: copy_planes(g, terms[0]))
        return d_x, [dw1] + gn1 + [dw2] + gn2
    dw1 = conv_s2_bwd_weight(x, dz1, 3, bias=False)[0]
    dzs, gns = _norm_adjoint(block.downsample[0], block.norm3, g, r['zs'])
    dws = conv_s2_bwd_weight(x, dzs, 1, bias=False)[0]
    both = torch.empty(2, *x.shape, dtype=torch.float32, device=x.device)
    conv_s2_bwd_data(dz1, block.conv1.weight, x.shape[-2:], out=both[0])
    conv_s2_bwd_data(dzs, block.downsample[0].weight, x.shape[-2:], out=both[1])
    return sum_groups(both), [dw1] + gn1 + [dw2] + gn2 + [dws] + gns


def _check_modes(who, module):
    """The refusals that need no tensor: a batch norm that would update its statistics, an active dropout."""
    for m in module.modules():
        if isinstance(m, nn.BatchNorm2d) and m.training:
            raise _lib.RpeError(f'{who}: the batch norms must be frozen (eval mode, RAFT.freeze_bn): a batch norm in training mode has no backward here')
        if isinstance(m, (nn.Dropout, nn.Dropout2d)) and m.training and m.p > 0:
            raise _lib.RpeError(f'{who}: dropout > 0 in training mode has no backward here')


def _check_block(who, block):
    if block.conv1.stride[0] not in (1, 2) or (block.conv1.stride[0] == 2) != (block.downsample is not None) \
            or not isinstance(block.norm1, (nn.BatchNorm2d, nn.InstanceNorm2d)):
        raise _lib.RpeError(f'{who}: expected a ResidualBlock of stride 1, or of stride 2 with the norm3(conv1x1) shortcut, with batch or instance norm')
    if isinstance(block.norm1, nn.InstanceNorm2d) and block.norm1.affine:
        raise _lib.RpeError(f'{who}: the instance norms have no affine parameters here (raft._norm)')


def residual_block_backward(block, x, d_out, packed, name='block'):
    """Backward of ONE ResidualBlock (csrc/encoder_backward.hip), both norm kinds, stride 1 and stride 2 with the norm3(conv1x1) shortcut:
    x (b,cin,h,w): the block's input; d_out: the gradient of its output; ``packed``: the _SplitConvs the weight slices are kept in
    (``_packed(_EncoderPacked, block_params(block))``, or the encoder's, with the block's ``name`` in it).
    -> (d_x, the gradients in block_params' order).  The block is recomputed from x on the unfused route; f32, bit-identical from run to run."""
    who = 'residual_block_backward'
    _check_modes(who, block)
    _check_block(who, block)
    x, d_out = _nchw(x, f'{who}: x'), _nchw(d_out, f'{who}: d_out')
    b, cin, hi, wi = x.shape
    st = block.conv1.stride[0]
    want = (b, block.conv2.out_channels) + ((hi, wi) if st == 1 else ops._s2_out(hi, wi, 3))
    if cin != block.conv1.in_channels or tuple(d_out.shape) != want:
        raise _lib.RpeError(f'{who}: x must have {block.conv1.in_channels} channels and d_out be {want}, got {tuple(x.shape)} and {tuple(d_out.shape)}')
    with torch.no_grad():
        return _block_backward(block, _block_forward(block, x, packed, name), d_out, packed, name)


def _encoder_out_shape(enc, n, hh, ww):
    for _ in range(3):
        hh, ww = ops._s2_out(hh, ww, 3)
    return (n, enc.conv2.out_channels, hh, ww)


def encoder_backward(enc, images, d_out, raw255=True, split_act=False, route=None, wgrad_bands=False):
    """Backward of a BasicEncoder (fnet: instance norm; cnet: frozen batch norm) for one batch: ``images`` as BasicEncoder.forward takes them
    (one batch or a list of batches, raw 0..255 with ``raw255``), d_out = d loss / d (the encoder's output), behind the tanh | ReLU of
    ``split_act`` when that is set -> the list of parameter gradients in encoder_params' order.  Nothing goes into the images.
    Every intermediate is recomputed from the images on an unfused route of its own -- the forward keeps nothing --: stride-1 layers and
    their data gradients through conv_split, stride-2 layers on ops.conv_direct, the norms as passes of their own; raw convolution outputs
    and block inputs live during the call only.  ``route``: the pass's raft.Route (RAFT hands its own; else the encoder's own flags under
    the module switches).  Refused before any launch: a batch norm in training mode, dropout > 0 in training mode, update_fp16,
    CONV_BF16X3, mixed_precision, tensors that are not float32, a d_out that is not the encoder's output shape.  f32, bit-identical
    from run to run.  ``wgrad_bands`` (the node sets it under a gradient per iteration): the stride-1 layers' weight gradients on maps of
    ENC_WGRAD_CHAIN < b h w <= ENC_BAND_CAP pixels in row bands added in f64; with it or without, a batch of several images of at most
    ENC_WGRAD_CHAIN pixels in all one image each, added in f64 (_split_bwd_weight's two encoder policies)."""
    from . import raft
    who = 'encoder_backward'
    _check_modes(who, enc)
    route = raft.resolve_route(pad_encoders=enc.pad_encoders) if route is None else route
    for flag, on in (('update_fp16', route.update_fp16), ('CONV_BF16X3', raft.CONV_BF16X3), ('mixed_precision', route.mixed_precision)):
        if on:
            raise _lib.RpeError(f'{who}: the encoders\' backward differentiates the f32 layers -- not with {flag}')
    many = list(images) if isinstance(images, (list, tuple)) else [images]
    for t in many + [d_out]:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise _lib.RpeError(f'{who}: images and d_out must be float32 tensors')
    if any(im.dim() != 4 or im.shape[1:] != many[0].shape[1:] or im.shape[1] != enc.conv1.in_channels for im in many):
        raise _lib.RpeError(f'{who}: images must be (n,{enc.conv1.in_channels},H,W) batches of one size')
    want = _encoder_out_shape(enc, sum(im.shape[0] for im in many), *many[0].shape[-2:])
    if tuple(d_out.shape) != want:
        raise _lib.RpeError(f'{who}: d_out must have the encoder\'s output shape {want}, got {tuple(d_out.shape)}')
    blocks = [(f'{ln}.{bi}', blk) for ln in ('layer1', 'layer2', 'layer3') for bi, blk in enumerate(getattr(enc, ln))]
    for name, blk in blocks:
        _check_block(f'{who}: {name}', blk)
    d_out = _nchw(d_out, f'{who}: d_out')
    P = _packed(_EncoderPacked, encoder_params(enc))
    half = enc.conv2.out_channels // 2
    with torch.no_grad():
        x0 = _nchw((torch.cat(many, dim=0) if len(many) > 1 else many[0]).contiguous(), f'{who}: images')
        if raw255:
            x0 = 2 * (x0 / 255.0) - 1.0
        # the forward, again
        z0 = _conv_raw(P, 'conv1', enc.conv1, x0)
        a0 = _norm_act(P, 'conv1', enc.conv1, enc.norm1, z0, True)
        recs, x = [], a0
        for name, blk in blocks:
            recs.append(_block_forward(blk, x, P, name))
            x = recs[-1]['out']
        w2, b2 = enc.conv2.weight.detach(), enc.conv2.bias.detach()
        if split_act:
            out = torch.empty(want, dtype=torch.float32, device=x.device)
            P.conv_split('conv2.lo', x, w2[:half], b2[:half].contiguous(), False, ENC_GROUP_1X1, out=out[:, :half])
            out[:, :half].tanh_()
            P.conv_split('conv2.hi', x, w2[half:], b2[half:].contiguous(), True, ENC_GROUP_1X1, out=out[:, half:])
            d = split_act_backward(d_out, out, half, out=torch.empty_like(d_out))
        else:
            d = d_out
        # the adjoints, last layer first
        wgrad = _ENCODER_BANDS if wgrad_bands else _ENCODER
        grads = list(_split_bwd_weight(x, d, (1, 1), **wgrad))
        d = P.conv_split('conv2.t', d, P.tr('conv2', w2), None, False, ENC_GROUP_1X1)
        for (name, blk), r in zip(reversed(blocks), reversed(recs)):
            d, g = _block_backward(blk, r, d, P, name, wgrad)
            grads = g + grads
            r.clear()
        relu_backward(d, a0)
        dz0, gn0 = _norm_adjoint(enc.conv1, enc.norm1, d, z0)
        return [conv_s2_bwd_weight(x0, dz0, 7, bias=False)[0]] + gn0 + grads


# ------------------------------------------------------------------------------------------------- a pass's record and the node
STAGES = ('heads', 'update', 'corr', 'encoders')


def _source_rows(source):
    """A record's source (images, lo, hi) -- ``images`` one raw image batch or a tuple of batches read as one -- -> [(batch, row in it)] of
    its rows lo .. hi - 1: the identity of each image."""
    images, lo, hi = source
    flat = [(im, r) for im in (images if isinstance(images, (list, tuple)) else (images,)) for r in range(im.shape[0])]
    if not 0 <= lo <= hi <= len(flat):
        raise _lib.RpeError(f'raft_grad: a source\'s rows {lo}:{hi} are not rows of its {len(flat)} images')
    return flat[lo:hi]


@dataclasses.dataclass(eq=False)
class GradPass:
    """What one gradient-free RAFT pass hands the node (the module docstring names the stages).  Absent stages are None, and nothing but
    which fields are present says how far the pass's backward goes (``depth``).  RAFT.grad_pass fills it with the pass's own tensors;
    ``rows`` makes of them the leaves whose .grad the backward fills."""
    flow_up: torch.Tensor                                    # (n,2,H,W): the pass's last prediction
    hidden: torch.Tensor                                     # (n,128,h8,w8): net_N
    flow_low: torch.Tensor                                   # (n,2,h8,w8): the last 1/8 flow
    net0: Optional[torch.Tensor] = None                      # 'update': (n,128,h8,w8), tanh half of the context encoder's output
    inp: Optional[torch.Tensor] = None                       # (n,128,h8,w8), its ReLU half
    states: Optional[List[Tuple[torch.Tensor, torch.Tensor]]] = None     # [(hx_k, coords1_k)], k = 1 .. N: every iteration's entry state
    pyr: Any = None                                          # the pass's correlation pyramid, no longer the model's
    fmap1: Optional[torch.Tensor] = None                     # 'corr': (n,256,h8,w8), the two maps the pass correlated
    fmap2: Optional[torch.Tensor] = None
    whole: Optional[tuple] = None                            # rows(): (the whole pass's coords1_k, lo, hi) -- the pyramid holds every row
    _last: tuple = (None, None)                              # corr's memo: (k, the whole pass's window of iteration k + 1)
    sources: Optional[tuple] = None                          # 'encoders': ((images, lo, hi) of fmap1, of fmap2, of the context): _source_rows
    earlier: Optional[List[torch.Tensor]] = None             # ``grad_all_flows``, any depth: the N - 1 earlier up-sampled predictions, k = 1 .. N - 1
    tail_states: Optional[List[Tuple[torch.Tensor, torch.Tensor]]] = None      # ... at 'heads', which has no states: [(net_k, flow_low_k)], k = 1 .. N - 1

    TENSORS = ('flow_up', 'hidden', 'flow_low', 'net0', 'inp', 'fmap1', 'fmap2')        # the node's tensor inputs, in this order
    LEAVES = ('hidden', 'net0', 'inp', 'fmap1', 'fmap2')                                # ... of which a backward fills the .grad

    @property
    def depth(self):
        return STAGES[(self.net0 is not None) + (self.fmap1 is not None) + (self.fmap1 is not None and self.sources is not None)]

    def tensors(self):
        """{field: tensor} of the tensor fields that are present, in field order."""
        return {name: getattr(self, name) for name in self.TENSORS if getattr(self, name) is not None}

    def rows(self, lo, hi):
        """The record of rows [lo, hi) of the batch: tensors and states sliced, ``hidden`` a detached leaf that requires grad, ``net0``,
        ``inp``, ``fmap1`` and ``fmap2`` cloned into fresh leaves, the sources' row ranges narrowed.  The pyramid stays whole: ``corr``
        slices the window."""
        leaf = lambda t: None if t is None else t[lo:hi].clone().requires_grad_(True)
        fleaf = lambda t: None if t is None else t[lo:hi].float().clone(memory_format=torch.contiguous_format).requires_grad_(True)
        states, whole = None, None
        if self.states is not None:
            states = [(st[lo:hi], co[lo:hi]) for st, co in self.states]
            coords, base = ([co for _, co in self.states], 0) if self.whole is None else self.whole[:2]
            whole = (coords, base + lo, base + hi)
        sources = None if self.sources is None else tuple((images, base + lo, base + hi) for images, base, _ in self.sources)
        earlier = None if self.earlier is None else [e[lo:hi].contiguous() for e in self.earlier]
        tails = None if self.tail_states is None else [(n[lo:hi], f[lo:hi]) for n, f in self.tail_states]
        return GradPass(self.flow_up[lo:hi].contiguous(), self.hidden[lo:hi].detach().requires_grad_(True), self.flow_low[lo:hi],
                        leaf(self.net0), leaf(self.inp), states, self.pyr, fleaf(self.fmap1), fleaf(self.fmap2), whole, sources=sources,
                        earlier=earlier, tail_states=tails)

    def tail_inputs(self, k):
        """(net_k, flow_low_k) of the earlier prediction k, 1 <= k < N, as contiguous tensors: what the heads read when they formed it.
        Below 'heads' both lie in the saved entry state of iteration k + 1 (``states[k]``): its first 128 channels (h_k, which the next
        step is about to update in place) and its last two (the flow the next motion encoder reads -- on the fused route the flow
        head's own output slot, on the generic route the same coords1 - coords0 the prediction was formed from; under pad_maps the
        content of the padded maps, as the returned hidden state and 1/8 flow are).  At 'heads' the pass kept copies of just these."""
        if self.tail_states is not None:
            net, flow = self.tail_states[k - 1]
        else:
            st = self.states[k][0]
            c = self.hidden.shape[1]
            net, flow = st[:, :c], st[:, st.shape[1] - 2:]
        fresh = lambda t: t if t.is_contiguous() else copy_planes(t, torch.empty(t.shape, dtype=torch.float32, device=t.device))
        return fresh(net), fresh(flow)

    def corr(self, k):
        """The window iteration k + 1 looked up (``states[k]`` = its (hx, coords1)): the pass's lookup on the saved coordinates against
        its pyramid, which the record keeps alive (the model builds itself a new one for its next pass) -- the forward's bits; of a
        record made by ``rows``, those rows of it.  The last k's window is kept.  (coords0 + flow_k would not do: coords1 - coords0
        rounds where a target lies much closer to column or row 0 than its source.)"""
        if self._last[0] != k:
            self._last = (k, self.pyr.lookup(self.states[k][1] if self.whole is None else self.whole[0][k]))
        return self._last[1] if self.whole is None else self._last[1][self.whole[1]:self.whole[2]]


def _by_field(passes, tensors):
    """The node's flat tensor inputs -> ([{field: tensor}] per pass, the parameters behind them)."""
    it = iter(tensors)
    return [{name: next(it) for name in p.tensors()} for p in passes], list(it)


def _through_time(rec, t, heads, upd, grads, g_early=(), hg=None):
    """The walk over one pass's predictions k = N .. 1, at every depth, behind grads['hidden'] = d net_N (the last tail's, at 'encoders'
    plus what arrived on hidden_out): the steps and, from 'corr' on, every step's lookup adjoint and, after step 1, the build's.  ``t``:
    the pass's tensor inputs by field; ``heads``: (the flow head's four parameters, the mask head's).  ``g_early`` (``grad_all_flows``):
    the gradients that arrived on the earlier predictions k = 1 .. N - 1, None where none did.  In front of step k + 1 -- the step that
    takes d net_k on to d net_{k-1} runs next -- a prediction k that received one runs its own tail (GradPass.tail_inputs(k)), whose d_net
    is ADDED to the carried d net_k.  While nothing has arrived yet the carried gradient is absent and the steps above the first such
    prediction are not run: they would carry zeros.  A record of depth 'heads' has no steps: the same walk runs its tails alone.
    ``hg``: the eight head gradients of the pass's last tail, or None; the earlier tails' are added to it one by one, so the heads' sum
    runs ((N + (N - 1)) + ...) + 1 at every depth.  Fills ``grads`` (field -> gradient); -> the heads' sum (None each without a tail),
    then the 22 update gradients summed in descending k (zeros for a pass without a step; none at 'heads'): without a gradient on an
    earlier prediction the float32 chain it always was; with one, every step forms its weight gradients in row bands on small maps
    (wgrad_bands) and the steps' 22 gradients are kept and added in f64, rounded once (_sum_f64)."""
    steps, with_corr = rec.states is not None, rec.fmap1 is not None
    inp, d = (t['inp'].detach() if steps else None), grads['hidden']
    d_inp, ug, vol, levels = None, None, None, None
    early, per_step = any(g is not None for g in g_early), []
    bands = {'wgrad_bands': True} if early else {}             # (absent without a gradient per iteration: the call of before)
    for k in reversed(range(len(rec.states) if steps else len(g_early))):
        if k < len(g_early) and g_early[k] is not None:                # prediction k + 1 < N, formed from net_{k+1}: states[k + 1]
            dn, tg = raft_tail_backward(*rec.tail_inputs(k + 1), g_early[k].contiguous(), *heads)
            hg = _plus(hg, tg)
            if steps:
                d = _plus(d, dn)
        if not steps or d is None:
            continue
        r = update_step_backward(rec.states[k][0], inp, rec.corr(k), d, upd, ret_d_corr=with_corr, **bands)
        d, di, sg = r[:3]
        if with_corr:
            if vol is None:
                levels = r[3].shape[1] // 81
                vol = ops.corr_grad_volume(r[3].shape[0], *r[3].shape[2:], levels, device=r[3].device)
            ops.corr_lookup_backward(rec.states[k][1], r[3], vol)
        d_inp = _plus(d_inp, di)
        if early:
            per_step.append(sg)
        else:
            ug = _plus(ug, sg)
    ug = _sum_f64(per_step) if per_step else ug if ug is not None else [torch.zeros_like(p) for p in upd]
    if steps:
        grads['net0'], grads['inp'] = d, d_inp
    if vol is not None:                                         # (S h8 w8 4 bytes per pair: freed on return, before the next pass)
        grads['fmap1'], grads['fmap2'] = ops.corr_build_backward(vol, t['fmap1'].detach(), t['fmap2'].detach(), levels)
    return [*(hg or [None] * 8), *ug]


def _plus(a, b):
    """a + b of two gradients, or of two lists of gradients element by element (-> a list); a, or an element of either, may be absent."""
    if isinstance(b, (list, tuple)):
        return list(b) if a is None else [_plus(x, y) for x, y in zip(a, b)]
    return b if a is None else a if b is None else a + b


def _per_image(contributions):
    """[(source, gradient (n,C,h8,w8) or None)] in walk order -> (the distinct images [(batch, row)] in the order of first appearance, their
    gradients as one batch): every image's contributions added in f64 and rounded once (sum_groups), a single one passed through.  An
    absent gradient contributes nothing, and an image nothing contributed to is left out."""
    order, terms = [], {}
    for source, g in contributions:
        if g is None:
            continue
        for i, (im, r) in enumerate(_source_rows(source)):
            key = (id(im), r)
            if key not in terms:
                order.append((im, r))
                terms[key] = []
            terms[key].append(g[i:i + 1])
    if not order:
        return [], None
    rows = [terms[id(im), r] for im, r in order]
    return order, torch.cat([ts[0] if len(ts) == 1 else sum_groups(torch.stack(ts).contiguous()) for ts in rows], dim=0)


def _image_batches(order):
    """[(batch, row)] -> the list of image batches encoder_backward takes: runs of consecutive rows of one batch stay one slice."""
    runs = []
    for im, r in order:
        if runs and runs[-1][0] is im and runs[-1][2] == r:
            runs[-1][2] = r + 1
        else:
            runs.append([im, r, r + 1])
    return [im if (lo, hi) == (0, im.shape[0]) else im[lo:hi] for im, lo, hi in runs]


def _encoders_backward(passes, all_grads, encoders, need, bands=False):
    """The encoders behind the last pass of an 'encoders' node: ``all_grads`` = every pass's {field: gradient}; ``need`` = (does a parameter
    of fnet, of cnet require grad) -> fnet's gradients + cnet's in encoder_params' order, None for an encoder that is not run."""
    fnet, cnet = encoders
    out = []
    walk_f = [(rec.sources[i], g[name]) for rec, g in zip(passes, all_grads) for i, name in ((0, 'fmap1'), (1, 'fmap2'))]
    walk_c = []
    for rec, g in zip(passes, all_grads):
        d0, di = g['net0'], g['inp']
        if d0 is None and di is None:
            continue
        d0, di = (torch.zeros_like(di) if d0 is None else d0), (torch.zeros_like(d0) if di is None else di)
        walk_c.append((rec.sources[2], torch.cat((d0, di), dim=1)))
    for enc, walk, split, wanted in ((fnet, walk_f, False, need[0]), (cnet, walk_c, True, need[1])):
        order, d = _per_image(walk) if wanted else ([], None)
        n = len(encoder_params(enc))
        out += [None] * n if d is None else list(encoder_backward(enc, _image_batches(order), d.contiguous(), raw255=True, split_act=split,
                                                                        **({'wgrad_bands': True} if bands else {})))
    return out


class _RaftGradFn(torch.autograd.Function):
    """Gradient-free RAFT passes as ONE autograd node: inputs the records' tensor fields, pass by pass in field order, then the eight head
    parameters, below 'heads' the 22 of UPDATE_PARAMS and at 'encoders' encoder_params(fnet) + encoder_params(cnet); outputs the
    up-sampled flows unchanged and, at 'encoders', behind them every pass's hidden_out and then every pass's context_out.  ``passes`` (the
    records) stay on the node.  Backward, per pass in the order given: the last tail, then the walk (_through_time); at 'encoders' the two
    encoders once, behind the last pass (_encoders_backward).  The parameter gradients are summed over the steps in descending k,
    concatenated (heads | update) per pass, then summed over the passes in the given order; a pass none of whose outputs anything
    differentiates is skipped and launches nothing: the sum's bits do not depend on the autograd engine's scheduling."""

    @staticmethod
    def forward(ctx, passes, encoders, *tensors):
        ctx.passes, ctx.encoders = passes, encoders
        ctx.save_for_backward(*tensors)
        ctx.set_materialize_grads(False)
        fields = _by_field(passes, tensors)[0]
        flows = tuple(t['flow_up'].view_as(t['flow_up']) for t in fields)
        early = tuple(e.detach() for p in passes for e in (p.earlier or ()))
        if encoders is None:
            return flows + early
        return flows + tuple(t['hidden'].detach() for t in fields) + tuple(t['inp'].detach() for t in fields) + early

    @staticmethod
    def backward(ctx, *grads_out):
        fields, params = _by_field(ctx.passes, ctx.saved_tensors)
        heads, upd, n, deep = (params[:4], params[4:8]), params[8:30], len(ctx.passes), ctx.encoders is not None
        totals, flat, all_grads, any_early = None, [], [], False
        at = 3 * n if deep else n                                  # the earlier predictions' gradients: behind the existing outputs, pass by pass
        for i, (rec, t) in enumerate(zip(ctx.passes, fields)):
            g, g_hid, g_ctx = grads_out[i], (grads_out[n + i] if deep else None), (grads_out[2 * n + i] if deep else None)
            g_early = grads_out[at:at + len(rec.earlier or ())]
            at += len(g_early)
            early = any(x is not None for x in g_early)
            any_early = any_early or early
            grads, both = dict.fromkeys(t), None
            if g is not None:
                grads['hidden'], both = raft_tail_backward(t['hidden'].detach(), t['flow_low'], g.contiguous(), *heads)
            grads['hidden'] = _plus(grads['hidden'], g_hid)        # (once, before step N)
            if grads['hidden'] is not None or early:
                both = _through_time(rec, t, heads, upd, grads, g_early, both)
            if g_ctx is not None:                                  # (once, behind the steps' sum)
                grads['inp'] = _plus(grads['inp'], g_ctx)
            totals = _plus(totals, both)
            flat += grads.values()
            all_grads.append(grads)
        totals = totals if totals is not None else [None] * 30
        if deep:
            need = ctx.needs_input_grad[2 + len(flat) + 30:]
            n_f = len(encoder_params(ctx.encoders[0]))
            totals += _encoders_backward(ctx.passes, all_grads, ctx.encoders, (any(need[:n_f]), any(need[n_f:])), any_early)
        return (None, None, *flat, *totals[:len(params)])


def attach(passes, head_params, update_params=None, encoders=None, ret_earlier=False):
    """Attach the backward to the results of gradient-free RAFT passes: ``passes`` = GradPass records of ONE depth whose ``hidden`` -- and,
    below 'heads', ``net0``, ``inp``, ``fmap1``, ``fmap2`` -- are leaves that require grad (GradPass.rows); ``head_params`` = RAFT.head_params(),
    ``update_params`` = RAFT.update_params() (needed below 'heads'), ``encoders`` = (fnet, cnet), the modules (needed at 'encoders', refused
    at every other depth) -> the list of up-sampled flows (the same values), outputs of one _RaftGradFn node; at 'encoders' the list of
    every pass's (flow, hidden_out, context_out).  After a backward the leaves' and the parameters' .grad are what the module docstring
    says of the passes' depth.  ``ret_earlier``: -> (that result, per pass the list of its ``earlier`` predictions as outputs of the same
    node -- empty for a pass that carries none)."""
    depth = {p.depth for p in passes}
    if len(depth) != 1:
        raise _lib.RpeError(f'raft_grad.attach: every pass must carry the same stages, got {sorted(depth)}')
    if (update_params is None) != (depth == {'heads'}):
        raise _lib.RpeError("raft_grad.attach: update_params goes with passes of depth 'update', 'corr' or 'encoders', and only with them")
    if (encoders is None) != (depth != {'encoders'}):
        raise _lib.RpeError("raft_grad.attach: encoders = (fnet, cnet) goes with passes of depth 'encoders', and only with them")
    fh, mk = head_params
    flat = [t for p in passes for t in p.tensors().values()]
    enc_params = [] if encoders is None else encoder_params(encoders[0]) + encoder_params(encoders[1])
    with torch.enable_grad():
        outs = _RaftGradFn.apply(list(passes), None if encoders is None else tuple(encoders), *flat, *fh, *mk, *(update_params or ()), *enc_params)
    n = len(passes)
    res = list(outs[:n]) if encoders is None else [(outs[i], outs[n + i], outs[2 * n + i]) for i in range(n)]
    if not ret_earlier:
        return res
    it = iter(outs[n if encoders is None else 3 * n:])
    return res, [[next(it) for _ in (p.earlier or ())] for p in passes]
