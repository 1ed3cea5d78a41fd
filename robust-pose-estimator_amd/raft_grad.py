"""RAFT's backward for training on the pose loss, composed on the host from the one-kernel wrappers of ops.py: the two stage functions
(raft_tail_backward, update_step_backward), the weight packings they run on, the record of what a pass saves (GradPass) and the ONE
autograd node over such records (attach).  The forward stays what it is -- a gradient-free pass, the launches and the bits of a
``ret_lowres`` pass --; RAFT.grad_pass runs it and fills the record, RAFT.forward(grad_heads= / grad_update= / grad_corr=) and
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
Refused before any launch (RAFT.check_grad_heads): update_fp16, CONV_BF16X3, mixed_precision -- a route that rounds the heads' operands
has no honest gradient here -- and upsample=False; for 'corr' also alternate_corr (no pyramid) and CORR_BF16X3 (RAFT.check_grad_corr)."""
import dataclasses
from typing import Any, List, Optional, Tuple

import torch

from . import _lib, ops
from .ops import (CONV_LINEAR, PackedConv, _nchw, bounded_put, conv3x3_to2_bwd_data, conv_bwd_weight, conv_direct, conv_fused, copy_planes,
                  gru_gates_h_recompute, gru_gates_r_backward, gru_gates_zq_backward, gru_gates_zr_recompute, relu_backward, sum_groups,
                  upsample_convex_backward, wkey)

TAIL_GROUP_3X3_FWD, TAIL_GROUP_3X3_BWD, TAIL_GROUP_1X1 = 16, 32, 64      # input channels per launch of the tail's forward-kernel convolutions
# update_step_backward's parameter (and gradient) order: weight, bias of each -- 12 tensors of ``gru``, 10 of ``encoder``
UPDATE_PARAMS = tuple(f'{m}.{t}' for m in ('gru.convz1', 'gru.convr1', 'gru.convq1', 'gru.convz2', 'gru.convr2', 'gru.convq2', 'encoder.convc1',
                                           'encoder.convc2', 'encoder.convf1', 'encoder.convf2', 'encoder.conv') for t in ('weight', 'bias'))
# input channels per launch of the step's forward-kernel convolutions (forward recomputation and data gradients alike): 144 terms of a 3x3
# layer, 160 of a 5-tap layer, 64 of the 1x1 -- the k-ordered f32 chain of a launch stays below the tail's 288, the groups are added in f64
UPDATE_GROUP_3X3, UPDATE_GROUP_5TAP, UPDATE_GROUP_1X1 = 16, 32, 64


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


def update_step_backward(hx, inp, corr, d_net, params, ret_d_corr=False):
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
    paths are added in that same f64 sum.  f32 throughout, bit-identical from run to run, a row's result independent of its batch."""
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
            grads['q' + hf] = conv_bwd_weight(R, dq, kernel)
            T = P.conv_split('q' + hf + 't', dq, P.w['q' + hf + 't'], None, False, G5)
            gru_gates_r_backward(T[:, :c], A[:, :c], r[i], dh, dzr[:, c:], T[:, :c])
            dw, db = conv_bwd_weight(A, dzr, kernel)                     # convz | convr read the same input: one GEMM of 2 c output channels
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
        grads['cv'] = conv_bwd_weight(cat, dm, (3, 3))
        dcat = P.conv_split('cvt', dm, P.w['cvt'], None, False, G3)
        relu_backward(dcat, cat)
        grads['c2'] = conv_bwd_weight(c1, dcat[:, :192], (3, 3))
        grads['f2'] = conv_bwd_weight(f1, dcat[:, 192:], (3, 3))
        dc1 = P.conv_split('c2t', dcat[:, :192], P.w['c2t'], None, False, G3)
        relu_backward(dc1, c1)
        grads['c1'] = conv_bwd_weight(corr, dc1, (1, 1))
        df1 = P.conv_split('f2t', dcat[:, 192:], P.w['f2t'], None, False, G3)
        relu_backward(df1, f1)
        grads['f1'] = conv_bwd_weight(flow, df1, (7, 7))
        d_corr = P.conv_split('c1t', dc1, P.w['c1t'], None, False, G1) if ret_d_corr else None
    order = ('z1', 'r1', 'q1', 'z2', 'r2', 'q2', 'c1', 'c2', 'f1', 'f2', 'cv')
    out = (d_net_prev, d_inp, tuple(t for name in order for t in grads[name]))
    return out + (d_corr,) if ret_d_corr else out


# ------------------------------------------------------------------------------------------------- a pass's record and the node
STAGES = ('heads', 'update', 'corr')


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

    TENSORS = ('flow_up', 'hidden', 'flow_low', 'net0', 'inp', 'fmap1', 'fmap2')        # the node's tensor inputs, in this order
    LEAVES = ('hidden', 'net0', 'inp', 'fmap1', 'fmap2')                                # ... of which a backward fills the .grad

    @property
    def depth(self):
        return STAGES[(self.net0 is not None) + (self.fmap1 is not None)]

    def tensors(self):
        """{field: tensor} of the tensor fields that are present, in field order."""
        return {name: getattr(self, name) for name in self.TENSORS if getattr(self, name) is not None}

    def rows(self, lo, hi):
        """The record of rows [lo, hi) of the batch: tensors and states sliced, ``hidden`` a detached leaf that requires grad, ``net0``,
        ``inp``, ``fmap1`` and ``fmap2`` cloned into fresh leaves.  The pyramid stays whole: ``corr`` slices the window."""
        leaf = lambda t: None if t is None else t[lo:hi].clone().requires_grad_(True)
        fleaf = lambda t: None if t is None else t[lo:hi].float().clone(memory_format=torch.contiguous_format).requires_grad_(True)
        states, whole = None, None
        if self.states is not None:
            states = [(st[lo:hi], co[lo:hi]) for st, co in self.states]
            coords, base = ([co for _, co in self.states], 0) if self.whole is None else self.whole[:2]
            whole = (coords, base + lo, base + hi)
        return GradPass(self.flow_up[lo:hi].contiguous(), self.hidden[lo:hi].detach().requires_grad_(True), self.flow_low[lo:hi],
                        leaf(self.net0), leaf(self.inp), states, self.pyr, fleaf(self.fmap1), fleaf(self.fmap2), whole)

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


def _through_time(rec, t, upd, grads):
    """The steps k = N .. 1 of one pass behind its tail's grads['hidden'] = d net_N; at 'corr' depth every step's lookup adjoint and, after
    step 1, the build's.  ``t``: the pass's tensor inputs by field.  Fills ``grads`` (field -> gradient); -> the 22 update gradients
    summed in descending k (zeros for a pass without states)."""
    with_corr = rec.depth == 'corr'
    inp, d = t['inp'].detach(), grads['hidden']
    d_inp, ug, vol, levels = None, None, None, None
    for k in reversed(range(len(rec.states))):
        r = update_step_backward(rec.states[k][0], inp, rec.corr(k), d, upd, ret_d_corr=with_corr)
        d, di, sg = r[:3]
        if with_corr:
            if vol is None:
                levels = r[3].shape[1] // 81
                vol = ops.corr_grad_volume(r[3].shape[0], *r[3].shape[2:], levels, device=r[3].device)
            ops.corr_lookup_backward(rec.states[k][1], r[3], vol)
        d_inp = di if d_inp is None else d_inp + di
        ug = list(sg) if ug is None else [a + b for a, b in zip(ug, sg)]
    grads['net0'], grads['inp'] = d, d_inp
    if vol is not None:                                         # (S h8 w8 4 bytes per pair: freed on return, before the next pass)
        grads['fmap1'], grads['fmap2'] = ops.corr_build_backward(vol, t['fmap1'].detach(), t['fmap2'].detach(), levels)
    return ug if ug is not None else [torch.zeros_like(p) for p in upd]


class _RaftGradFn(torch.autograd.Function):
    """Gradient-free RAFT passes as ONE autograd node: inputs the records' tensor fields, pass by pass in field order, then the eight head
    parameters and, below 'heads', the 22 of UPDATE_PARAMS; outputs the up-sampled flows unchanged.  ``passes`` (the records) stay on the
    node.  Backward, per pass in the order given: the tail, then the steps (_through_time).  The parameter gradients are summed over the
    steps in descending k, concatenated (heads | update) per pass, then summed over the passes in the given order; a pass whose flow
    nothing differentiates is skipped and launches nothing: the sum's bits do not depend on the autograd engine's scheduling."""

    @staticmethod
    def forward(ctx, passes, *tensors):
        ctx.passes = passes
        ctx.save_for_backward(*tensors)
        ctx.set_materialize_grads(False)
        return tuple(t['flow_up'].view_as(t['flow_up']) for t in _by_field(passes, tensors)[0])

    @staticmethod
    def backward(ctx, *grads_up):
        fields, params = _by_field(ctx.passes, ctx.saved_tensors)
        heads, upd = params[:8], params[8:]
        totals, flat = None, []
        for rec, t, g in zip(ctx.passes, fields, grads_up):
            grads = dict.fromkeys(t)
            if g is not None:
                grads['hidden'], both = raft_tail_backward(t['hidden'].detach(), t['flow_low'], g.contiguous(), heads[:4], heads[4:])
                both = list(both)
                if rec.depth != 'heads':
                    both += _through_time(rec, t, upd, grads)
                totals = both if totals is None else [a + b for a, b in zip(totals, both)]
            flat += grads.values()
        return (None, *flat, *(totals if totals is not None else [None] * len(params)))


def attach(passes, head_params, update_params=None):
    """Attach the backward to the results of gradient-free RAFT passes: ``passes`` = GradPass records of ONE depth whose ``hidden`` -- and,
    below 'heads', ``net0``, ``inp``, ``fmap1``, ``fmap2`` -- are leaves that require grad (GradPass.rows); ``head_params`` = RAFT.head_params(),
    ``update_params`` = RAFT.update_params() (needed below 'heads') -> the list of up-sampled flows (the same values), outputs of one
    _RaftGradFn node.  After a backward the leaves' and the parameters' .grad are what the module docstring says of the passes' depth."""
    depth = {p.depth for p in passes}
    if len(depth) != 1:
        raise _lib.RpeError(f'raft_grad.attach: every pass must carry the same stages, got {sorted(depth)}')
    if (update_params is None) != (depth == {'heads'}):
        raise _lib.RpeError("raft_grad.attach: update_params goes with passes of depth 'update' or 'corr', and only with them")
    fh, mk = head_params
    flat = [t for p in passes for t in p.tensors().values()]
    with torch.enable_grad():
        return list(_RaftGradFn.apply(list(passes), *flat, *fh, *mk, *(update_params or ())))
