"""PoseNet host mirror (boundary B3): ``PoseNet(config).infer(image1l, image2l, intrinsics, baseline, depth1,
image2r, mask1, mask2, stereo_flow1, ret_details)`` and ``.flow2depth(imagel, imager, baseline)`` with the
reference's argument meaning (core/pose/pose_net.py:14-27,60-85,102-135) and parameter names (checkpoints load
unchanged: ``flow.*``, ``weight_head_2d.0.*``, ``weight_head_3d.0.*``, ``loss_weight``).

Per call: one batch-2n RAFT pass (hand-written HIP throughout: raft.py), one fused HIP pass for depth + back-projection +
the four warps + both 1/8 stacks, both TinyUNet heads as one HIP kernel chain (csrc/unet.hip; when they train: PyTorch-ROCm ops, or
the kernels of csrc/unet_train.hip with config['train_heads_hip']), and the device-resident SE(3) solve.  ``infer`` is generalised from the reference's hard-coded single frame
(``flow_predictions[-1][0]`` / ``[1]``, :66-67) to n frames by splitting the RAFT batch in halves.
"""
import torch
import torch.nn as nn

from . import ops, raft_grad
from .pose_head import DeclarativeLayerLie, DPoseSE3Head, create_img_coords_t
from .raft import RAFT
from .se3 import SE3
from .unet import TinyUNet, pack_params

FUSED_HEADS = True      # the heads on the HIP kernel chain (csrc/unet.hip); tools/ set this to False for A/B runs against the module route


class PoseNet(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.loss_weight = nn.Parameter(torch.tensor([1.0, 1.0]))
        H, W = config['image_shape']
        self.register_buffer('img_coords', create_img_coords_t(y=H, x=W), persistent=False)
        self.use_weights = config.get('use_weights', True)
        self.flow = RAFT(config)
        self.flow.freeze_bn()
        self.pose_head = DeclarativeLayerLie(DPoseSE3Head(self.img_coords, config.get('lbgfs_iters', 100),
                                                          solver=config.get('solver', 'lbfgs')))
        self.weight_head_2d = nn.Sequential(TinyUNet(in_channels=128 + 128 + 8, output_size=(H, W)), nn.Sigmoid())
        self.weight_head_3d = nn.Sequential(TinyUNet(in_channels=128 + 128 + 8 + 8, output_size=(H, W)), nn.Sigmoid())
        # config['train_heads_hip']: forward() (the training forward) runs the two heads, forward and backward, on the hand-written
        # training kernels instead of PyTorch-ROCm ops; only these two heads are switched, and inference is unaffected
        self.train_heads_hip = bool(config.get('train_heads_hip', False))
        if self.train_heads_hip:
            self.weight_head_2d[0].train_hip = self.weight_head_3d[0].train_hip = True

    def train(self, mode=True):
        super().train(mode)
        self.flow.eval()
        return self

    @torch.no_grad()
    def encode_frame(self, imagel, imager):
        """The encoder work of one new stereo frame -- fnet(left | right) and cnet(left) -- as ``infer(..., cache1=..., enc2=...)`` and
        ``flow2depth(..., enc=...)`` accept it: {'f': (2n,256,h/8,w/8), 'c': (n,256,h/8,w/8)}.  It depends on the frame's two images
        only, so a tracker can run it for frame t+1 (on a side stream) while frame t's update loop is still on the GPU
        (PoseEstimator.submit / result); the kernels and their inputs are the same, the results bit-identical."""
        f, c = self._encode_both((imagel, imager), imagel)
        return dict(f=f, c=c)

    @torch.no_grad()
    def flow2depth(self, imagel, imager, baseline, upsample=True, ret_cache=False, enc=None, grad=None):
        """pose_net.py:127-135 -> (depth (n,1,h,w), stereo flow (n,2,h,w), valid (n,1,h,w) bool).
        ``upsample=False``: everything at 1/8 resolution, the flow in 1/8-pixel units and the depth divided by 8 (:131-132;
        a division by a power of two commutes with the rounding of b / -flow.x, so the kernel is handed b / 8).
        ``ret_cache`` additionally returns the encoder outputs of ``imagel`` for reuse by the next ``infer``.
        ``grad`` = 'heads', 'update', 'corr' or 'encoders': the pass runs as RAFT.grad_pass runs it, and its raft_grad.GradPass, leaves
        made, is returned as a fourth element: what ``stages`` takes as ``pass1``.  At 'encoders' the record names ``imagel`` and ``imager``
        as the sources of its maps (not with ``enc``: maps encoded elsewhere cannot be differentiated here)."""
        n = imagel.shape[0]
        if grad == 'encoders' and enc is not None:
            raise ValueError("flow2depth: grad='encoders' encodes the images itself: not with enc=")
        f, cn = (enc['f'], enc['c']) if enc is not None else self._encode_both((imagel, imager), imagel)
        if grad is not None:
            kw = dict(sources=((imagel, 0, n), (imager, 0, n), (imagel, 0, n))) if grad == 'encoders' else {}
            r, rec = self.flow.grad_pass((f[:n], f[n:]), cn, stages=grad, upsample=upsample, **kw)
        else:
            r = self.flow(None, None, upsample=upsample, fmaps=(f[:n], f[n:]), cnet=cn)
        flow = r[0][-1]
        depth, valid = ops.flow2depth(flow, baseline if upsample else baseline / 8.0)
        if grad is not None:
            return depth, flow, valid, rec.rows(0, n)
        if ret_cache:
            return depth, flow, valid, dict(fmap=f[:n], cnet=cn)
        return depth, flow, valid

    def forward(self, image1l, image2l, intrinsics, baseline, image1r, image2r, mask1=None, mask2=None, ret_confmap=False, ret_flows=False,
                grad_corr=False):
        """The reference's TRAINING forward (core/pose/pose_net.py:28-58): both stereo depths, the temporal flow, the weight
        maps and the declarative pose layer -> (log-pose (n,6), depth1, depth2[, (w2d, w3d)]).  Gradients reach what the
        reference trains while the flow network is frozen (train.yaml: freeze_flow_steps; RAFT.eval() always): the two
        weight heads and ``loss_weight``, through the layer's closed-form backward (csrc/pose_backward.hip).  Flow, depth
        and the warps are computed by the (non-differentiable) HIP kernels, i.e. this mirrors the frozen-flow phase.
        ``ret_flows``: the gradients go one stage further, to the three flows.  The flows of the (still gradient-free) RAFT passes become
        leaves that require grad, depth1 comes from ``ops.flow2depth_grad`` and the geometry stage runs as ``ops.geometry_stage``
        (csrc/geometry_backward.hip), so the heads' inputs and the pose layer's time_flow / pcl1 / pcl2w carry gradients.  The result gains
        a last element {'time_flow', 'stereo_flow1', 'stereo_flow2'}: after ``loss.backward()`` each tensor's ``.grad`` is d loss / d that
        flow -- what a differentiable flow model has to be handed.  Values, and the gradients of the heads and ``loss_weight``, are those
        of the default call; without the flag nothing here changes, launches included.
        With RAFT's output heads trainable (``freeze_flow(False, parts='heads')``) the call takes the ``ret_flows`` route whether asked or
        not, and the three flows are the outputs of ONE autograd node (raft_grad.attach; passes in the order time, stereo1, stereo2)
        over the three RAFT results -- the ``flow2depth`` pass of frame 1 and both halves of the batched pass --, whose backward hands the
        pose loss's gradient to the flow head's and the mask head's eight parameters, summed over the three.  With the whole update
        block trainable (``freeze_flow(False, parts='update')``) the passes and the node go as deep as 'update': all 30 update-block
        parameters get the pose loss's exact gradient under upstream's detach of coords1 (raft_grad's module docstring says what each
        depth saves, costs and differentiates), and the dict gains 'net0' and 'inp', leaves per pass whose ``.grad`` is d loss / d net_0 and
        d loss / d inp.  The flows keep their ``.grad`` (retain_grad), and with ``ret_flows`` the returned dict gains 'hidden': {'time',
        'stereo1', 'stereo2'}, leaves whose ``.grad`` is the tail's d loss / d net_N, plus the weight heads' input gradient for 'time'.
        ``grad_corr`` (with ``ret_flows``): the call goes as deep as 'corr' whether or not the update block's parameters require grad: the
        dict gains 'fmap1' and 'fmap2', leaves per pass ('time', 'stereo1', 'stereo2') beside 'net0' and 'inp' -- copies of the rows of the
        feature maps each pass correlated -- whose ``.grad`` is d loss / d fmap: what a backward of the feature encoder has to be handed.
        Pose, depths and every other gradient keep their bits.  Refused before any launch with alternate_corr.
        With a parameter of an encoder trainable (``freeze_flow(False, parts='fnet' | 'cnet' | 'encoders' | 'raft')``) the call goes as deep as
        'encoders', whatever ``ret_flows`` and ``grad_corr`` say: the node runs each encoder's backward once, on the distinct images -- fnet
        on (1l, 2l, 1r, 2r), cnet on (1l, 2l), the gradients of the passes that share an image summed first --, and the weight heads read the
        time pass's ``hidden_out`` and ``context_out``, so the pose loss also reaches the GRU and the context encoder through the weight
        heads, as in the reference's training forward.  The dict carries the same leaf groups as with ``grad_corr``; their .grad hold
        the full gradients.  Pose, depths, weight maps and the gradients of the weight heads and ``loss_weight`` keep their bits."""
        n = image1l.shape[0]
        intrinsics = intrinsics.expand(n, 3, 3).contiguous()
        baseline = baseline.expand(n).contiguous()
        if grad_corr and not ret_flows:
            raise ValueError('PoseNet.forward: grad_corr returns its leaves in the dict of ret_flows: it needs ret_flows=True')
        grad = 'encoders' if self.flow_encoders_trainable() else 'corr' if grad_corr else 'update' if self.flow_update_trainable() \
            else 'heads' if self.flow_heads_trainable() else None
        if grad is not None:
            self.flow.check_grad(grad)                         # (before anything is launched)
        with torch.no_grad():
            pass1 = None
            if grad is not None:
                depth1, stereo_flow1, valid1, pass1 = self.flow2depth(image1l, image1r, baseline, grad=grad)
            else:
                depth1, stereo_flow1, valid1 = self.flow2depth(image1l, image1r, baseline)
            mask1 = (mask1.bool() & valid1) if mask1 is not None else valid1
            mask2 = mask2.bool().clone() if mask2 is not None else torch.ones_like(valid1)
            s = self.stages(image1l, image2l, intrinsics, baseline, depth1, image2r, mask1, mask2, stereo_flow1, heads=False,
                            grad_flows=ret_flows or grad is not None, pass1=pass1)
        if self.use_weights and self.train_heads_hip:
            # the heads' training route on hand-written kernels (csrc/unet_train.hip): the parts are read where they are (no torch.cat),
            # the Sigmoid modules' work is fused into the resize
            w2d = self.weight_head_2d[0].forward_train_hip((s['inp1'], s['hidden'], s['context']), sigmoid=True)
            w3d = self.weight_head_3d[0].forward_train_hip((s['inp1'], s['inp2'], s['hidden'], s['context']), sigmoid=True)
        elif self.use_weights:
            w2d = self.weight_head_2d(torch.cat((s['inp1'], s['hidden'], s['context']), dim=1))
            w3d = self.weight_head_3d(torch.cat((s['inp1'], s['inp2'], s['hidden'], s['context']), dim=1))
        else:
            w2d, w3d = torch.ones_like(s['depth2']), torch.ones_like(s['depth2'])
        _, log6 = self.pose_head(s['time_flow'], s['pcl1'], s['pcl2w'], w2d, w3d, mask1, s['mask2w'], s['intrinsics'],
                                 self.loss_weight.repeat(n, 1))
        pose_tan = log6.squeeze(1)
        out = (pose_tan, depth1, s['depth2'], (w2d, w3d)) if ret_confmap else (pose_tan, depth1, s['depth2'])
        if ret_flows:
            flows = {k: s[k] for k in ('time_flow', 'stereo_flow1', 'stereo_flow2')}
            flows.update({k: s[k + '_leaves'] for k in raft_grad.GradPass.LEAVES if k + '_leaves' in s})      # (the leaves of the passes' depth)
            out = (*out, flows)
        return out

    def flow_head_params(self):
        """RAFT's flow-head and mask-head parameters (raft_grad.raft_tail_backward's order): what ``freeze_flow(False, parts='heads')`` trains."""
        fh, mk = self.flow.head_params()
        return fh + mk

    def flow_heads_trainable(self):
        return any(p.requires_grad for p in self.flow_head_params())

    def flow_update_trainable(self):
        """Does a parameter of RAFT's SepConvGRU or motion encoder require grad (``freeze_flow(False, parts='update')``)?"""
        params = getattr(self.flow, 'update_params', None)
        return params is not None and any(p.requires_grad for p in params())

    def flow_encoder_params(self, which='encoders'):
        """The parameters of RAFT's feature encoder ('fnet'), context encoder ('cnet') or both, fnet's first, in raft_grad.encoder_params' order."""
        return [p for name in (('fnet', 'cnet') if which == 'encoders' else (which,)) for p in raft_grad.encoder_params(getattr(self.flow, name))]

    def flow_encoders_trainable(self):
        """Does a parameter of RAFT's encoders require grad (``freeze_flow(False, parts='fnet' | 'cnet' | 'encoders' | 'raft')``)?"""
        if not (hasattr(self.flow, 'fnet') and hasattr(self.flow, 'cnet')):
            return False
        return any(p.requires_grad for p in self.flow_encoder_params())

    def freeze_flow(self, freeze=True, parts=None):
        """pose_net.py:148-153.  Un-freezing the whole flow network needs its backward, which is built from the loss inwards as far as the
        update block: the gradients of the pose loss reach the three flows (``forward(..., ret_flows=True)``: the pose layer's and the geometry
        stage's backward), through the backward of RAFT's last flow-head / mask-head application (csrc/raft_backward.hip) those heads'
        parameters -- ``freeze_flow(False, parts='heads')`` sets requires_grad on ``flow.update_block.flow_head`` and ``flow.update_block.mask``
        only --, and through the backward of the N update steps (csrc/update_backward.hip, raft_grad.update_step_backward) the SepConvGRU and the
        motion encoder -- ``freeze_flow(False, parts='update')`` sets it on all of ``flow.update_block``.  The correlation has a backward as
        well (csrc/corr_backward.hip; it has no parameters): ``forward(..., ret_flows=True, grad_corr=True)`` hands the gradient to the two
        feature maps of every pass.  Behind it the two encoders have theirs (csrc/encoder_backward.hip, raft_grad.encoder_backward), run by
        the same node: ``parts='fnet'`` and ``parts='cnet'`` set requires_grad on that encoder's parameters only, ``parts='encoders'`` on both,
        and ``parts='raft'`` on every parameter of ``self.flow`` -- ``freeze_flow(False, parts='raft')`` is what the reference's
        ``freeze_flow(False)`` means here: the whole flow network trains on the pose loss through ``forward`` and ``loss.backward()``.
        The bare ``freeze_flow(False)`` without ``parts`` is still refused, with the message it had while the encoders had no backward:
        callers (and this project's tests) that rely on the refusal keep it, and training RAFT whole is asked for by name."""
        if parts not in (None, 'heads', 'update', 'fnet', 'cnet', 'encoders', 'raft'):
            raise ValueError(f"freeze_flow: parts must be None, 'heads', 'update', 'fnet', 'cnet', 'encoders' or 'raft', got {parts!r}")
        if not freeze and parts == 'heads':
            for p in self.flow_head_params():
                p.requires_grad = True
            return self
        if not freeze and parts == 'update':
            for p in self.flow.update_block.parameters():
                p.requires_grad = True
            return self
        if not freeze and parts in ('fnet', 'cnet', 'encoders'):
            for p in self.flow_encoder_params(parts):
                p.requires_grad = True
            return self
        if not freeze and parts == 'raft':
            for p in self.flow.parameters():
                p.requires_grad = True
            return self
        if not freeze:
            raise NotImplementedError('training the whole flow network (freeze_flow(False)) is out of scope: the gradients stop at the flows '
                                      '(forward(..., ret_flows=True) returns them), at RAFT\'s output heads (parts=\'heads\') or at its update '
                                      'block (parts=\'update\'), and through the correlation at the feature maps (grad_corr=True); the two '
                                      'encoders have no backward here under this spelling -- whole-network training, the reference\'s '
                                      'freeze_flow(False), is freeze_flow(False, parts=\'raft\')')
        for p in self.parameters():
            p.requires_grad = True
        for p in self.flow.parameters():
            p.requires_grad = False
        return self

    @torch.no_grad()
    def _encode_both(self, feature_images, context_images):
        """RAFT.encode_both (the two encoders side by side on two streams), or the two calls for a flow module that only has them."""
        both = getattr(self.flow, 'encode_both', None)
        if both is not None:
            return both(feature_images, context_images)
        return self.flow.encode_features(feature_images), self.flow.encode_context(context_images)

    def _heads(self, g, hidden, context):
        """(w2d, w3d) of a pass from ops.depth_backproject_warp's ``g`` and RAFT's hidden / context maps: both heads + resize + sigmoid as
        one hand-written kernel chain (csrc/unet.hip, no concatenations) when they are in eval mode and FUSED_HEADS is set, the modules
        otherwise, ones without ``use_weights``."""
        if not self.use_weights:
            return torch.ones_like(g['depth2']), torch.ones_like(g['depth2'])
        if FUSED_HEADS and not (self.weight_head_2d.training or self.weight_head_3d.training):
            return ops.unet_heads(g['inp1'], g['inp2'], hidden, context, pack_params(self.weight_head_2d[0]),
                                  pack_params(self.weight_head_3d[0]), self.config['image_shape'])
        return (self.weight_head_2d(torch.cat((g['inp1'], hidden, context), dim=1)),
                self.weight_head_3d(torch.cat((g['inp1'], g['inp2'], hidden, context), dim=1)))

    def _solve(self, inputs, rows_alone=False):
        """vec7 (n,1,7) of ``self.pose_head(*inputs)``.  ``rows_alone``: with ``partition_rows = 1`` for this solve, so that a row's float64
        sums are grouped as if it were solved alone and its result does not depend on the rows it shares the batch with."""
        problem = self.pose_head.problem
        keep = problem.partition_rows
        if rows_alone:
            problem.partition_rows = 1
        try:
            return self.pose_head(*inputs)[0]
        finally:
            problem.partition_rows = keep

    @torch.no_grad()
    def stages(self, image1l, image2l, intrinsics, baseline, depth1, image2r, mask1, mask2, stereo_flow1, cache1=None, heads=True, enc2=None,
               flow_init=None, ret_lowres=False, grad_flows=False, pass1=None):
        """Every stage of infer() before the solve.  ``cache1`` = {'fmap','cnet'} of image1l from the previous call
        (streaming: frame t's image2l is frame t+1's image1l), so only the two new images are encoded -- or not even those when
        ``enc2`` = encode_frame(image2l, image2r) was computed ahead of the call (needs cache1).
        ``flow_init`` (n,2,h/8,w/8): warm start of the n TEMPORAL pairs (RAFT.forward's flow_init); the n stereo pairs of the same RAFT
        batch start from zero, so depth and stereo flow are bit-identical to a cold pass.  ``ret_lowres``: the temporal pairs' last 1/8 flow
        (n,2,h/8,w/8) is added as 'time_flow_low' to the result and to its 'cache2'.
        ``grad_flows`` (the training forward's ``ret_flows``): time_flow, stereo_flow2 and stereo_flow1 become leaves that require grad
        ('stereo_flow1' is added to the result) and the geometry stage runs, with gradients enabled, through ``ops.flow2depth_grad`` and
        ``ops.geometry_stage``: the same values, now differentiable with respect to the three flows.
        ``pass1`` = the raft_grad.GradPass of the pass that made stereo_flow1 (flow2depth's ``grad``; needs grad_flows): RAFT trains as deep
        as that record goes.  The batched pass runs as deep (RAFT.grad_pass), its two halves are rows of its record, and the three flows
        leave ONE raft_grad.attach node over (time, stereo1, stereo2).  'hidden' is the temporal pairs' hidden state as a leaf that requires
        grad -- at depth 'encoders' 'hidden' and 'context' are the time pass's hidden_out and context_out of the node, and the batched pass's
        record names (image1l | image2l), (image2l | image2r) and (image1l | image2l) as the sources of its maps --, and for every leaf field the records carry -- 'hidden'; 'net0', 'inp'; 'fmap1', 'fmap2' -- the result gains
        '<field>_leaves' = {'time', 'stereo1', 'stereo2'}."""
        n = image1l.shape[0]
        intrinsics = intrinsics.expand(n, 3, 3).contiguous()
        baseline = baseline.expand(n).contiguous()
        # The reference's batch-2 RAFT call is (image1l, image2l) -> (image2l, image2r) (pose_net.py:63-64).  image2l sits in both
        # halves and the feature encoder normalises per sample, so it is encoded once: f = (f1l | f2l | f2r) in ONE encoder batch
        # whose overlapping slices f[:2n], f[n:] ARE the two operand batches of the correlation -- no torch.cat of images or maps
        if cache1 is None:
            f, cn = self._encode_both((image1l, image2l, image2r), (image1l, image2l))
            f2l = f[n:2 * n]
            fmaps = (f[:2 * n], f[n:])
            c2l = cn[n:]
        else:
            f, c2l = (enc2['f'], enc2['c']) if enc2 is not None else self._encode_both((image2l, image2r), image2l)
            f2l = f[:n]
            fmaps = (torch.cat((cache1['fmap'], f2l), dim=0), f)
            cn = torch.cat((cache1['cnet'], c2l), dim=0)
        kw = {}
        if flow_init is not None:
            kw['flow_init'] = torch.cat((flow_init, torch.zeros_like(flow_init)), dim=0)      # (temporal | stereo) rows of the RAFT batch
        if pass1 is not None:
            deep = pass1.depth == 'encoders'
            if deep and cache1 is not None:
                raise ValueError("stages: a pass1 of depth 'encoders' encodes every image here: not with cache1=")
            if deep:                                          # (fmaps = f[:2n], f[n:] of f = fnet(1l | 2l | 2r); cn = cnet(1l | 2l))
                kw['sources'] = (((image1l, image2l), 0, 2 * n), ((image2l, image2r), 0, 2 * n), ((image1l, image2l), 0, 2 * n))
            r, rec2 = self.flow.grad_pass(fmaps, cn, stages=pass1.depth, upsample=True, **kw)
        else:
            r = self.flow(None, None, upsample=True, fmaps=fmaps, cnet=cn, ret_lowres=ret_lowres, **kw)
        flow_predictions, hidden, context = r[:3]
        time_flow = flow_predictions[-1][:n].contiguous()
        stereo_flow2 = flow_predictions[-1][n:].contiguous()
        hidden, context = hidden[:n], context[:n]
        passes = None
        if grad_flows:
            with torch.enable_grad():
                if pass1 is not None:
                    passes = dict(time=rec2.rows(0, n), stereo1=pass1, stereo2=rec2.rows(n, 2 * n))
                    hidden = passes['time'].hidden             # (the weight heads read it: their input gradient lands in its .grad)
                    outs = raft_grad.attach(list(passes.values()), self.flow.head_params(), None if pass1.depth == 'heads' else self.flow.update_params(),
                                            (self.flow.fnet, self.flow.cnet) if deep else None)
                    if deep:                                   # (the weight heads read the node's outputs: their input gradients return into the chain)
                        _, hidden, context = outs[0]
                        outs = [o[0] for o in outs]
                    time_flow, stereo_flow1, stereo_flow2 = outs
                    for t in (time_flow, stereo_flow1, stereo_flow2):
                        t.retain_grad()
                else:
                    time_flow, stereo_flow2, stereo_flow1 = (t.detach().requires_grad_(True) for t in (time_flow, stereo_flow2, stereo_flow1))
                g = ops.geometry_stage(stereo_flow2, time_flow, baseline, intrinsics, ops.flow2depth_grad(stereo_flow1, baseline)[0],
                                       image1l, image2l, stereo_flow1, mask2)
            g['stereo_flow1'] = stereo_flow1
        else:
            g = ops.depth_backproject_warp(stereo_flow2, time_flow, baseline, intrinsics, depth1, image1l, image2l,
                                           stereo_flow1, mask2)
        w2d, w3d = self._heads(g, hidden, context) if heads else (None, None)
        g.update(time_flow=time_flow, stereo_flow2=stereo_flow2, hidden=hidden, context=context, w2d=w2d, w3d=w3d,
                 intrinsics=intrinsics, cache2=dict(fmap=f2l, cnet=c2l))
        if passes is not None:
            g.update({k + '_leaves': {p: getattr(rec, k) for p, rec in passes.items()} for k in raft_grad.GradPass.LEAVES if getattr(pass1, k) is not None})
        if ret_lowres:
            g['time_flow_low'] = g['cache2']['time_flow_low'] = r[3][:n]
        return g

    @torch.no_grad()
    def infer(self, image1l, image2l, intrinsics, baseline, depth1, image2r, mask1, mask2, stereo_flow1,
              ret_details=False, cache1=None, ret_cache=False, enc2=None, flow_init=None, ret_lowres=False, ret_quality=False, rows_alone=False):
        """``flow_init`` / ``ret_lowres``: see stages (warm start of the temporal pairs; the temporal 1/8 flow comes back as the returned
        cache's 'time_flow_low', so ret_lowres needs ret_cache).
        ``ret_quality`` (needs ret_details): the details gain, behind stereo_flow2, the solve-quality report of the n rows as a dict of
        device tensors (``_quality``): two more launches, no host synchronisation; everything else is unchanged bit for bit.
        ``rows_alone``: every row's solve as if it were alone in the batch (``_solve``), for callers that batch independent sequences."""
        if enc2 is not None and cache1 is None:
            raise ValueError('infer: enc2 (the new frame encoded ahead of the call) needs cache1 (the previous frame\'s encoder outputs)')
        if ret_lowres and not ret_cache:
            raise ValueError("infer: ret_lowres returns the temporal 1/8 flow in the cache dict ('time_flow_low'): it needs ret_cache=True")
        if ret_quality and not ret_details:
            raise ValueError('infer: ret_quality adds the quality report to the details: it needs ret_details=True')
        s = self.stages(image1l, image2l, intrinsics, baseline, depth1, image2r, mask1, mask2, stereo_flow1, cache1, enc2=enc2,
                        flow_init=flow_init, ret_lowres=ret_lowres)
        mask2.copy_(s['mask2'])                               # `mask2 &= valid` mutates the caller's tensor (:77)
        n = image1l.shape[0]
        lw = self.loss_weight.detach()[None, :].repeat(n, 1)
        inputs = (s['time_flow'], s['pcl1'], s['pcl2w'], s['w2d'], s['w3d'], mask1.bool(), s['mask2w'], s['intrinsics'], lw)
        vec7 = self._solve(inputs, rows_alone)
        pose = SE3(vec7[:, 0]) if n > 1 else SE3(vec7)[0]     # reference returns SE3(pose_se3)[0] for its n == 1
        out = (pose, depth1, s['depth2'], (s['w2d'], s['w3d']), s['time_flow'], s['stereo_flow2']) if ret_details else pose
        if ret_quality:
            out = (*out, self._quality(inputs))
        if ret_cache:
            return (*out, s['cache2']) if ret_details else (out, s['cache2'])
        return out

    def _quality(self, inputs):
        """The report of the solve that has just run on ``inputs``, at its float64 pose: cov (n,6,6), pd, n2d, n3d, rms2d_px, rms3d, f,
        grad_max (f64; ops.quality_fields) and n_iter, func_evals, stop_reason (int32, the solve's info).  Device tensors, in the
        solve's normalised units."""
        problem = self.pose_head.problem
        q = ops.quality_fields(problem.quality(*inputs))
        info = problem.last_info
        d = {k: q[k] for k in ('cov', 'pd', 'n2d', 'n3d', 'rms2d_px', 'rms3d', 'f', 'grad_max')}
        d.update(n_iter=info[:, 0], func_evals=info[:, 1], stop_reason=info[:, 2])
        return d

    @torch.no_grad()
    def infer_chunk(self, image0l, imagesl, imagesr, intrinsics, baseline, depth0, mask0, masks, stereo_flow0, cache0=None,
                    depth_roundtrip=None, ret_quality=False):
        """c consecutive calls of ``infer`` as ONE pass: frame t of the chunk is ``infer(image1l = frame t-1, image2l = frame t, ...)``
        with frame -1 = (image0l, depth0, mask0, stereo_flow0) and, for t > 0, depth1 / mask1 / stereo_flow1 = the depth2 / mask2 /
        stereo_flow2 that call t-1 produced (core/pose/pose_estimator.py:113-122 feeds them back through its Frame) -- a shift by one
        row INSIDE the batch, after the 2c RAFT pairs, which are independent.  imagesl, imagesr (c,3,h,w) 0..255; masks (c,1,h,w) bool,
        ANDed in place with the stereo validity like ``infer``'s mask2 (pose_net.py:77); depth0 / stereo_flow0 / mask0 (1,..) as ``infer``
        takes them; ``cache0`` = encoder outputs of image0l ({'fmap','cnet'}) when the caller has them.
        ``depth_roundtrip`` = s: depth1 of row t > 0 is (depth2[t-1] / s) * s, the two roundings PoseEstimator's Frame puts between
        consecutive calls (it stores depth / scale and hands over depth * scale, pose_estimator.py:107,116,121).
        Every kernel on the way computes a row independently of its batch (tests), and the solve runs with partition_rows = 1, so the
        result is BIT-IDENTICAL to the c single calls.  Returns (vec7 (c,7) f32, depth2 (c,1,h,w), (w2d, w3d), time_flow (c,2,h,w),
        stereo_flow2 (c,2,h,w), cache of the last frame[, the quality dict of ``infer`` with one row per frame, with ``ret_quality``])."""
        c = imagesl.shape[0]
        intrinsics = intrinsics.expand(c, 3, 3).contiguous()
        baseline = baseline.expand(c).contiguous()
        f, cn = self._encode_both((imagesl, imagesr), imagesl)          # f = (L_0..L_c-1 | R_0..R_c-1)
        fl = f[:c]
        if cache0 is None:
            f0, c0 = self.flow.encode_features(image0l), self.flow.encode_context(image0l)
        else:
            f0, c0 = cache0['fmap'], cache0['cnet']
        # pairs: temporal (L_t-1 -> L_t) for t = 0..c-1, then stereo (L_t -> R_t): the order PoseNet.stages uses per frame
        fmap1 = torch.cat((f0, fl[:c - 1], fl), dim=0)
        cnet = torch.cat((c0, cn[:c - 1], cn), dim=0)
        flows, hidden, context = self.flow(None, None, upsample=True, fmaps=(fmap1, f), cnet=cnet)
        time_flow = flows[-1][:c].contiguous()
        stereo_flow2 = flows[-1][c:].contiguous()
        hidden, context = hidden[:c], context[:c]
        depth2, valid = ops.flow2depth(stereo_flow2, baseline)            # the same division and tests rpe_depth_backproject_warp repeats
        masks &= valid
        d_prev = depth2[:c - 1]
        if depth_roundtrip is not None:
            d_prev = (d_prev / depth_roundtrip) * depth_roundtrip
        depth1 = torch.cat((depth0, d_prev), dim=0)
        mask1 = torch.cat((mask0.bool(), masks[:c - 1]), dim=0)
        stereo_flow1 = torch.cat((stereo_flow0, stereo_flow2[:c - 1]), dim=0)
        image1l = torch.cat((image0l, imagesl[:c - 1]), dim=0)
        g = ops.depth_backproject_warp(stereo_flow2, time_flow, baseline, intrinsics, depth1, image1l, imagesl, stereo_flow1, masks)
        if self.use_weights and not FUSED_HEADS:
            # the A/B switch selects the module route in _heads(); here it would silently break forward_chunk == c forward calls
            raise RuntimeError('infer_chunk runs the fused weight heads only: set pose_net.FUSED_HEADS = True (or walk the frames with infer)')
        if self.use_weights and (self.weight_head_2d.training or self.weight_head_3d.training):
            raise RuntimeError('infer_chunk: the weight heads must be in eval mode')
        w2d, w3d = self._heads(g, hidden, context)
        lw = self.loss_weight.detach()[None, :].repeat(c, 1)
        inputs = (time_flow, g['pcl1'], g['pcl2w'], w2d, w3d, mask1, g['mask2w'], intrinsics, lw)
        vec7 = self._solve(inputs, rows_alone=True)
        out = (vec7[:, 0], g['depth2'], (w2d, w3d), time_flow, stereo_flow2, dict(fmap=fl[c - 1:], cnet=cn[c - 1:]))
        return (*out, self._quality(inputs)) if ret_quality else out

    def init_from_raft(self, raft_ckp):
        state = torch.load(raft_ckp, map_location='cpu')
        self.flow.load_state_dict({k.replace('module.', ''): v for k, v in state.items()})
        return self
