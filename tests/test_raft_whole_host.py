"""CPU: the host side of whole-network training -- RAFT.forward(grad_encoders=True)'s refusals, raised where any launch would fail, and
PoseNet.freeze_flow's new ``parts``."""
import pytest
import torch
import torch.nn as nn


def test_grad_encoders_refusals_before_any_launch(rpe):
    from rpe_amd import raft, synth
    from rpe_amd._lib import RpeError
    img = torch.zeros(1, 3, 64, 96)
    model = raft.RAFT(synth.model_config(64, 96)).eval()
    f, c = torch.zeros(1, 256, 8, 12), torch.zeros(1, 256, 8, 12)
    for kw in (dict(fmaps=(f, f)), dict(cnet=c), dict(fmaps=(f, f), cnet=c)):
        with pytest.raises(RpeError, match='computed elsewhere'):
            model(img, img, grad_encoders=True, **kw)
    with pytest.raises(RpeError, match='computed elsewhere'):
        model(None, None, grad_encoders=True, fmaps=(f, f), cnet=c)
    # a batch norm in training mode, in either encoder's place (fnet has none: cnet's stem and a block's)
    for norm in (model.cnet.norm1, model.cnet.layer2[0].norm3):
        norm.train()
        with pytest.raises(RpeError, match='batch norm'):
            model(img, img, grad_encoders=True)
        with pytest.raises(RpeError, match='batch norm'):
            model.check_grad('encoders')
        model.check_grad('corr')                                         # (the depth above does not read the encoders)
        norm.eval()
    model.check_grad('encoders')
    dropped = raft.RAFT(synth.model_config(64, 96)).eval()               # (the encoders here carry no dropout module of their own)
    dropped.fnet.add_module('drop', nn.Dropout2d(0.5).train())
    with pytest.raises(RpeError, match='dropout'):
        dropped(img, img, grad_encoders=True)
    dropped.fnet.drop.eval()
    dropped.check_grad('encoders')
    # everything grad_corr refuses
    for key in ('alternate_corr', 'update_fp16', 'mixed_precision'):
        other = raft.RAFT(dict(synth.model_config(64, 96), **{key: True})).eval()
        with pytest.raises(RpeError, match=key):
            other(img, img, grad_encoders=True)
    with pytest.raises(RpeError, match='upsample'):
        model(img, img, grad_encoders=True, upsample=False)
    with pytest.raises(ValueError, match='stages'):
        model.check_grad('encoder')
    # sources go with the depth, and only with it
    with pytest.raises(RpeError, match='sources'):
        model.grad_pass((f, f), c, stages='encoders')
    with pytest.raises(RpeError, match='sources'):
        model.grad_pass((f, f), c, stages='corr', sources=((img, 0, 1),) * 3)
    with pytest.raises(RpeError, match='source'):
        model.grad_pass((f, f), c, stages='encoders', sources=((img, 0, 1), ((img, img), 0, 2), (img, 0, 1)))


def test_freeze_flow_parts_set_exactly_the_parameters_named(rpe):
    from rpe_amd import pose_net, raft_grad, synth
    net = pose_net.PoseNet(synth.model_config(352, 352)).train().freeze_flow(True)
    assert not net.flow_encoders_trainable()
    ids = lambda params: {id(p) for p in params}
    fnet, cnet = ids(net.flow.fnet.parameters()), ids(net.flow.cnet.parameters())
    assert len(fnet) == 32 and len(cnet) == 62 and ids(raft_grad.encoder_params(net.flow.fnet)) == fnet and ids(raft_grad.encoder_params(net.flow.cnet)) == cnet
    every = ids(net.flow.parameters())
    assert len(every) == 124
    own = [p for k, p in net.named_parameters() if not k.startswith('flow.')]
    for parts, want in (('fnet', fnet), ('cnet', cnet), ('encoders', fnet | cnet), ('raft', every)):
        net.freeze_flow(True).freeze_flow(False, parts=parts)
        assert {id(p) for p in net.flow.parameters() if p.requires_grad} == want, parts
        assert all(p.requires_grad for p in own)
        assert net.flow_encoders_trainable()
        assert net.flow_update_trainable() == net.flow_heads_trainable() == (parts == 'raft')
    net.freeze_flow(True)
    assert not net.flow_encoders_trainable() and not any(p.requires_grad for p in net.flow.parameters())
    # the bare form stays refused, with the message it had, and now names the spelling
    for kw in ({}, dict(parts=None)):
        with pytest.raises(NotImplementedError, match='stop at the flows') as e:
            net.freeze_flow(False, **kw)
        assert 'encoders have no backward' in str(e.value) and "parts='raft'" in str(e.value)
    assert not any(p.requires_grad for p in net.flow.parameters())
    for bad in ('gru', 'encoder', 'all', '', 'flow'):
        with pytest.raises(ValueError, match='parts'):
            net.freeze_flow(False, parts=bad)
    doc = pose_net.PoseNet.freeze_flow.__doc__
    assert 'correlation has a backward' in doc and "parts='raft'" in doc


def test_posenet_refuses_a_training_batch_norm_before_any_launch(rpe):
    from rpe_amd import pose_net, synth
    from rpe_amd._lib import RpeError
    net = pose_net.PoseNet(synth.model_config(352, 352)).train().freeze_flow(True).freeze_flow(False, parts='cnet')
    net.flow.cnet.norm1.train()
    z = torch.zeros(1, 3, 352, 352)
    with pytest.raises(RpeError, match='batch norm'):
        net(z, z, torch.eye(3)[None], torch.ones(1), z, z)
    with pytest.raises(ValueError, match='enc='):
        net.flow2depth(z, z, torch.ones(1), grad='encoders', enc=dict(f=None, c=None))
