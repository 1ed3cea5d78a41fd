"""CPU: the weight-derived caches of raft.py (_cached / wkey / _switches) with a stand-in for raft.ops whose packing classes count their
constructions and need no library: nothing is rebuilt while nothing changes, a changed weight rebuilds exactly what was made from it, and
every route switch invalidates the update block's packings."""
import collections
import re
import types

import pytest
import torch
import torch.nn as nn

PACKINGS = ('PackedConv', 'PackedWino', 'PackedWino24', 'PackedWinoX3', 'PackedWino1d', 'PackedWino1dX3', 'PackedStem', 'PackedLookupConv', 'Conv1x1')


def _fake_ops(made):
    class Counted:
        def __init__(self, *a, **k):
            made[type(self).__name__] += 1

        supported = staticmethod(lambda *a: True)

        def __call__(self, x, mode, out, **k):
            return out
    fake = types.SimpleNamespace(CONV_LINEAR=0, CONV_RELU=1, CONV_GATE_ZR=2, CONV_GATE_H=3, CONV_TANH=4,
                                 conv_direct=lambda x, w, b, stride, padding, relu=False: torch.zeros(x.shape[0], w.shape[0], *x.shape[2:]))
    for name in PACKINGS:
        setattr(fake, name, type(name, (Counted,), {}))
    return fake


@pytest.fixture()
def live(rpe, monkeypatch):
    """(raft module, a RAFT on the CPU, the construction counter, touch() = one evaluation of every cache under test)."""
    from rpe_amd import raft
    made = collections.Counter()
    monkeypatch.setattr(raft, 'ops', _fake_ops(made))
    torch.manual_seed(0)
    model = raft.RAFT({}).eval()
    ub, cnet = model.update_block, model.cnet

    def touch():
        ub.gate_weights()
        ub.packed_convs(8)
        ub.up_mask(torch.zeros(1, 128, 4, 8))
        raft._bn_affine(cnet.conv1, cnet.norm1)
        cnet._final(torch.zeros(1, 128, 4, 8), True)
        return {'stacked': ub.__dict__['_stacked'], 'packed': ub.__dict__['_packed'], 'mask': ub.__dict__['_mask_packed'],
                'affine': cnet.norm1.__dict__['_rpe_affine'], 'final': cnet.__dict__['_final_packed']}
    return raft, model, made, touch


def _rebuilt(before, after):
    return {k for k in before if after[k] is not before[k]}


def test_nothing_is_rebuilt_while_nothing_changes(live):
    raft, model, made, touch = live
    first = touch()
    assert made['Conv1x1'] == 4 and made['PackedStem'] == 1 and made['PackedConv'] == 5 and made['PackedWino1d'] == 8, dict(made)
    count = dict(made)
    for _ in range(3):
        assert _rebuilt(first, touch()) == set() and dict(made) == count


# (what is changed, the caches made from it): the packed convolutions hold the stacked gate weights, so they follow them
DEPENDANTS = [(lambda m: m.update_block.gru.convz1, 'weight', {'stacked', 'packed'}),
              (lambda m: m.update_block.gru.convq2, 'bias', {'stacked', 'packed'}),
              (lambda m: m.update_block.encoder.convc2, 'weight', {'packed'}),
              (lambda m: m.update_block.encoder.convf1, 'bias', {'packed'}),
              (lambda m: m.update_block.mask[0], 'weight', {'mask'}),
              (lambda m: m.update_block.mask[2], 'bias', {'mask'}),
              (lambda m: m.cnet.conv2, 'bias', {'final'}),
              (lambda m: m.cnet.norm1, 'running_var', {'affine'}),
              (lambda m: m.cnet.conv1, 'bias', {'affine'}),
              (lambda m: m.fnet.conv2, 'weight', set())]


def _in_place(mod, name):
    with torch.no_grad():
        getattr(mod, name).mul_(1.5)


def _replace(mod, name):
    t = getattr(mod, name)
    setattr(mod, name, nn.Parameter(t.detach().clone()) if isinstance(t, nn.Parameter) else t.clone())


def _round_trip(mod, name):
    held = [t.data for t in list(mod.parameters()) + list(mod.buffers())]      # (held by the caller: the allocator may otherwise hand the
    mod.double().float()                                                        # same addresses back, and an equal copy there IS the old weight)
    return held


@pytest.mark.parametrize('change', [_in_place, _replace, _round_trip])
@pytest.mark.parametrize('case', range(len(DEPENDANTS)))
def test_a_changed_weight_rebuilds_exactly_its_dependants(live, change, case):
    raft, model, made, touch = live
    pick, name, want = DEPENDANTS[case]
    before = touch()
    held = change(pick(model), name)
    after = touch()
    assert _rebuilt(before, after) == want
    assert _rebuilt(after, touch()) == set()
    del held


def test_a_whole_model_round_trip_rebuilds_everything(live):
    raft, model, made, touch = live
    before = touch()
    held = _round_trip(model, None)
    assert _rebuilt(before, touch()) == set(before)
    del held


def test_every_route_switch_is_in_the_snapshot_and_invalidates_the_packings(live, monkeypatch):
    raft, model, made, touch = live
    need = {'WINOGRAD', 'WINO_2X4', 'S2_M96', 'S2_M96_MIN_WGS', 'CORR_BF16X3', 'CONV_BF16X3', 'X3_MIN_CIN', 'X3_GRU', 'SIDE_STREAM', 'SIDE_STREAM_MAX',
            'LOOKUP_FUSED', 'LOOKUP_FUSED_MAX_WGS', 'ENC_STREAMS', 'ENC_STREAMS_MIN'}
    assert need <= set(raft.ROUTE_SWITCHES) and len(raft._switches()) == len(raft.ROUTE_SWITCHES)
    for name in raft.ROUTE_SWITCHES:
        before, snap = touch(), raft._switches()
        value = getattr(raft, name)
        monkeypatch.setattr(raft, name, (not value) if isinstance(value, bool) else value + 1)
        assert raft._switches() != snap, name
        after = touch()
        assert {'packed', 'mask'} <= _rebuilt(before, after) and 'stacked' not in _rebuilt(before, after), name
        assert _rebuilt(after, touch()) == set(), name


def test_winograd_off_on_a_live_model_leaves_no_winograd_packing(live, monkeypatch):
    raft, model, made, touch = live
    touch()
    monkeypatch.setattr(raft, 'WINOGRAD', False)
    P = model.update_block.packed_convs(8)
    assert P['wino'] == {} and P['wino24'] == {} and type(P['zr1']).__name__ == 'PackedConv'


def test_no_key_is_an_object_identity(rpe):
    from rpe_amd import raft
    assert not re.search(r'\bid\(', open(raft.__file__).read())
