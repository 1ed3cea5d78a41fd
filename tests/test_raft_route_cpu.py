"""CPU: raft.Route, the resolved description of a RAFT pass (raft.resolve_route / RAFT._route): the refusal table over every combination
of the six config keys and the module switches the refusals read, refusals and instance flags on a live model, the sized facts (the loop's
and the encoders' padded maps, the fused route) and its behaviour as a part of cache keys."""
import collections
import itertools

import pytest
import torch.nn as nn

from test_raft_caches_cpu import _fake_ops

KEYS = ('mixed_precision', 'alternate_corr', 'alt_corr_fp16', 'pad_maps', 'pad_encoders', 'update_fp16')
# (switch, its value when "on" for the table = the value that is not the default)
SWITCHES = (('CONV_BF16X3', True), ('CORR_BF16X3', True), ('WINOGRAD', False), ('PAD_MAPS', True), ('PAD_ENCODERS', True), ('UPDATE_FP16', True))


def refused(cfg, sw):
    """The rules as raft.py states them, in its words:
      * alt_corr_fp16 needs alternate_corr; alternate_corr is f32 only -- not with mixed_precision, CORR_BF16X3 or CONV_BF16X3
      * pad_maps / pad_encoders (key or switch) run on the f32 Winograd kernels -- not with CONV_BF16X3, not without WINOGRAD
      * update_fp16 (key or switch): not with CONV_BF16X3, not without WINOGRAD, not with pad_maps / pad_encoders (key or switch)"""
    mp, alt, alt16 = cfg['mixed_precision'], cfg['alternate_corr'], cfg['alt_corr_fp16']
    pm, pe, uf = cfg['pad_maps'] or sw['PAD_MAPS'], cfg['pad_encoders'] or sw['PAD_ENCODERS'], cfg['update_fp16'] or sw['UPDATE_FP16']
    x3, wino = sw['CONV_BF16X3'], sw['WINOGRAD']
    return bool((alt16 and not alt) or (alt and (mp or sw['CORR_BF16X3'] or x3)) or ((pm or pe) and (x3 or not wino))
                or (uf and (x3 or not wino or pm or pe)))


class _UpdateBlock(nn.Module):
    route = ()


def test_refusal_table_over_every_combination(rpe, monkeypatch):
    """2^6 configs x 2^6 switch settings; the submodules are stand-ins (the table is about RAFT.__init__'s refusals, and 4096 real
    encoders would take minutes to initialise)."""
    from rpe_amd import raft
    monkeypatch.setattr(raft, 'BasicEncoder', lambda *a, **k: nn.Module())
    monkeypatch.setattr(raft, 'BasicUpdateBlock', lambda *a, **k: _UpdateBlock())
    seen = collections.Counter()
    for sw_bits in itertools.product((False, True), repeat=len(SWITCHES)):
        sw = {}
        for (name, on), bit in zip(SWITCHES, sw_bits):
            sw[name] = on if bit else not on
            monkeypatch.setattr(raft, name, sw[name])
        for bits in itertools.product((False, True), repeat=len(KEYS)):
            cfg = dict(zip(KEYS, bits))
            try:
                raft.RAFT(dict(cfg))
                got = False
            except rpe.RpeError:
                got = True
            assert got == refused(cfg, sw), (cfg, sw)
            seen[got] += 1
    assert seen[True] + seen[False] == 4096 and seen[True] > 0 and seen[False] > 0


# one case per option: (config that is fine, what is flipped or assigned on the live model, a word of the refusal)
LIVE = [(dict(alternate_corr=True), ('switch', 'CORR_BF16X3', True), 'alternate_corr'),
        (dict(alternate_corr=True), ('flag', 'mixed_precision', True), 'alternate_corr'),
        (dict(), ('flag', 'alt_corr_fp16', True), 'alt_corr_fp16'),
        (dict(pad_maps=True), ('switch', 'CONV_BF16X3', True), 'pad_maps'),
        (dict(pad_encoders=True), ('switch', 'WINOGRAD', False), 'pad_encoders'),
        (dict(update_fp16=True), ('switch', 'PAD_MAPS', True), 'valid-extent')]


@pytest.mark.parametrize('cfg,change,word', LIVE)
def test_a_live_model_is_refused_at_the_next_resolution(rpe, monkeypatch, cfg, change, word):
    from rpe_amd import raft
    net = raft.RAFT(cfg)
    net._route(), net._route(map_size=(16, 20)), net._route(image_size=(128, 160))
    kind, name, value = change
    if kind == 'switch':
        monkeypatch.setattr(raft, name, value)
    else:
        setattr(net, name, value)
    for kw in (dict(), dict(map_size=(16, 20)), dict(image_size=(128, 160))):
        with pytest.raises(rpe.RpeError, match=word):
            net._route(**kw)
    with pytest.raises(rpe.RpeError, match=word):
        net.encode_features(None)
    with pytest.raises(rpe.RpeError, match=word):
        net.encode_context(None)
    with pytest.raises(rpe.RpeError, match=word):
        net(None, None, fmaps=(_Shaped(1, 256, 16, 20),) * 2)                 # refused before anything of the pass is touched


class _Shaped:
    """What RAFT.forward reads of its encoder outputs in front of the resolution: a shape and a device."""
    def __init__(self, *shape):
        self.shape, self.device = shape, 'cpu'


@pytest.mark.parametrize('key', KEYS)
def test_an_assigned_instance_flag_is_honoured_at_the_next_resolution(rpe, key):
    from rpe_amd import raft
    base = dict(alternate_corr=True) if key == 'alt_corr_fp16' else {}
    net = raft.RAFT(base)
    assert getattr(net._route(), key) is False
    setattr(net, key, True)
    assert getattr(net._route(), key) is True and getattr(net._route(map_size=(16, 20)), key) is True
    setattr(net, key, False)
    assert getattr(net._route(), key) is False


@pytest.mark.parametrize('switch,key', [('PAD_MAPS', 'pad_maps'), ('PAD_ENCODERS', 'pad_encoders'), ('UPDATE_FP16', 'update_fp16')])
def test_a_module_switch_does_what_the_key_does(rpe, monkeypatch, switch, key):
    from rpe_amd import raft
    net = raft.RAFT({})
    size = (128, 160) if key == 'update_fp16' else (360, 360)               # (a 45-wide map is refused under update_fp16, as it should be)
    off = net._route(image_size=size)
    monkeypatch.setattr(raft, switch, True)
    if key == 'update_fp16':                                                  # the update block of a model built under the switch sees it,
        assert raft.RAFT({}).update_block.fp16() and not net.update_block.fp16()
    assert getattr(net._route(), key) is True and net._route(image_size=size) != off
    assert net._route(image_size=size) == raft.RAFT({key: True})._route(image_size=size)
    if key == 'update_fp16':                                                  # ... that of a live one from its next pass on
        assert net.update_block.fp16() and net.update_block.update_fp16 is True


MAPS = [(64, 80), (45, 45), (45, 44), (11, 13)]
IMAGES = [(512, 640), (360, 360), (88, 96)]


def _want_pad(on, h8, w8):
    """RAFT._padded / BasicEncoder._padded as they were: padded_size of the 1/8 map under the option, None where that is the map itself."""
    hp, wp = h8 + (h8 & 1), (w8 + 3) // 4 * 4
    return (hp, wp) if on and (hp, wp) != (h8, w8) else None


@pytest.mark.parametrize('pad_maps', [False, True])
@pytest.mark.parametrize('pad_encoders', [False, True])
def test_sized_facts(rpe, monkeypatch, pad_maps, pad_encoders):
    from rpe_amd import raft
    assert raft.padded_size(45, 45) == (46, 48) and raft.padded_size(64, 80) == (64, 80) and raft.padded_size(11, 13) == (12, 16)
    net = raft.RAFT(dict(pad_maps=pad_maps, pad_encoders=pad_encoders))
    monkeypatch.setattr(raft, 'ops', _fake_ops(collections.Counter()))
    assert net._route().loop_pad is None and net._route().enc_pad is None and net._route().fused is None
    for h8, w8 in MAPS:
        r = net._route(map_size=(h8, w8))
        assert r.loop_pad == _want_pad(pad_maps, h8, w8) == net._padded(h8, w8) and r.enc_pad is None
        loop_w = w8 if r.loop_pad is None else r.loop_pad[1]
        assert r.fused is (loop_w % 4 == 0) and r.fused is (net.update_block.packed_convs(loop_w) is not None)
    for H, W in IMAGES:
        r = net._route(image_size=(H, W))
        h8, w8 = H // 8, W // 8
        assert r.loop_pad == _want_pad(pad_maps, h8, w8) == net._padded(h8, w8)
        assert r.enc_pad == _want_pad(pad_encoders, h8, w8) == net.fnet._padded(H, W) == net.cnet._padded(H, W)
        loop_w = w8 if r.loop_pad is None else r.loop_pad[1]
        assert r.fused is (loop_w % 4 == 0) and r.fused is (net.update_block.packed_convs(loop_w) is not None)
        assert r == net._route(image_size=(H, W)) and r._replace(enc_pad=None) == net._route(map_size=(h8, w8))
    assert net._route(image_size=(364, 360)).enc_pad is None                 # no whole number of 8x8 cells: the encoders stay as they are
    # fixed expectations, so that the rule above cannot drift with the code
    if pad_maps:
        assert net._route(map_size=(45, 45)).loop_pad == (46, 48) and net._route(map_size=(45, 44)).loop_pad == (46, 44)
        assert net._route(map_size=(11, 13)).loop_pad == (12, 16) and net._route(map_size=(64, 80)).loop_pad is None
        assert net._route(map_size=(11, 13)).fused is True
    else:
        assert net._route(map_size=(45, 45)).fused is False and net._route(map_size=(11, 13)).fused is False
        assert net._route(map_size=(45, 44)).fused is True
    if pad_encoders:
        assert net._route(image_size=(360, 360)).enc_pad == (46, 48) and net._route(image_size=(88, 96)).enc_pad == (12, 12)
        assert net._route(image_size=(512, 640)).enc_pad is None


def test_update_fp16_needs_whole_quads(rpe):
    from rpe_amd import raft
    net = raft.RAFT(dict(update_fp16=True))
    assert net._route(map_size=(15, 20)).fused is True and net._route(image_size=(120, 160)).fused is True
    for kw in (dict(map_size=(15, 19)), dict(image_size=(120, 152))):
        with pytest.raises(rpe.RpeError, match='w8 = 19'):
            net._route(**kw)
    assert raft.RAFT({})._route(map_size=(15, 19)).fused is False            # flag off: the generic route


def test_hashable_equal_for_equal_inputs_and_every_option_changes_it(rpe):
    from rpe_amd import raft
    assert raft.Route._fields[:6] == KEYS
    base = dict(alternate_corr=True)
    a, b = raft.RAFT(base)._route(map_size=(45, 45)), raft.RAFT(dict(base))._route(map_size=(45, 45))
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1 and {a: 1}[b] == 1
    assert a.options == a.options.options == raft.RAFT(base)._route() and a.options != a and hash(a.options) == hash(b.options)
    seen = {a.options}
    for key in KEYS:
        if key == 'alternate_corr':
            cfg = {}
        elif key == 'mixed_precision':
            cfg = dict(mixed_precision=True)                                  # (refused beside alternate_corr)
        else:
            cfg = dict(base, **{key: True})
        r = raft.RAFT(cfg)._route()
        assert r not in seen and hash(r) is not None, key
        assert (1, 'a key', r) != (1, 'a key', a.options)                     # ... and so does every key that contains it
        seen.add(r)
    assert len(seen) == len(KEYS) + 1
