"""CPU: the host side of RAFT's ``pad_encoders`` (both encoders' layer2, layer3 and output layer on zero-padded maps at image sizes whose
1/8 map the tuned kernels refuse): the config plumbing, the refusals, the ABI of the encoders' valid-extent entry points (header, exported
symbols, ctypes tables, kind numbers, struct sizes on both sides) and their argument checks, which run before anything touches a device."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

CONVS = ('rpe_enc_conv_wino_v', 'rpe_enc_conv_wino24_v', 'rpe_enc_conv_s2_v', 'rpe_enc_conv_s2_m96_v')
NEW = CONVS + ('rpe_instnorm_apply_v',)


def test_flag_defaults_to_off_and_reaches_the_model(rpe):
    from rpe_amd import pose_net, raft, synth
    cfg = synth.model_config(64, 96)
    net = raft.RAFT(cfg)
    assert cfg['pad_encoders'] is False and net.pad_encoders is False and raft.PAD_ENCODERS is False
    assert net.fnet.pad_encoders is False and net.cnet.pad_encoders is False
    assert raft.RAFT({k: v for k, v in cfg.items() if k != 'pad_encoders'}).pad_encoders is False      # key absent
    on = synth.model_config(64, 96, pad_encoders=True)
    assert on['pad_maps'] is False                                                                     # a switch of its own
    net = raft.RAFT(on)
    assert net.pad_encoders is True and net.fnet.pad_encoders is True and net.cnet.pad_encoders is True and net.pad_maps is False
    assert pose_net.PoseNet(on).flow.fnet.pad_encoders is True
    assert 'PAD_ENCODERS' in raft.ROUTE_SWITCHES and len(raft._switches()) == len(raft.ROUTE_SWITCHES)
    # an encoder pass runs on padded maps only where the tuned kernels refuse the 1/8 map (the predicate of RAFT._padded)
    assert net.fnet._padded(512, 640) is None and net.fnet._padded(360, 360) == (46, 48) and net.fnet._padded(88, 96) == (12, 12)
    assert raft.RAFT(cfg).fnet._padded(360, 360) is None
    assert raft.RAFT(synth.model_config(64, 96, pad_maps=True)).fnet._padded(360, 360) is None         # pad_maps alone leaves the encoders alone


def test_module_switch_does_what_the_key_does(rpe, monkeypatch):
    from rpe_amd import raft, synth
    net = raft.RAFT(synth.model_config(64, 96))
    monkeypatch.setattr(raft, 'PAD_ENCODERS', True)
    assert net.cnet._padded(360, 360) == (46, 48) and net.cnet._padded(512, 640) is None


def test_refusals(rpe, monkeypatch):
    from rpe_amd import raft, synth
    on = synth.model_config(64, 96, pad_encoders=True)
    monkeypatch.setattr(raft, 'CONV_BF16X3', True)
    with pytest.raises(rpe.RpeError, match='pad_encoders'):
        raft.RAFT(on)
    raft.RAFT(synth.model_config(64, 96))                                                              # flag off: the variant is fine
    monkeypatch.setattr(raft, 'CONV_BF16X3', False)
    net = raft.RAFT(on)
    monkeypatch.setattr(raft, 'CONV_BF16X3', True)                                                     # flipped on a live model: refused at the pass
    with pytest.raises(rpe.RpeError, match='pad_encoders'):
        net.fnet._padded(360, 360)
    with pytest.raises(rpe.RpeError, match='pad_encoders'):
        net.encode_features(None)
    with pytest.raises(rpe.RpeError, match='pad_encoders'):
        net.encode_context(None)
    monkeypatch.setattr(raft, 'CONV_BF16X3', False)
    monkeypatch.setattr(raft, 'WINOGRAD', False)
    with pytest.raises(rpe.RpeError, match='pad_encoders'):
        raft.RAFT(on)
    with pytest.raises(rpe.RpeError, match='pad_encoders'):
        net.cnet._padded(360, 360)


def test_abi_of_the_new_entry_points(rpe):
    from rpe_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rpe.h')).read(), flags=re.S)
    L = rpe.lib()
    assert L.rpe_abi_minor() == 4 and re.search(r'#define RPE_ABI_MINOR 4\b', text)
    kinds = set()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SIGNATURES and name in _lib.KIND_OF_ENTRY and hasattr(L, name), name
        kind = _lib.KIND_OF_ENTRY[name]
        kinds.add(kind)
        assert kind > _lib.OP_STREAM_WAIT and _lib.ALL_LIST_OPS[kind][0] == name                      # behind the event ops, names distinct
        assert re.search(r'#define RPE_OP_[A-Z0-9_]+ %d\b' % kind, text), name                        # the kind's number in the header
        assert getattr(L, name).argtypes[-1] is ctypes.c_void_p
    assert len(kinds) == len(NEW) and not kinds & set(_lib.LIST_OPS)
    for name in CONVS:                                                                                  # struct rpe_conv_desc_v, reused
        assert list(getattr(L, name).argtypes) == [ctypes.POINTER(_lib.ConvDesc), ctypes.c_void_p]
    assert set(_lib.ENC_FORM.values()) == set(CONVS) and all(k in _lib.KIND_OF_ENTRY for k in _lib.ENC_FORM)
    src = open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'oplist.hip')).read()
    assert ctypes.sizeof(_lib.ConvDescV) == 208 and 'static_assert(sizeof(rpe_conv_desc_v) == 208,' in src
    assert ctypes.sizeof(_lib.InstnormApplyVArgs) == 72 and 'static_assert(sizeof(rpe_instnorm_apply_v_args) == 72,' in src
    assert list(L.rpe_instnorm_apply_v.argtypes) == [t for _, t in _lib.InstnormApplyVArgs._fields_] + [ctypes.c_void_p]
    params = re.search(r'\brpe_instnorm_apply_v\s*\(([^)]*)\)\s*;', text).group(1)
    assert len(params.split(',')) == len(_lib.InstnormApplyVArgs._fields_) + 1
    for name in NEW:                                                                                    # every kind has its case in run_one
        assert re.search(r'case RPE_OP_[A-Z0-9_]+: .*\b%s\(' % name, src) or re.search(r'return %s\(' % name, src), name


def _desc(_lib, **kw):
    base = dict(x=16, packed=16, out=16, b=1, cin=16, cout=16, h=12, w=16, kh=3, kw=3, mode=0, h_valid=11, w_valid=13)
    base.update(kw)
    return _lib.ConvDescV(**base)


def test_bad_extents_and_null_pointers_return_badarg(rpe):
    from rpe_amd import _lib
    L = rpe.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)                     # never dereferenced: the checks fail first
    for entry in ('rpe_enc_conv_wino_v', 'rpe_enc_conv_wino24_v'):
        fn = getattr(L, entry)
        assert fn(None, null) == -1, entry
        for hv, wv in ((13, 16), (12, 17), (0, 16), (12, -1)):
            assert fn(ctypes.byref(_desc(_lib, h_valid=hv, w_valid=wv)), null) == -1, (entry, hv, wv)
        for field in ('x', 'packed', 'out'):
            assert fn(ctypes.byref(_desc(_lib, **{field: 0})), null) == -1, (entry, field)
    for entry in ('rpe_enc_conv_s2_v', 'rpe_enc_conv_s2_m96_v'):              # the extent lies on the OUTPUT map: (6, 8) here
        fn = getattr(L, entry)
        assert fn(None, null) == -1, entry
        for hv, wv in ((7, 8), (6, 9), (0, 8), (6, -1)):
            assert fn(ctypes.byref(_desc(_lib, stride=2, h_valid=hv, w_valid=wv)), null) == -1, (entry, hv, wv)
        for field in ('x', 'packed', 'out'):
            assert fn(ctypes.byref(_desc(_lib, stride=2, h_valid=5, w_valid=7, **{field: 0})), null) == -1, (entry, field)
    ina = lambda x, mi, out, hv, wv, res=null, rmi=null, w=16: L.rpe_instnorm_apply_v(x, mi, 1, 4, 12, w, hv, wv, 1, res, rmi, out, null)
    assert ina(one, one, one, 13, 16) == -1 and ina(one, one, one, 12, 17) == -1 and ina(one, one, one, 0, 4) == -1 and ina(one, one, one, 3, -2) == -1
    assert ina(null, one, one, 11, 13) == -1 and ina(one, null, one, 11, 13) == -1 and ina(one, one, null, 11, 13) == -1
    assert ina(one, one, one, 11, 13, rmi=one) == -1                        # the residual's moments without a residual


def test_unsupported_fields_return_unsupported(rpe):
    from rpe_amd import _lib
    L = rpe.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    for entry in ('rpe_enc_conv_wino_v', 'rpe_enc_conv_wino24_v'):
        fn = getattr(L, entry)
        assert fn(ctypes.byref(_desc(_lib, mode=2)), null) == -3, entry                       # a GRU gate mode
        assert fn(ctypes.byref(_desc(_lib, add=16)), null) == -3, entry                       # a GRU operand
        assert fn(ctypes.byref(_desc(_lib, stride=2)), null) == -3, entry
        assert fn(ctypes.byref(_desc(_lib, kh=1, kw=5)), null) == -3, entry
        assert fn(ctypes.byref(_desc(_lib, pre_norm=16, cin=256)), null) == -3, entry         # no LDS room for the pairs
        assert fn(ctypes.byref(_desc(_lib, out=8)), null) == -3, entry                        # the valid-extent stores are 16-byte ones
    assert L.rpe_enc_conv_wino_v(ctypes.byref(_desc(_lib, h=12, w=18, h_valid=11, w_valid=17)), null) == -3   # rows that are not whole quads
    for entry in ('rpe_enc_conv_s2_v', 'rpe_enc_conv_s2_m96_v'):
        fn = getattr(L, entry)
        s2 = dict(stride=2, h_valid=5, w_valid=7)
        assert fn(ctypes.byref(_desc(_lib, **dict(s2, stride=1))), null) == -3, entry         # stride 2 only
        assert fn(ctypes.byref(_desc(_lib, residual=16, **s2)), null) == -3, entry
        assert fn(ctypes.byref(_desc(_lib, pre_norm=16, **s2)), null) == -3, entry
        assert fn(ctypes.byref(_desc(_lib, out2=16, **s2)), null) == -3, entry
        assert fn(ctypes.byref(_desc(_lib, mode=4, **s2)), null) == -3, entry                 # TANH
        assert fn(ctypes.byref(_desc(_lib, kh=5, kw=5, **s2)), null) == -3, entry
    ina = lambda x, w, relu=1: L.rpe_instnorm_apply_v(x, one, 1, 4, 12, w, 11, 13, relu, null, null, one, null)
    assert ina(one, 18) == -3 and ina(ctypes.c_void_p(20), 16) == -3 and ina(one, 16, relu=4) == -3
    # the update loop's entry points keep their rules (tests/test_pad_maps_host.py): an encoder epilogue there stays unsupported
    assert L.rpe_conv_wino_v(ctypes.byref(_desc(_lib, scale=16)), null) == -3 and L.rpe_conv_wino24_v(ctypes.byref(_desc(_lib, stats=16)), null) == -3


def test_wrappers_route_to_the_encoder_forms(rpe):
    from rpe_amd import _lib, ops
    assert ops._kind('rpe_conv_wino', (1, 1), True) == _lib.OP_ENC_CONV_WINO_V and ops._kind('rpe_conv_wino24', (1, 1), True) == _lib.OP_ENC_CONV_WINO24_V
    assert ops._kind('rpe_conv_fused', (1, 1), True) == _lib.OP_ENC_CONV_S2_V and ops._kind('rpe_conv_fused_m96', (1, 1), True) == _lib.OP_ENC_CONV_S2_M96_V
    assert ops._kind('rpe_conv_wino', (1, 1)) == _lib.OP_CONV_WINO_V and ops._kind('rpe_conv_wino', None, True) == _lib.OP_CONV_WINO
    with pytest.raises(rpe.RpeError, match='no encoder valid-extent form'):
        ops._kind('rpe_conv_wino1d', (1, 1), True)
    with pytest.raises(rpe.RpeError, match='no valid-extent form'):
        ops._kind('rpe_conv_fused', (1, 1))
