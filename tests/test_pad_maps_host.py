"""CPU: the host side of RAFT's ``pad_maps`` (the update loop on zero-padded maps at 1/8 map sizes the tuned kernels refuse): the config
plumbing, the refusal together with the bf16x3 variant, the padded-size rule, the ABI of the valid-extent / pitch entry points (header,
exported symbols, ctypes table, struct sizes on both sides) and their argument checks, which run before anything touches a device."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ('rpe_conv_wino_v', 'rpe_conv_wino24_v', 'rpe_conv_wino1d_v', 'rpe_conv1x1_v', 'rpe_stem_conv_v', 'rpe_conv3x3_to2_flow_v',
       'rpe_corr_lookup_ex', 'rpe_corr_alt_lookup_ex', 'rpe_upsample_convex_ex', 'rpe_copy_rect')


def test_flag_defaults_to_off_and_reaches_the_model(rpe):
    from rpe_amd import pose_net, raft, synth
    cfg = synth.model_config(64, 96)
    assert cfg['pad_maps'] is False and raft.RAFT(cfg).pad_maps is False and raft.PAD_MAPS is False
    assert raft.RAFT({k: v for k, v in cfg.items() if k != 'pad_maps'}).pad_maps is False          # key absent
    on = synth.model_config(64, 96, pad_maps=True)
    assert raft.RAFT(on).pad_maps is True and pose_net.PoseNet(on).flow.pad_maps is True
    assert 'PAD_MAPS' in raft.ROUTE_SWITCHES                                                        # recorded passes and launchers key on it
    # a pass runs on padded maps only where the tuned kernels refuse the 1/8 map
    net = raft.RAFT(on)
    assert net._padded(64, 80) is None and net._padded(45, 45) == (46, 48) and raft.RAFT(cfg)._padded(45, 45) is None


def test_refused_with_the_bf16x3_variant(rpe, monkeypatch):
    from rpe_amd import raft, synth
    on = synth.model_config(64, 96, pad_maps=True)
    monkeypatch.setattr(raft, 'CONV_BF16X3', True)
    with pytest.raises(rpe.RpeError, match='pad_maps'):
        raft.RAFT(on)
    raft.RAFT(synth.model_config(64, 96))                                                           # flag off: the variant is fine
    monkeypatch.setattr(raft, 'CONV_BF16X3', False)
    net = raft.RAFT(on)
    monkeypatch.setattr(raft, 'CONV_BF16X3', True)                                                  # flipped on a live model: refused at the pass
    with pytest.raises(rpe.RpeError, match='pad_maps'):
        net._padded(45, 45)
    monkeypatch.setattr(raft, 'CONV_BF16X3', False)
    monkeypatch.setattr(raft, 'WINOGRAD', False)
    with pytest.raises(rpe.RpeError, match='pad_maps'):
        raft.RAFT(on)


def test_padded_size_rule(rpe):
    """Rows up to an even count, row length up to a multiple of 4; the identity on sizes the tuned kernels take."""
    from rpe_amd import ops, raft
    assert raft.padded_size(11, 13) == (12, 16) and raft.padded_size(45, 44) == (46, 44) and raft.padded_size(135, 240) == (136, 240)
    assert raft.padded_size(45, 45) == (46, 48) and raft.padded_size(72, 90) == (72, 92) and raft.padded_size(43, 50) == (44, 52)
    import torch
    w3 = torch.zeros(8, 8, 3, 3)
    for h8 in range(2, 70):
        for w8 in range(4, 70):
            hp, wp = raft.padded_size(h8, w8)
            assert h8 <= hp <= h8 + 1 and w8 <= wp <= w8 + 3
            assert ops.PackedWino24.supported(w3, hp, wp) and ops.PackedWino1d.supported(torch.zeros(8, 8, 1, 5), wp) and ops.PackedConv1x1.supported(hp, wp)
            if ops.PackedWino24.supported(w3, h8, w8):
                assert (hp, wp) == (h8, w8)


def test_abi_of_the_new_entry_points(rpe):
    from rpe_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rpe.h')).read(), flags=re.S)
    L = rpe.lib()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SIGNATURES and name in _lib.KIND_OF_ENTRY and hasattr(L, name), name
        kind = _lib.KIND_OF_ENTRY[name]
        assert re.search(r'#define RPE_OP_[A-Z0-9_]+ %d\b' % kind, text), name                      # the kind's number in the header
    sizes = {'rpe_conv_desc_v': (_lib.ConvDescV, 208), 'rpe_corr_lookup_ex_args': (_lib.CorrLookupExArgs, 56),
             'rpe_corr_alt_lookup_ex_args': (_lib.CorrAltLookupExArgs, 56), 'rpe_stem_conv_v_args': (_lib.StemConvVArgs, 104),
             'rpe_flow_update_v_args': (_lib.FlowUpdateVArgs, 104), 'rpe_upsample_convex_ex_args': (_lib.UpsampleConvexExArgs, 48),
             'rpe_copy_rect_args': (_lib.CopyRectArgs, 80)}
    src = open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'oplist.hip')).read()
    for cname, (mirror, size) in sizes.items():
        assert ctypes.sizeof(mirror) == size and f'static_assert(sizeof({cname}) == {size},' in src, cname
    assert _lib.ConvDescV.h_valid.offset == 200 and issubclass(_lib.ConvDescV, _lib.ConvDesc)
    names = [n for n, _ in _lib.struct_fields(_lib.ConvDescV())]
    assert names[:2] == ['x', 'x_batch_stride'] and names[-2:] == ['h_valid', 'w_valid'] and len(names) == len(_lib.ConvDesc._fields_) + 2


def test_bad_extents_and_null_pointers_return_badarg(rpe):
    from rpe_amd import _lib
    L = rpe.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)                     # never dereferenced: the checks fail first
    for entry, (kh, kw) in (('rpe_conv_wino_v', (3, 3)), ('rpe_conv_wino24_v', (3, 3)), ('rpe_conv_wino1d_v', (1, 5)), ('rpe_conv1x1_v', (1, 1))):
        fn = getattr(L, entry)
        assert fn(None, null) == -1, entry
        for hv, wv in ((13, 16), (12, 17), (0, 16), (12, -1)):
            d = _lib.ConvDescV(x=16, packed=16, out=16, b=1, cin=16, cout=16, h=12, w=16, kh=kh, kw=kw, mode=0, h_valid=hv, w_valid=wv)
            assert fn(ctypes.byref(d), null) == -1, (entry, hv, wv)
        d = _lib.ConvDescV(x=0, packed=16, out=16, b=1, cin=16, cout=16, h=12, w=16, kh=kh, kw=kw, mode=0, h_valid=11, w_valid=13)
        assert fn(ctypes.byref(d), null) == -1, entry                         # null input
    # a valid extent with an epilogue the _v form does not have -> unsupported, not a launch
    d = _lib.ConvDescV(x=16, packed=16, out=16, scale=16, b=1, cin=16, cout=16, h=12, w=16, kh=3, kw=3, mode=0, h_valid=11, w_valid=13)
    assert L.rpe_conv_wino_v(ctypes.byref(d), null) == -3 and L.rpe_conv_wino24_v(ctypes.byref(d), null) == -3
    stem = lambda img, hv, wv: L.rpe_stem_conv_v(img, 1, 2, 12, 16, 1, 1.0, 1.0, 0.0, one, 128, null, null, 1, one, null, hv, wv, null)
    assert stem(one, 13, 16) == -1 and stem(one, 12, 17) == -1 and stem(one, 0, 4) == -1 and stem(null, 11, 13) == -1
    flow = lambda x, hv, wv: L.rpe_conv3x3_to2_flow_v(x, one, null, 1, 256, 12, 16, one, one, null, null, 0, null, 0, hv, wv, null)
    assert flow(one, 13, 16) == -1 and flow(one, 12, 17) == -1 and flow(null, 11, 13) == -1
    assert L.rpe_corr_lookup_ex(one, one, 1, 17, 18, 4, 4, 16, 20, one, null) == -1 and L.rpe_corr_lookup_ex(one, one, 1, 17, 18, 4, 4, 18, 17, one, null) == -1
    assert L.rpe_corr_lookup_ex(null, one, 1, 17, 18, 4, 4, 18, 20, one, null) == -1
    assert L.rpe_corr_alt_lookup_ex(one, one, 1, 256, 17, 18, 4, 4, 16, 20, one, null) == -1 and L.rpe_corr_alt_lookup_ex(null, one, 1, 256, 17, 18, 4, 4, 18, 20, one, null) == -1
    assert L.rpe_upsample_convex_ex(one, one, 1, 17, 18, 16, 20, one, null) == -1 and L.rpe_upsample_convex_ex(one, null, 1, 17, 18, 18, 20, one, null) == -1
    assert L.rpe_copy_rect(one, 100, 20, 3, one, 100, 20, 4, 1, 1, 4, 4, null) == -1          # pitch below the rectangle's width
    assert L.rpe_copy_rect(one, 100, 15, 4, one, 100, 20, 4, 1, 1, 4, 4, null) == -1          # plane below (h - 1) pitch + w
    assert L.rpe_copy_rect(null, 100, 20, 4, one, 100, 20, 4, 1, 1, 4, 4, null) == -1
    # the old entry points keep their rules
    assert L.rpe_corr_lookup(one, one, 1, 8, 8, 4, 3, one, null) == -1 and L.rpe_upsample_convex(null, one, 1, 8, 8, one, null) == -1


def test_wrappers_check_the_extent_before_the_library(rpe, monkeypatch):
    from rpe_amd import ops
    with pytest.raises(rpe.RpeError, match='valid extent'):
        ops._valid_extent('x', (13, 16), 12, 16)
    assert ops._valid_extent('x', (11, 13), 12, 16) == (11, 13)
    with pytest.raises(rpe.RpeError, match='no valid-extent form'):
        ops._kind('rpe_conv_fused', (1, 1))
    assert ops._kind('rpe_conv_wino1d', (1, 1)) == rpe._lib.OP_CONV_WINO1D_V and ops._kind('rpe_conv_wino1d', None) == rpe._lib.OP_CONV_WINO1D
