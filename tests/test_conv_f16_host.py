"""CPU: the host side of RAFT's ``update_fp16`` (the update block's convolutions with fp16 operands, rpe_conv_f16) -- the config key and its
pass-through, the module switch, the refused combinations, the entry points' argument checks (they return before anything is launched),
and the helper oracle of tests/conv_f16_ref.py: which modules it wraps, that it moves the flow, and that wrapping is idempotent."""
import ctypes
import os
import re

import pytest
import torch

import conv_f16_ref as ref
from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, 'include', 'rpe.h')).read()


def test_config_key_and_module_switch(rpe):
    from rpe_amd import pose_net, raft, synth
    cfg = synth.model_config(64, 96, update_fp16=True)
    assert cfg['update_fp16'] is True and synth.model_config(64, 96)['update_fp16'] is False
    net = raft.RAFT(cfg)
    assert net.update_fp16 is True and net.update_block.update_fp16 is True and net.update_block.fp16()
    off = raft.RAFT(synth.model_config(64, 96))
    assert off.update_fp16 is False and off.update_block.update_fp16 is False and not off.update_block.fp16()
    assert raft.RAFT({}).update_fp16 is False
    assert 'UPDATE_FP16' in raft.ROUTE_SWITCHES and raft.UPDATE_FP16 is False and len(raft._switches()) == len(raft.ROUTE_SWITCHES)
    assert pose_net.PoseNet(cfg).flow.update_fp16 is True                 # (the trackers build their PoseNet from this model config)
    # allowed together with the correlation's own precision flags
    for kw in (dict(mixed_precision=True), dict(alternate_corr=True), dict(alternate_corr=True, alt_corr_fp16=True)):
        assert raft.RAFT(synth.model_config(64, 96, update_fp16=True, **kw)).update_fp16 is True


def test_module_switch_is_part_of_the_snapshot(rpe, monkeypatch):
    from rpe_amd import raft
    snap = raft._switches()
    monkeypatch.setattr(raft, 'UPDATE_FP16', True)
    assert raft._switches() != snap and raft.RAFT({}).update_block.fp16()


@pytest.mark.parametrize('switch,value,word', [('CONV_BF16X3', True, 'CONV_BF16X3'), ('WINOGRAD', False, 'WINOGRAD'), ('PAD_MAPS', True, 'pad_maps'),
                                               ('PAD_ENCODERS', True, 'pad_encoders')])
def test_refused_module_switches(rpe, monkeypatch, switch, value, word):
    from rpe_amd import raft, synth
    net = raft.RAFT(synth.model_config(64, 96, update_fp16=True))
    monkeypatch.setattr(raft, switch, value)
    with pytest.raises(rpe.RpeError, match=word):
        raft.RAFT(synth.model_config(64, 96, update_fp16=True))              # at construction
    with pytest.raises(rpe.RpeError, match=word):
        net._check_update_fp16(12)                                           # and at every pass of a live model
    monkeypatch.setattr(raft, switch, not value)
    monkeypatch.setattr(raft, 'UPDATE_FP16', True)
    monkeypatch.setattr(raft, switch, value)
    with pytest.raises(rpe.RpeError, match=word):
        raft.RAFT(synth.model_config(64, 96))._check_update_fp16(12)         # the module switch on a model without the key


@pytest.mark.parametrize('key', ['pad_maps', 'pad_encoders'])
def test_refused_config_keys(rpe, key):
    from rpe_amd import raft, synth
    with pytest.raises(rpe.RpeError, match='valid-extent'):
        raft.RAFT(synth.model_config(64, 96, update_fp16=True, **{key: True}))
    assert raft.RAFT(synth.model_config(64, 96, **{key: True})).update_fp16 is False


def test_a_map_the_kernel_does_not_take_is_refused_not_run_in_f32(rpe):
    from rpe_amd import raft, synth
    net = raft.RAFT(synth.model_config(120, 152, update_fp16=True))
    net._check_update_fp16(20)
    with pytest.raises(rpe.RpeError, match='w8 = 19'):
        net._check_update_fp16(19)
    with pytest.raises(rpe.RpeError, match='w8 = 19'):
        net.update_block.packed_convs(19)
    assert raft.RAFT(synth.model_config(120, 152)).update_block.packed_convs(19) is None     # flag off: the generic route, as before


def test_abi_declared_bound_and_listed(rpe):
    from rpe_amd import _lib
    L, header = rpe.lib(), _header()
    for name in ('rpe_conv_f16_packed_bytes', 'rpe_conv_f16_pack', 'rpe_conv_f16'):
        assert re.search(r'\b' + name + r'\(', header) and name in _lib.SIGNATURES and hasattr(L, name), name
    # the header states the kind as the one after the last numbered kind: (RPE_OP_CORR_ALT_LOOKUP_DT + 1)
    base, plus = re.search(r'#define RPE_OP_CONV_F16 \((RPE_OP_\w+) \+ (\d+)\)', header).groups()
    numbered = {n: int(v) for n, v in re.findall(r'#define (RPE_OP_\w+) (\d+)', header)}
    kind = numbered[base] + int(plus)
    assert kind == _lib.OP_CONV_F16 == 41 == max(numbered.values()) + 1 and kind not in numbered.values()
    assert _lib.OP_CONV_F16 not in [v for k, v in vars(_lib).items() if k.startswith('OP_') and k != 'OP_CONV_F16']
    assert _lib.ALL_LIST_OPS[kind] == ('rpe_conv_f16', _lib.ConvDesc) and _lib.KIND_OF_ENTRY['rpe_conv_f16'] == kind
    src = open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'oplist.hip')).read()
    assert 'case RPE_OP_CONV_F16: return rpe_conv_f16(' in src
    assert 'SPECIAL VALUES (this entry point' in header


def test_size_query_and_argument_checks_without_a_gpu(rpe):
    """Bad pointers / extents -> RPE_E_BADARG, what the kernel does not take -> RPE_E_UNSUPPORTED, all before anything is dereferenced."""
    from rpe_amd import _lib
    L = rpe.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    frag = 2 * 64 * 8 * 2                                                   # bytes of a (32 channels x 32 rows) tap: two 16-channel fragments
    assert L.rpe_conv_f16_packed_bytes(256, 256, 3, 3) == 8 * 8 * 9 * frag
    assert L.rpe_conv_f16_packed_bytes(126, 324, 1, 1) == 4 * 11 * 1 * frag  # K tail and ragged cout are padded
    assert L.rpe_conv_f16_packed_bytes(20, 16, 3, 3) == 1 * 1 * 9 * frag and L.rpe_conv_f16_packed_bytes(1, 1, 5, 1) == 5 * frag
    for bad in ((64, 64, 7, 7), (64, 64, 3, 1), (64, 64, 5, 5), (0, 64, 3, 3), (64, 0, 3, 3)):
        assert L.rpe_conv_f16_packed_bytes(*bad) == 0, bad
    assert L.rpe_conv_f16_pack(null, 8, 8, 3, 3, one, null) == -1 and L.rpe_conv_f16_pack(one, 8, 8, 3, 3, null, null) == -1
    assert L.rpe_conv_f16_pack(one, 8, 8, 7, 7, one, null) == -3
    assert L.rpe_conv_f16(None, null) == -1
    good = dict(x=16, packed=16, out=16, b=1, cin=16, cout=16, h=8, w=12, kh=3, kw=3, mode=0)
    run = lambda **kw: L.rpe_conv_f16(ctypes.byref(_lib.ConvDesc(**dict(good, **kw))), null)
    for kw in (dict(x=0), dict(packed=0), dict(out=0), dict(b=0), dict(cin=0), dict(cout=0), dict(h=0), dict(w=-4), dict(mode=5), dict(mode=-1),
               dict(mode=2), dict(mode=2, out2=16, hidden=16, gate_channels=7), dict(mode=3), dict(mode=3, hidden=16)):
        assert run(**kw) == -1, kw
    for kw in (dict(w=10), dict(stride=2), dict(scale=16), dict(residual=16), dict(stats=16), dict(pre_norm=16), dict(kh=7, kw=7), dict(kh=3, kw=1),
               dict(x=20), dict(x_batch_stride=6), dict(out=24), dict(out2=8), dict(add=4), dict(packed=8), dict(b=65536),
               dict(mode=3, hidden=16, zgate=20), dict(mode=2, out2=16, hidden=24, gate_channels=8)):
        assert run(**kw) == -3, kw


def test_oracle_wrap_touches_exactly_the_covered_modules(rpe):
    from oracle import raft as oraft
    from rpe_amd import synth
    base = synth.init_synthetic_weights(oraft.RAFT(synth.model_config(64, 96, iters=2))).eval()
    wrapped = ref.f16_update_oracle(base)
    own = {n for n, m in wrapped.named_modules() if 'forward' in m.__dict__}
    want = {f'update_block.encoder.{n}' for n in ('convc1', 'convc2', 'convf2', 'conv')} | {f'update_block.gru.conv{g}{k}' for g in 'zrq' for k in '12'} | \
        {'update_block.flow_head.conv1', 'update_block.mask.0', 'update_block.mask.2'}
    assert own == want == set(ref.COVERED) == set(wrapped.wrapped_f16)
    assert not any('forward' in m.__dict__ for m in base.modules())          # the model handed in stays as it was
    for n, p in wrapped.named_parameters():                                  # parameters stay f32 and unchanged: only operands are rounded
        assert p.dtype == torch.float32 and torch.equal(p, dict(base.named_parameters())[n])


def test_oracle_moves_the_flow_and_wrapping_is_idempotent(rpe):
    """At 128 x 160, the smallest size of this suite's RAFT tests: on a 64 x 96 image the 8 x 12 map's fourth correlation level is 1 x 1, where the
    oracle's own bilinear sampler divides by zero -- the f32 oracle's flow is NaN there, with or without the wrap."""
    from oracle import raft as oraft
    from rpe_amd import synth
    H, W = 128, 160
    base = synth.init_synthetic_weights(oraft.RAFT(synth.model_config(H, W, iters=3))).eval()
    fr = synth.stereo_frames(5, 1, H, W)
    once = ref.f16_update_oracle(base)
    twice = ref.f16_update_oracle(once)
    with torch.no_grad():
        f32 = base(fr['image1l'], fr['image2l'])[0][-1]
        a, b = once(fr['image1l'], fr['image2l'])[0][-1], twice(fr['image1l'], fr['image2l'])[0][-1]
        again = base(fr['image1l'], fr['image2l'])[0][-1]
    d_cpu = float((a - f32).abs().max())
    print(f'{H}x{W}, 3 iterations: D_cpu = max|flow(fp16-operand oracle) - flow(f32 oracle)| = {d_cpu:.3e} px')
    assert d_cpu > 0 and bool(torch.isfinite(a).all())
    assert torch.equal(a, b) and torch.equal(again, f32)


def test_reference_rounding_and_epilogues():
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.9, 65520.0, -65520.0, 2.0 ** -14, 0.0, -0.0])
    want = torch.tensor([1.0, 1.0 + 2.0 ** -9, 65504.0, 65504.0, float('inf'), float('-inf'), 2.0 ** -14, 0.0, -0.0])
    assert torch.equal(ref.round_h(x), want)                                # ties to even, both parities; 65520 is the first value that overflows
    g = torch.Generator().manual_seed(0)
    xx, w, b = torch.randn(1, 4, 5, 8, generator=g), torch.randn(6, 4, 3, 3, generator=g), torch.randn(6, generator=g)
    lin, _ = ref.conv_ref(xx, w, b)
    assert torch.allclose(lin, torch.nn.functional.conv2d(ref.round_h(xx).double(), ref.round_h(w).double(), b.double(), padding=1))
    assert torch.equal(ref.conv_ref(xx, w, b, mode=ref.RELU)[0], lin.clamp_min(0)) and torch.equal(ref.conv_ref(xx, w, b, mode=ref.TANH)[0], torch.tanh(lin))
    hid = torch.randn(1, 3, 5, 8, generator=g)
    z, rh = ref.conv_ref(xx, w, b, mode=ref.GATE_ZR, hidden=hid, gate_channels=3)
    assert torch.equal(z, torch.sigmoid(lin[:, :3])) and torch.equal(rh, torch.sigmoid(lin[:, 3:]) * hid.double())
    zg = torch.rand(1, 6, 5, 8, generator=g)
    h6 = torch.randn(1, 6, 5, 8, generator=g)
    assert torch.equal(ref.conv_ref(xx, w, b, mode=ref.GATE_H, hidden=h6, zgate=zg)[0], (1 - zg.double()) * h6.double() + zg.double() * torch.tanh(lin))
