"""CPU: the backward of RAFT's update block (csrc/update_backward.hip) as far as it goes without a GPU -- the entry points declared, bound
and exported with RPE_ABI_MINOR unchanged, the new kernel sizes of rpe_conv_bwd_weight accepted and the others still refused, the host-side
refusals of ``grad_update`` / ``freeze_flow``, and the file compiling for gfx950 with every kernel at ScratchSize 0."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ('rpe_gru_gates_zr_recompute', 'rpe_gru_gates_h_recompute', 'rpe_gru_gates_zq_backward', 'rpe_gru_gates_r_backward')


def test_declared_bound_exported_minor_unchanged(rpe):
    from rpe_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'rpe.h')).read()
    L = rpe.lib()
    for name in NEW:
        assert re.search(r'\bint ' + name + r'\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
        assert name in header[header.index('minor 0:'):header.index('#define RPE_ABI_VERSION')], name
    assert int(re.search(r'#define RPE_ABI_MINOR (\d+)', header).group(1)) == 4 == L.rpe_abi_minor()


def test_weight_gradient_kernel_sizes(rpe):
    """(1,5), (5,1), (7,7) join (3,3) and (1,1) under the same workspace rule; everything else is still refused, in the library and in ops."""
    from rpe_amd import ops, raft_grad
    from rpe_amd._lib import RpeError
    L = rpe.lib()
    f = L.rpe_conv_bwd_weight_workspace_bytes
    r256 = lambda v: (v + 255) // 256 * 256
    for kh, kw in ((1, 5), (5, 1), (7, 7)):
        assert f(2, 8, 16, 25, 41, kh, kw) == r256(3 * 16 * 8 * kh * kw * 4) + r256(3 * 16 * 8)        # 2050 pixels: three chunks of 1024
    for kh, kw in ((5, 5), (1, 3), (3, 1), (7, 1), (1, 7), (5, 7), (0, 5), (9, 9)):
        assert f(1, 8, 16, 4, 4, kh, kw) == 0, (kh, kw)
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)              # never dereferenced: validation fails first
    bw = L.rpe_conv_bwd_weight
    assert bw(one, 8 * 15, one, 16 * 15, 1, 8, 16, 3, 5, 5, 5, 1.0, one, one, one, null) == -1
    assert bw(one, 8 * 15, one, 16 * 15, 1, 8, 16, 3, 5, 1, 3, 1.0, one, one, one, null) == -1
    assert bw(null, 8 * 15, one, 16 * 15, 1, 8, 16, 3, 5, 1, 5, 1.0, one, one, one, null) == -1
    assert bw(one, 8 * 15 - 1, one, 16 * 15, 1, 8, 16, 3, 5, 7, 7, 1.0, one, one, one, null) == -1
    if torch.cuda.is_available():
        x, dy = torch.zeros(1, 8, 4, 4, device='cuda'), torch.zeros(1, 16, 4, 4, device='cuda')
        for kernel in ((5, 5), (1, 3)):
            with pytest.raises(RpeError, match='unsupported shape'):
                ops.conv_bwd_weight(x, dy, kernel)
    assert len(raft_grad.UPDATE_PARAMS) == 22 and raft_grad.UPDATE_PARAMS[0] == 'gru.convz1.weight' and raft_grad.UPDATE_PARAMS[-1] == 'encoder.conv.bias'


def test_gate_entry_points_refuse_bad_arguments_without_a_gpu(rpe):
    L = rpe.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    per = 8 * 15
    zq = lambda a: L.rpe_gru_gates_zq_backward(*a)
    good = [one, per, one, per, one, per, one, per, 1, 8, 15, one, per, one, per, one, per, null]
    for i in (0, 2, 4, 6, 11, 13, 15):
        a = list(good)
        a[i] = null
        assert zq(a) == -1, i
    for i in (1, 3, 5, 7, 12, 14, 16):
        a = list(good)
        a[i] = per - 1
        assert zq(a) == -1, i
    assert zq(good[:8] + [0] + good[9:]) == 0 and zq(good[:8] + [65536] + good[9:]) == -1 and zq(good[:9] + [0] + good[10:]) == -1
    rb = lambda a: L.rpe_gru_gates_r_backward(*a)
    good = [one, per, one, per, one, per, one, per, 1, 8, 15, one, per, one, per, null]
    for i in (0, 2, 4, 6, 11, 13):
        a = list(good)
        a[i] = null
        assert rb(a) == -1, i
    assert rb(good[:1] + [per - 1] + good[2:]) == -1 and rb(good[:8] + [0] + good[9:]) == 0
    fz = L.rpe_gru_gates_zr_recompute
    assert fz(one, 2 * per - 1, one, per, 1, 8, 15, one, per, one, per, one, per, null) == -1           # zr_pre holds z | r
    assert fz(null, 2 * per, one, per, 1, 8, 15, one, per, one, per, one, per, null) == -1
    assert fz(one, 2 * per, one, per, 0, 8, 15, one, per, one, per, one, per, null) == 0
    fh = L.rpe_gru_gates_h_recompute
    assert fh(one, per, one, per, one, per, 1, 8, 15, one, per, null, per, null) == -1
    assert fh(one, per, one, per, one, per, 0, 8, 15, one, per, one, per, null) == 0


def test_host_side_refusals_before_any_launch(rpe):
    """grad_update with update_fp16 / CONV_BF16X3 / mixed_precision / no up-sampling, and freeze_flow's forms: raised on the CPU, where any
    launch would fail."""
    from rpe_amd import pose_net, raft, synth
    from rpe_amd._lib import RpeError
    img = torch.zeros(1, 3, 64, 96)
    for key in ('update_fp16', 'mixed_precision'):
        model = raft.RAFT(dict(synth.model_config(64, 96), **{key: True}))
        with pytest.raises(RpeError, match=key):
            model(img, img, grad_update=True)
    model = raft.RAFT(synth.model_config(64, 96))
    with pytest.raises(RpeError, match='upsample'):
        model(img, img, grad_update=True, upsample=False)
    raft.CONV_BF16X3 = True
    try:
        with pytest.raises(RpeError, match='CONV_BF16X3'):
            model(img, img, grad_update=True)
    finally:
        raft.CONV_BF16X3 = False
    assert len(model.update_params()) == 22 and model.update_params()[4] is model.update_block.gru.convq1.weight
    net = pose_net.PoseNet(synth.model_config(352, 352)).train().freeze_flow(True)
    with pytest.raises(NotImplementedError, match='stop at the flows'):
        net.freeze_flow(False)
    with pytest.raises(NotImplementedError):
        net.freeze_flow(False, parts=None)
    for bad in ('gru', 'encoder', 'all', ''):
        with pytest.raises(ValueError, match='parts'):
            net.freeze_flow(False, parts=bad)
    assert not net.flow_update_trainable() and not net.flow_heads_trainable()
    net.freeze_flow(False, parts='update')
    on = sorted(k for k, p in net.flow.named_parameters() if p.requires_grad)
    assert len(on) == 30 and on == sorted(k for k, _ in net.flow.named_parameters() if k.startswith('update_block.'))
    assert net.flow_update_trainable() and net.flow_heads_trainable()
    assert not net.freeze_flow(True).flow_update_trainable()
    net.freeze_flow(False, parts='heads')
    assert net.flow_heads_trainable() and not net.flow_update_trainable()


def test_kernels_build_for_gfx950_without_scratch(tmp_path):
    """hipcc --offload-arch=gfx950 with the Makefile's flags: every kernel of csrc/update_backward.hip reports ScratchSize 0."""
    import subprocess
    src = os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'update_backward.hip')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '-fPIC', '-Rpass-analysis=kernel-resource-usage',
                        '-c', src, '-o', str(tmp_path / 'update_backward.o')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    assert len(names) == len(scratch) == 4, names
    for kernel in ('k_gate_bwd_zq', 'k_gate_bwd_r', 'k_gate_fwd_zr', 'k_gate_fwd_h'):
        assert any(kernel in nm for nm in names), kernel
    assert scratch == [0] * 4, dict(zip(names, scratch))
    makefile = open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'Makefile')).read()
    assert 'update_backward.hip' in makefile and re.search(r'build/update_backward\.o: CXXFLAGS \+= -Rpass-analysis=kernel-resource-usage', makefile)
