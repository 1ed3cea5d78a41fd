"""CPU: the backward of RAFT's output heads (csrc/raft_backward.hip) as far as it goes without a GPU -- the entry points declared, bound and
exported with RPE_ABI_MINOR unchanged, every bad-argument path returning its code before any launch (fake pointers), the workspace rule, the
host-side refusals of ``grad_heads`` / ``freeze_flow``, and the file compiling for gfx950 with every kernel at ScratchSize 0."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ('rpe_upsample_convex_backward', 'rpe_conv_bwd_weight', 'rpe_conv_bwd_weight_workspace_bytes', 'rpe_conv3x3_to2_bwd_data',
       'rpe_relu_backward', 'rpe_sum_groups')


def test_declared_bound_exported_minor_unchanged(rpe):
    from rpe_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'rpe.h')).read()
    L = rpe.lib()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert int(re.search(r'#define RPE_ABI_MINOR (\d+)', header).group(1)) == 4 == L.rpe_abi_minor()
    assert int(re.search(r'#define RPE_ABI_VERSION (\d+)', header).group(1)) == 5 == L.rpe_abi_version()
    for name in NEW:                                   # listed where the header says what the next bump counts
        assert name in header[header.index('minor 0:'):header.index('#define RPE_ABI_VERSION')], name


def test_workspace_follows_the_split_rule(rpe):
    f = rpe.lib().rpe_conv_bwd_weight_workspace_bytes
    assert f(0, 8, 8, 4, 4, 3, 3) == 0 and f(1, 8, 8, 4, 4, 5, 5) == 0 and f(1, 8, 8, 4, 4, 3, 1) == 0 and f(1, 0, 8, 4, 4, 3, 3) == 0
    r256 = lambda v: (v + 255) // 256 * 256

    def want(b, cin, cout, h, w, taps):
        K = b * h * w
        chunk = max(1024, (-(-K // 64) + 31) // 32 * 32)           # the documented rule: a function of b h w alone
        chunks = -(-K // chunk)
        return r256(chunks * cout * cin * taps * 4) + r256(chunks * cout * 8)
    for shape in ((1, 128, 256, 1, 1), (2, 128, 256, 3, 5), (1, 8, 16, 32, 32), (1, 8, 16, 25, 41), (48, 128, 256, 64, 80), (3, 256, 2, 40, 40)):
        for k in (3, 1):
            assert f(*shape, k, k) == want(*shape, k * k), (shape, k)
    # 1024 pixels are one chunk, 1025 two; never more than 64
    assert f(1, 64, 64, 32, 32, 1, 1) == r256(64 * 64 * 4) + r256(64 * 8) and f(1, 64, 64, 25, 41, 1, 1) == r256(2 * 64 * 64 * 4) + r256(2 * 64 * 8)
    assert f(48, 128, 256, 64, 80, 3, 3) == r256(64 * 256 * 128 * 9 * 4) + r256(64 * 256 * 8)


def test_bad_arguments_return_status_without_a_gpu(rpe):
    L = rpe.lib()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(20)     # never dereferenced: validation fails first
    up = L.rpe_upsample_convex_backward
    for i in (0, 1, 2, 6, 7):
        a = [one, one, one, 1, 3, 5, one, one, null]
        a[i] = null
        assert up(*a) == -1, i
    assert up(one, one, one, 1, 0, 5, one, one, null) == -1 and up(one, one, one, 1, 3, -5, one, one, null) == -1
    assert up(one, one, one, -1, 3, 5, one, one, null) == -1 and up(one, one, one, 65536, 3, 5, one, one, null) == -1
    assert up(odd, one, one, 1, 3, 5, one, one, null) == -1                            # grad_up is read in 16-byte pieces
    assert up(one, one, one, 0, 3, 5, one, one, null) == 0                             # empty batch: success, nothing launched
    bw = L.rpe_conv_bwd_weight

    def call(x=one, dy=one, dims=(1, 8, 16, 3, 5), k=(3, 3), xbs=None, dbs=None, dw=one, db=one, ws=one):
        b, cin, cout, h, w = dims
        return bw(x, cin * h * w if xbs is None else xbs, dy, cout * h * w if dbs is None else dbs, b, cin, cout, h, w, *k, 1.0, dw, db, ws, null)
    assert call(x=null) == -1 and call(dy=null) == -1 and call(ws=null) == -1 and call(dw=null, db=null) == -1
    assert call(ws=odd) == -1
    assert call(k=(5, 5)) == -1 and call(k=(1, 3)) == -1
    for bad in ((0, 8, 16, 3, 5), (1, 0, 16, 3, 5), (1, 8, 0, 3, 5), (1, 8, 16, 0, 5), (1, 8, 16, 3, -1)):
        assert call(dims=bad) == -1, bad
    assert call(xbs=8 * 15 - 1) == -1 and call(dbs=16 * 15 - 1) == -1                  # a batch stride shorter than the slice
    assert call(dims=(1 << 11, 8, 16, 1 << 10, 1 << 10)) == -3                         # b h w >= 2^31: pixel indices are 32 bits
    assert call(dims=(1, 1 << 12, 16, 1 << 10, 1 << 10)) == -3                         # cin h w >= 2^31
    d2 = L.rpe_conv3x3_to2_bwd_data
    for i in (0, 2, 9):
        a = [one, 30, one, one, 8 * 15, 1, 8, 3, 5, one, 8 * 15, null]
        a[i] = null
        assert d2(*a) == -1, i
    assert d2(one, 29, one, one, 120, 1, 8, 3, 5, one, 120, null) == -1 and d2(one, 30, one, one, 119, 1, 8, 3, 5, one, 120, null) == -1
    assert d2(one, 30, one, null, 0, 1, 8, 3, 5, one, 119, null) == -1 and d2(one, 30, one, null, 0, 1, 0, 3, 5, one, 120, null) == -1
    assert d2(one, 30, one, null, 0, 65536, 8, 3, 5, one, 120, null) == -1 and d2(one, 30, one, null, 0, 0, 8, 3, 5, one, 120, null) == 0
    rb = L.rpe_relu_backward
    for i in (0, 2, 7):
        a = [one, 120, one, 120, 1, 8, 15, one, 120, null]
        a[i] = null
        assert rb(*a) == -1, i
    assert rb(one, 119, one, 120, 1, 8, 15, one, 120, null) == -1 and rb(one, 120, one, 120, 1, 8, 0, one, 120, null) == -1
    assert rb(one, 120, one, 120, 0, 8, 15, one, 120, null) == 0
    sg = L.rpe_sum_groups
    assert sg(null, 4, 1, 8, 15, null, 0, one, 120, null) == -1 and sg(one, 4, 1, 8, 15, null, 0, null, 120, null) == -1
    assert sg(one, 0, 1, 8, 15, null, 0, one, 120, null) == -1 and sg(one, 4, 1, 8, 15, null, 0, one, 119, null) == -1
    assert sg(one, 4, 65536, 8, 15, null, 0, one, 120, null) == -1 and sg(one, 4, 1, 0, 15, null, 0, one, 120, null) == -1
    assert sg(one, 4, 0, 8, 15, null, 0, one, 120, null) == 0


def test_host_side_refusals_before_any_launch(rpe):
    """grad_heads with update_fp16 / CONV_BF16X3 / mixed_precision, and freeze_flow's two forms: raised on the CPU, where any launch would fail."""
    from rpe_amd import pose_net, raft, synth
    from rpe_amd._lib import RpeError
    img = torch.zeros(1, 3, 64, 96)
    for key in ('update_fp16', 'mixed_precision'):
        model = raft.RAFT(dict(synth.model_config(64, 96), **{key: True}))
        with pytest.raises(RpeError, match=key):
            model(img, img, grad_heads=True)
    model = raft.RAFT(synth.model_config(64, 96))
    raft.CONV_BF16X3 = True
    try:
        with pytest.raises(RpeError, match='CONV_BF16X3'):
            model(img, img, grad_heads=True)
    finally:
        raft.CONV_BF16X3 = False
    net = pose_net.PoseNet(synth.model_config(352, 352)).train().freeze_flow(True)
    with pytest.raises(NotImplementedError, match='stop at the flows'):
        net.freeze_flow(False)
    with pytest.raises(ValueError, match='parts'):
        net.freeze_flow(False, parts='gru')
    assert not net.flow_heads_trainable()
    net.freeze_flow(False, parts='heads')
    on = sorted(k for k, p in net.flow.named_parameters() if p.requires_grad)
    assert on == sorted(f'update_block.{m}.{t}' for m in ('flow_head.conv1', 'flow_head.conv2', 'mask.0', 'mask.2') for t in ('weight', 'bias'))
    assert net.flow_heads_trainable() and not net.freeze_flow(True).flow_heads_trainable()


def test_kernels_build_for_gfx950_without_scratch(tmp_path):
    """hipcc --offload-arch=gfx950 with the Makefile's flags: every kernel of csrc/raft_backward.hip reports ScratchSize 0."""
    import subprocess
    src = os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'raft_backward.hip')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '-fPIC', '-Rpass-analysis=kernel-resource-usage',
                        '-c', src, '-o', str(tmp_path / 'raft_backward.o')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    assert len(names) == len(scratch) == 14, names
    for kernel in ('k_upsample_convex_bwd', 'k_bw_gemmILi3ELi3E', 'k_bw_gemmILi1ELi1E', 'k_bw_gemmILi1ELi5E', 'k_bw_gemmILi5ELi1E', 'k_bw_gemmILi7ELi7E',
                   'k_bw_smallILi9E', 'k_bw_smallILi1E', 'k_splitk_reduce', 'k_bw_bias_part', 'k_bw_bias_sum', 'k_conv3x3_to2_bwd_data', 'k_relu_bwd',
                   'k_sum_groups'):
        assert any(kernel in nm for nm in names), kernel
    assert scratch == [0] * 14, dict(zip(names, scratch))
    makefile = open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'Makefile')).read()
    assert 'raft_backward.hip' in makefile and re.search(r'build/raft_backward\.o: CXXFLAGS \+= -Rpass-analysis=kernel-resource-usage', makefile)
