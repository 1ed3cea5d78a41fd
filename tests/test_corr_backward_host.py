"""CPU: the backward of the correlation (csrc/corr_backward.hip) as far as it goes without a GPU -- the entry points declared, bound and
exported with RPE_ABI_MINOR unchanged, their argument checks, the sizes of the gradient volume, the host-side refusals of ``grad_corr`` and
``freeze_flow`` raised before any launch, and the file compiling for gfx950 with every kernel at ScratchSize 0."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = {'rpe_corr_grad_volume_floats': 'size_t', 'rpe_corr_lookup_backward': 'int', 'rpe_corr_build_backward_workspace_bytes': 'size_t',
       'rpe_corr_build_backward': 'int'}


def test_declared_bound_exported_minor_unchanged(rpe):
    from rpe_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'rpe.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    L = rpe.lib()
    for name, ret in NEW.items():
        m = re.search(r'\b' + ret + ' ' + name + r'\s*\(([^;]*)\);', code)
        assert m, name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name          # one ctypes argument per declared parameter
        assert name in header[header.index('minor 0:'):header.index('#define RPE_ABI_VERSION')], name
    assert int(re.search(r'#define RPE_ABI_MINOR (\d+)', header).group(1)) == 4 == L.rpe_abi_minor()
    assert int(re.search(r'#define RPE_ABI_VERSION (\d+)', header).group(1)) == 5 == L.rpe_abi_version()


def test_sizes_and_argument_checks_without_a_gpu(rpe):
    L = rpe.lib()
    vol = L.rpe_corr_grad_volume_floats
    assert vol(2, 21, 23, 4) == 2 * 483 * (483 + 110 + 25 + 4) and vol(1, 64, 80, 4) == 5120 * 6800       # 139 MB per pair at 640 x 512
    assert vol(1, 16, 16, 4) == 256 * 340 and vol(1, 15, 16, 4) == 0 and vol(1, 16, 16, 5) == 0 and vol(0, 16, 16, 4) == 0
    ws = L.rpe_corr_build_backward_workspace_bytes
    assert ws(1, 256, 16, 16, 4) > 0 and ws(1, 4, 16, 16, 4) > 0
    for c in (0, 6, 258, 260, -4):
        assert ws(1, c, 16, 16, 4) == 0, c
    assert ws(1, 8, 15, 16, 4) == 0
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)              # never dereferenced: validation fails first
    lb = L.rpe_corr_lookup_backward
    assert lb(null, one, 1, 16, 16, 4, 4, one, null) == -1 and lb(one, null, 1, 16, 16, 4, 4, one, null) == -1
    assert lb(one, one, 1, 16, 16, 4, 4, null, null) == -1 and lb(one, one, 1, 16, 16, 4, 3, one, null) == -1
    assert lb(one, one, 1, 15, 16, 4, 4, one, null) == -1 and lb(one, one, 65536, 16, 16, 4, 4, one, null) == -1
    bb = L.rpe_corr_build_backward
    good = [one, one, one, 1, 8, 16, 16, 4, one, one, null, one, null]
    for i in (0, 1, 2, 8, 9, 11):
        a = list(good)
        a[i] = null
        assert bb(*a) == -1, i
    for i, v in ((4, 6), (4, 260), (5, 15), (7, 5)):
        a = list(good)
        a[i] = v
        assert bb(*a) == -1, (i, v)


def test_host_side_refusals_before_any_launch(rpe):
    """grad_corr with alternate_corr, update_fp16, mixed_precision, CONV_BF16X3: raised on the CPU, where any launch would fail."""
    from rpe_amd import pose_net, raft, synth
    from rpe_amd._lib import RpeError
    img = torch.zeros(1, 3, 64, 96)
    for key in ('alternate_corr', 'update_fp16', 'mixed_precision'):
        model = raft.RAFT(dict(synth.model_config(64, 96), **{key: True}))
        with pytest.raises(RpeError, match=key):
            model(img, img, grad_corr=True)
    model = raft.RAFT(synth.model_config(64, 96))
    raft.CONV_BF16X3 = True
    try:
        with pytest.raises(RpeError, match='CONV_BF16X3'):
            model(img, img, grad_corr=True)
    finally:
        raft.CONV_BF16X3 = False
    net = pose_net.PoseNet(dict(synth.model_config(352, 352), alternate_corr=True)).train().freeze_flow(True)
    z = torch.zeros(1, 3, 352, 352)
    with pytest.raises(RpeError, match='alternate_corr'):
        net(z, z, torch.eye(3)[None], torch.ones(1), z, z, ret_flows=True, grad_corr=True)
    with pytest.raises(ValueError, match='ret_flows'):
        net(z, z, torch.eye(3)[None], torch.ones(1), z, z, grad_corr=True)
    with pytest.raises(NotImplementedError, match='encoders have no backward'):
        net.freeze_flow(False)
    assert 'correlation has a backward' in pose_net.PoseNet.freeze_flow.__doc__


def test_kernels_build_for_gfx950_without_scratch(tmp_path):
    import subprocess
    src = os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'corr_backward.hip')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '-fPIC', '-Rpass-analysis=kernel-resource-usage',
                        '-c', src, '-o', str(tmp_path / 'corr_backward.o')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    assert len(names) == len(scratch) == 6, names
    for kernel in ('k_corr_lookup_bwd', 'k_cb_pool', 'k_cb_gemmILb0E', 'k_cb_gemmILb1E', 'k_splitk_reduce', 'k_cb_unpool'):
        assert any(kernel in nm for nm in names), kernel
    assert scratch == [0] * 6, dict(zip(names, scratch))
    makefile = open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'Makefile')).read()
    assert 'corr_backward.hip' in makefile and re.search(r'build/corr_backward\.o: CXXFLAGS \+= -Rpass-analysis=kernel-resource-usage', makefile)
