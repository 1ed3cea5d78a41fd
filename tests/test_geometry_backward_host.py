"""CPU: the backward of the fused geometry stage (csrc/geometry_backward.hip) as far as it goes without a GPU -- the three entry points
declared, bound and exported with RPE_ABI_MINOR unchanged, every bad-argument path returning its code before any launch (fake pointers),
and the float64 truth of the GPU tests (tests/geometry_grad_ref.py): its forward pinned to the reference's own outputs
(tests/golden/warp.npz, geometry.npz), its gradients checked against finite differences (torch.autograd.gradcheck, 8x16)."""
import ctypes
import os
import re

import torch

import geometry_grad_ref as ref
from conftest import ROOT, load_golden

NEW = ('rpe_depth_backproject_warp_backward', 'rpe_depth_backproject_warp_backward_workspace_bytes', 'rpe_flow2depth_backward')


def test_declared_bound_exported_minor_unchanged(rpe):
    from rpe_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'rpe.h')).read()
    L = rpe.lib()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert int(re.search(r'#define RPE_ABI_MINOR (\d+)', header).group(1)) == 4 == L.rpe_abi_minor()
    for name in NEW:                                   # listed where the header says what the next bump counts
        assert name in header[header.index('minor 0:'):header.index('#define RPE_ABI_VERSION')], name


def test_workspace_size(rpe):
    L = rpe.lib()
    f = L.rpe_depth_backproject_warp_backward_workspace_bytes
    assert f(0, 8, 8) == 0 and f(1, 0, 8) == 0 and f(1, 8, -8) == 0 and f(-1, 8, 8) == 0
    hw = 512 * 640
    assert f(1, 512, 640) >= 7 * hw * 4 and f(1, 512, 640) % 256 == 0            # counts, cursors, offsets and four list entries per pixel
    assert f(16, 512, 640) >= 16 * 7 * hw * 4 and f(3, 8, 8) > 0


def test_bad_arguments_return_status_without_a_gpu(rpe):
    L = rpe.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)          # never dereferenced: argument validation fails first
    bw = L.rpe_depth_backproject_warp_backward

    def call(ins=None, dims=(1, 8, 8), grads=None, outs=None, ws=one):
        return bw(*(ins or [one] * 8), *dims, *(grads or [one] * 4), *(outs or [one] * 4), ws, null)
    for i in range(8):                                           # every forward input is required
        assert call(ins=[null if j == i else one for j in range(8)]) == -1, i
    assert call(ws=null) == -1
    assert call(dims=(1, 12, 16)) == -1 and call(dims=(1, 16, 12)) == -1                      # h % 8, w % 8
    assert call(dims=(1, 0, 8)) == -1 and call(dims=(1, 8, -8)) == -1 and call(dims=(-1, 8, 8)) == -1
    assert call(outs=[one, ctypes.c_void_p(20), one, one]) == -1                              # (n,2,h,w) pointers are 16-byte aligned
    assert call(dims=(1, 1 << 15, 1 << 14)) == -3                                             # h*w >= 2^29: a list entry is 32 bits
    assert call(dims=(65536, 8, 8)) == -1                                                     # more rows than grid lines (the header says so)
    assert call(dims=(0, 8, 8)) == 0                                                          # empty batch: success, nothing launched
    assert call(dims=(0, 8, 8), grads=[null] * 4, outs=[null] * 4) == 0                       # NULL gradients / outputs are legal
    fb = L.rpe_flow2depth_backward
    for i in (0, 1, 2, 6):
        a = [one, one, one, 1, 8, 8, one, null]
        a[i] = null
        assert fb(*a) == -1, i
    assert fb(one, one, one, 1, 0, 8, one, null) == -1 and fb(one, one, one, -1, 8, 8, one, null) == -1
    assert fb(one, one, one, 65536, 8, 8, one, null) == -1
    assert fb(one, one, one, 0, 3, 5, one, null) == 0


def test_kernels_build_for_gfx950_without_scratch(tmp_path):
    """hipcc --offload-arch=gfx950 with the Makefile's flags: every kernel of csrc/geometry_backward.hip reports ScratchSize 0."""
    import subprocess
    src = os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'geometry_backward.hip')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '-fPIC', '-Rpass-analysis=kernel-resource-usage',
                        '-c', src, '-o', str(tmp_path / 'geometry_backward.o')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    assert len(names) == len(scratch) == 6 and all('k_gb_' in nm or 'k_flow2depth_bwd' in nm for nm in names), names
    assert scratch == [0] * 6, dict(zip(names, scratch))


def test_restatement_forward_matches_the_reference_goldens():
    g = load_golden('warp.npz')
    assert torch.equal(ref.remap(g['x'], g['flow']), g['bilinear'])                           # remap_from_flow of the reference itself
    q = load_golden('geometry.npz')
    assert torch.equal(ref.backproject(q['depth'], q['K']).reshape(2, 3, -1), q['reproject'][:, :3])      # PoseNet.proj
    # and against oracle.warp (pinned to the same files by tests/test_oracle_golden.py) on the whole stage, bit for bit in float32
    from oracle import warp
    c = ref.case(2, 16, 24, seed=5)
    out = ref.stage(*[c[k] for k in ref.INPUTS if k != 'mask2'])
    d2, valid = warp.flow2depth(c['stereo_flow2'], c['baseline'])
    assert torch.equal(ref.flow2depth(c['stereo_flow2'], c['baseline'])[0], d2)
    pcl1, pcl2 = warp.backproject(c['depth1'], c['K']), warp.backproject(d2, c['K'])
    pcl2w, _, inp1, inp2 = warp.weight_inputs(pcl1, pcl2, c['image1l'], c['image2l'], c['mask2'] & valid, c['time_flow'], c['stereo_flow1'],
                                              c['stereo_flow2'])
    for k, v in dict(pcl1=pcl1, pcl2w=pcl2w, inp1=inp1, inp2=inp2).items():
        assert torch.equal(out[k], v), k
    # the explicit-tap sampler is the same function where the positions are not integers
    taps = warp.sample_taps(c['time_flow'])
    s = ref.remap_at_taps(dict(x0=torch.from_numpy(taps['x0']), y0=torch.from_numpy(taps['y0'])))
    want = ref.remap(c['image2l'].double(), c['time_flow'].double())
    assert float((s(c['image2l'].double(), c['time_flow'].double()) - want).abs().max()) < 1e-3 * 255      # float32 positions: ~1e-6 px apart


def test_restatement_passes_gradcheck():
    c = ref.case(1, 8, 16, seed=9)
    ref.decisions(c)
    d = {k: c[k].double() for k in ref.INPUTS if k != 'mask2'}
    leaves = [d[k].clone().requires_grad_(True) for k in ('stereo_flow2', 'time_flow', 'depth1', 'stereo_flow1')]

    def f(sf2, tf, d1, sf1):
        o = ref.stage(sf2, tf, d['baseline'], d['K'], d1, d['image1l'], d['image2l'], sf1)
        return o['pcl1'], o['pcl2w'], o['inp1'], o['inp2']
    assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-5, rtol=1e-4)
    leaf = d['stereo_flow1'].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda s: ref.flow2depth(s, d['baseline'])[0], [leaf], eps=1e-6, atol=1e-6, rtol=1e-4)
    # the fixed-tap sampler differentiates the same function
    from oracle import warp
    taps = warp.sample_taps(c['time_flow'])
    s = ref.remap_at_taps(dict(x0=torch.from_numpy(taps['x0']), y0=torch.from_numpy(taps['y0'])))
    up = ref.upstream(1, 8, 16)
    a, b = ref.stage_grads(c, up, torch.float64), ref.stage_grads(c, up, torch.float64, sampler=s)
    for k in ref.GRADS:
        assert ref.ratio(b[k], a[k]) < 1e-4, k                     # float32 positions against float64 positions
