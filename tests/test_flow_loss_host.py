"""CPU: RAFT's sequence loss (csrc/flow_loss.hip) and ``grad_all_flows`` as far as they go without a GPU -- the entry points declared, bound
and exported with header and binding agreeing on every argument list, every bad-argument path returning its code before any launch (fake
pointers), the refusals of ops.flow_sequence_loss and of RAFT.forward(grad_all_flows=True) raised before ANY library call (the loaded
library is replaced by a trap), the format of synth.flow_pairs, and the file compiling for gfx950 with its kernels at ScratchSize 0."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ('rpe_flow_sequence_loss_workspace_bytes', 'rpe_flow_sequence_loss', 'rpe_flow_sequence_loss_backward')
CTYPE = {'int': ctypes.c_int, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t}


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rpe.h')).read(), flags=re.S)


def test_declared_bound_exported_and_in_the_makefile(rpe):
    from rpe_amd import _lib
    raw = open(os.path.join(ROOT, 'include', 'rpe.h')).read()
    header, L = _header(), rpe.lib()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
        assert name in raw[raw.index('minor 0:'):raw.index('#define RPE_ABI_VERSION')], name      # listed for the next minor bump
    assert int(re.search(r'#define RPE_ABI_MINOR (\d+)', raw).group(1)) == L.rpe_abi_minor()            # the ABI only grew
    assert int(re.search(r'#define RPE_ABI_VERSION (\d+)', raw).group(1)) == L.rpe_abi_version()
    assert 'flow_loss.hip' in open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'Makefile')).read()
    # the departure from upstream is stated where a C caller reads it
    assert 'EXACTLY ZERO' in raw[raw.index('csrc/flow_loss.hip'):raw.index('#define RPE_FLOW_LOSS_TILE')]


def test_header_and_binding_agree_on_argument_lists(rpe):
    from rpe_amd import _lib, ops
    header = _header()
    for name in NEW:
        ret, args = re.search(r'(\w[\w ]*?)\s+\b' + name + r'\s*\(([^)]*)\)', header).groups()
        want = []
        for a in (x.strip() for x in args.split(',')):
            want.append('ptr' if '*' in a else re.sub(r'\s*\b\w+$', '', re.sub(r'\bconst\b', '', a).strip()).strip())
        res, argtypes = _lib.SIGNATURES[name]
        assert res is CTYPE[ret.strip()], name
        got = ['ptr' if t is ctypes.c_void_p else {v: k for k, v in CTYPE.items()}[t] for t in argtypes]
        assert got == want, (name, got, want)
    # the record's layout as ops reads it
    idx = {k: int(re.search(r'#define RPE_FLOW_LOSS_' + k + r' (\d+)', header).group(1)) for k in ('LOSS', 'EPE', '1PX', '3PX', '5PX', 'COUNT', 'TERMS')}
    F = ops.FLOW_LOSS_FIELDS
    assert (F['loss'], F['epe'], F['px1'], F['px3'], F['px5'], F['count']) == tuple(idx[k] for k in ('LOSS', 'EPE', '1PX', '3PX', '5PX', 'COUNT'))
    assert idx['TERMS'] == F['count'] + 1
    tile = int(re.search(r'#define RPE_FLOW_LOSS_TILE (\d+)', header).group(1))
    L = rpe.lib()
    for n, b, h, w in ((1, 1, 8, 8), (3, 2, 17, 23), (12, 1, 512, 640)):
        assert L.rpe_flow_sequence_loss_workspace_bytes(n, b, h, w) == (n + 5) * -(-(b * h * w) // tile) * 8
    assert L.rpe_flow_sequence_loss_workspace_bytes(0, 1, 8, 8) == 0 and L.rpe_flow_sequence_loss_workspace_bytes(1, 1, 0, 8) == 0


def test_bad_arguments_return_status_without_a_gpu(rpe):
    L = rpe.lib()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(68)                # never dereferenced: validation fails first
    fw, bw = L.rpe_flow_sequence_loss, L.rpe_flow_sequence_loss_backward
    good = [one, 3, one, one, one, 2, 17, 23, 40.0, one, one, one]
    for i in (0, 2, 3, 4, 9, 10, 11):
        a = list(good)
        a[i] = null
        assert fw(*a, null) == -1, i
    for i, v in ((1, 0), (5, 0), (6, 0), (7, -1), (8, 0.0), (8, float('nan')), (0, odd), (4, odd), (9, odd), (10, odd)):
        a = list(good)
        a[i] = v
        assert fw(*a, null) == -1, (i, v)
    a = list(good)
    a[1] = 1025
    assert fw(*a, null) == -3
    a = list(good)
    a[6], a[7] = 1 << 15, 1 << 15
    assert fw(*a, null) == -3
    good = [one, 3, one, one, one, one, 2, 17, 23, 40.0, one]
    for i in (0, 2, 3, 4, 5, 10):
        a = list(good)
        a[i] = null
        assert bw(*a, null) == -1, i
    for i, v in ((1, -2), (6, 0), (9, -1.0), (10, odd)):
        a = list(good)
        a[i] = v
        assert bw(*a, null) == -1, (i, v)


class _Trap:
    def __getattr__(self, name):
        raise AssertionError(f'the library was called: {name}')


def test_refusals_before_any_library_call(rpe, monkeypatch):
    from rpe_amd import _lib, ops, raft, synth, train
    from rpe_amd._lib import RpeError
    rpe.lib()
    monkeypatch.setattr(_lib, '_lib', _Trap())
    gt, valid = torch.zeros(2, 2, 8, 12), torch.ones(2, 8, 12, dtype=torch.bool)
    pred = torch.zeros(2, 2, 8, 12)
    for fn in (ops.flow_sequence_loss, train.sequence_loss):
        with pytest.raises(RpeError, match='non-empty'):
            fn([], gt, valid)
        with pytest.raises(RpeError, match='shape'):
            fn([pred, torch.zeros(2, 2, 8, 16)], gt, valid)
        with pytest.raises(RpeError, match='shape'):
            fn([torch.zeros(1, 2, 8, 12)], gt, valid)
        with pytest.raises(RpeError, match='float32'):
            fn([pred.double()], gt, valid)
        with pytest.raises(RpeError, match='float32'):
            fn([pred.half()], gt, valid)
        with pytest.raises(RpeError, match='contiguous'):
            fn([torch.zeros(2, 2, 12, 8).transpose(2, 3)], gt, valid)
        with pytest.raises(RpeError, match='flow_gt'):
            fn([pred], gt.double(), valid)
        with pytest.raises(RpeError, match='flow_gt'):
            fn([torch.zeros(2, 3, 8, 12)], torch.zeros(2, 3, 8, 12), valid)
        for bad in (torch.ones(2, 8, 12), torch.ones(2, 2, 8, 12, dtype=torch.bool), torch.ones(8, 12, dtype=torch.bool), torch.ones(2, 8, 13, dtype=torch.uint8),
                    torch.ones(2, 8, 12, dtype=torch.int64), None):
            with pytest.raises(RpeError, match='valid'):
                fn([pred], gt, bad)
        for ok in (valid, valid[:, None], valid.to(torch.uint8)):                     # accepted forms: refused only for where they live
            with pytest.raises(RpeError, match='on the GPU'):
                fn([pred], gt, ok)
    # RAFT.forward(grad_all_flows=True): without all_flows, without a stage, with upsample=False -- the encoders have not run
    model = raft.RAFT(synth.model_config(64, 96))
    img = torch.zeros(1, 3, 64, 96)
    with pytest.raises(RpeError, match='all_flows=True'):
        model(img, img, grad_encoders=True, grad_all_flows=True)
    with pytest.raises(RpeError, match='gradient stage'):
        model(img, img, all_flows=True, grad_all_flows=True)
    for stage in ('grad_heads', 'grad_update', 'grad_corr', 'grad_encoders'):
        with pytest.raises(RpeError, match='upsample=True'):
            model(img, img, all_flows=True, upsample=False, grad_all_flows=True, **{stage: True})
    f = torch.zeros(1, 256, 8, 12)
    with pytest.raises(RpeError, match='all_flows=True'):
        model.grad_pass((f, f), f, stages='update', grad_all_flows=True)
    with pytest.raises(RpeError, match='upsample=True'):
        model.grad_pass((f, f), f, stages='heads', grad_all_flows=True, all_flows=True, upsample=False)


def test_flow_pairs_format_and_content(rpe):
    from rpe_amd import synth
    batches = list(synth.flow_pairs(5, 2, 64, 96, batch=2))
    assert len(batches) == 2 and all(len(b) == 4 for b in batches)
    im1, im2, gt, valid = batches[0]
    assert all(tuple(x.shape) == (2, 3, 64, 96) and x.dtype == torch.float32 and 0 <= float(x.min()) and float(x.max()) <= 255 for x in (im1, im2))
    assert tuple(gt.shape) == (2, 2, 64, 96) and gt.dtype == torch.float32 and bool(torch.isfinite(gt).all()) and float(gt.abs().max()) > 0.1
    assert tuple(valid.shape) == (2, 64, 96) and valid.dtype == torch.bool
    for row in valid:                                                   # all true but one rectangle of h/5 x w/4
        off = (~row).nonzero()
        (y0, x0), (y1, x1) = off.min(0).values.tolist(), off.max(0).values.tolist()
        assert (y1 - y0 + 1, x1 - x0 + 1) == (64 // 5, 96 // 4) and int((~row).sum()) == (64 // 5) * (96 // 4)
    again = list(synth.flow_pairs(5, 2, 64, 96, batch=2))
    assert all(torch.equal(a, b) for x, y in zip(batches, again) for a, b in zip(x, y))
    # flow_gt is the flow image2 was rendered with: warping image2 back along it returns image1 far better than image2 itself does
    back = synth._warp(im2[:1], gt[:1, 0], gt[:1, 1])
    inner = (slice(None), slice(None), slice(8, -8), slice(8, -8))
    assert float((back - im1[:1])[inner].abs().mean()) < 0.5 * float((im2[:1] - im1[:1])[inner].abs().mean())


def test_kernels_build_for_gfx950_without_scratch(tmp_path):
    import subprocess
    src = os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'flow_loss.hip')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '-fPIC', '-Rpass-analysis=kernel-resource-usage',
                        '-c', src, '-o', str(tmp_path / 'flow_loss.o')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    assert len(names) == len(scratch) == 3 and all(any(k in n for n in names) for k in ('k_flow_loss_partial', 'k_flow_loss_finish', 'k_flow_loss_backward')), names
    assert scratch == [0, 0, 0], dict(zip(names, scratch))
    makefile = open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'build/flow_loss\.o: CXXFLAGS \+= -Rpass-analysis=kernel-resource-usage', makefile)
