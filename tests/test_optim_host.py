"""CPU: the training step's update (csrc/optim.hip) as far as it goes without a GPU -- the entry points declared, bound and exported with
RPE_ABI_MINOR unchanged, header and binding agreeing on every argument list and struct layout, the chunk rule, every bad-argument path
returning its code before any launch (fake pointers), ClippedAdamW's refusals at construction, the loss and the synthetic batches'
format, and the file compiling for gfx950 with both kernels at ScratchSize 0."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ('rpe_optim_chunk_floats', 'rpe_optim_chunk_offsets', 'rpe_optim_workspace_bytes', 'rpe_grad_norm', 'rpe_adamw_step')
CTYPE = {'void*': ctypes.c_void_p, 'int': ctypes.c_int, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'long long': ctypes.c_longlong}


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rpe.h')).read(), flags=re.S)


def test_declared_bound_exported_minor_unchanged(rpe):
    from rpe_amd import _lib
    raw = open(os.path.join(ROOT, 'include', 'rpe.h')).read()
    header, L = _header(), rpe.lib()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
        assert name in raw[raw.index('minor 0:'):raw.index('#define RPE_ABI_VERSION')], name      # listed for the next minor bump
    assert int(re.search(r'#define RPE_ABI_MINOR (\d+)', raw).group(1)) == 4 == L.rpe_abi_minor()       # the ABI only grew
    assert int(re.search(r'#define RPE_ABI_VERSION (\d+)', raw).group(1)) == 5 == L.rpe_abi_version()
    assert 'optim.hip' in open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'Makefile')).read()


def test_header_and_binding_agree_on_argument_lists_and_layouts(rpe):
    from rpe_amd import _lib
    header = _header()
    for name in NEW:
        ret, args = re.search(r'(\w[\w ]*?)\s+\b' + name + r'\s*\(([^)]*)\)', header).groups()
        want = []
        for a in (x.strip() for x in args.split(',')):
            if a == 'void':
                continue
            base = re.sub(r'\bconst\b', '', a)
            base = re.sub(r'\b\w+$', '', base.strip()).strip() if not base.strip().endswith('*') else base.strip()
            want.append('ptr' if '*' in base else base.strip())
        res, argtypes = _lib.SIGNATURES[name]
        assert res is CTYPE[ret.strip()], name
        got = ['ptr' if (t is ctypes.c_void_p or hasattr(t, 'contents')) else {v: k for k, v in CTYPE.items()}[t] for t in argtypes]
        assert got == want, (name, got, want)
    # struct mirrors and the record's layout as ops reads it
    assert ctypes.sizeof(_lib.OptimRow) == 40 and ctypes.sizeof(_lib.OptimChunk) == 8
    assert [f for f, _ in _lib.OptimRow._fields_] == re.search(r'struct rpe_optim_row \{([^}]*)\}', header).group(1).replace('*', ' ').replace(';', ' ') \
        .replace('const', ' ').replace('float', ' ').replace('long long', ' ').split()
    assert re.search(r'struct rpe_optim_record \{ double norm; float norm_f32; int reserved; long long nonfinite; long long reserved2; \}', header)
    assert int(re.search(r'#define RPE_OPTIM_CHUNK (\d+)', header).group(1)) == rpe.lib().rpe_optim_chunk_floats()


def test_chunk_rule_depends_on_the_sizes_alone(rpe):
    from rpe_amd import ops
    C = ops.optim_chunk()
    sizes = (1, 2, 3, 5, C - 1, C, C + 1, 2 * C + 5)
    chunks, n = ops.optim_chunk_offsets(sizes)
    assert [(c.row, c.offset) for c in chunks[:n]] == [(r, o) for r, s in enumerate(sizes) for o in range(0, s, C)]
    assert n == 5 + 1 + 2 + 3
    L = rpe.lib()
    one = (ctypes.c_longlong * 1)
    assert L.rpe_optim_chunk_offsets(one(0), 1, None, 0) == -1 and L.rpe_optim_chunk_offsets(one(-4), 1, None, 0) == -1
    assert L.rpe_optim_chunk_offsets(one(1 << 31), 1, None, 0) == -3 and L.rpe_optim_chunk_offsets(one((1 << 31) - 1), 1, None, 0) == -(-((1 << 31) - 1) // C)
    assert L.rpe_optim_chunk_offsets(None, 1, None, 0) == -1 and L.rpe_optim_chunk_offsets(None, -1, None, 0) == -1
    assert L.rpe_optim_chunk_offsets(None, 0, None, 0) == 0
    from rpe_amd import _lib
    assert L.rpe_optim_chunk_offsets(one(C + 1), 1, (_lib.OptimChunk * 1)(), 1) == -1                  # cap below the count
    assert L.rpe_optim_workspace_bytes(0) == 0 and L.rpe_optim_workspace_bytes(-3) == 0
    for k in (1, 3, 4, 5, 1000):
        assert L.rpe_optim_workspace_bytes(k) >= 16 + 12 * k and L.rpe_optim_workspace_bytes(k) % 16 == 0


def test_bad_arguments_return_status_without_a_gpu(rpe):
    L = rpe.lib()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(68)                # never dereferenced: validation fails first
    gn = L.rpe_grad_norm
    for i in (0, 2, 4, 5):
        a = [one, 1, one, 1, one, one, null]
        a[i] = null
        assert gn(*a) == -1, i
    assert gn(one, -1, one, 1, one, one, null) == -1 and gn(one, 1, one, -1, one, one, null) == -1
    assert gn(one, 2, one, 1, one, one, null) == -1                                              # fewer chunks than rows
    assert gn(one, 1, one, 1, odd, one, null) == -1 and gn(odd, 1, one, 1, one, one, null) == -1
    assert gn(one, 0, one, 0, one, one, null) == 0                                               # empty table: success, nothing launched
    ad = L.rpe_adamw_step
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1)
    for i in (0, 2, 4, 5, 6):
        a = [one, 1, one, 1, one, one, one]
        a[i] = null
        assert ad(*a, *hyper, null) == -1, i
    assert ad(one, -1, one, 1, one, one, one, *hyper, null) == -1 and ad(one, 1, one, -2, one, one, one, *hyper, null) == -1
    assert ad(one, 1, one, 1, one, one, odd, *hyper, null) == -1
    assert ad(one, 0, one, 0, one, one, one, *hyper, null) == 0


def test_optimizer_refuses_what_it_cannot_step(rpe):
    from rpe_amd import optim
    with pytest.raises(ValueError, match='float32 parameters on the GPU'):
        optim.ClippedAdamW([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
    with pytest.raises(ValueError, match='float32 parameters on the GPU'):
        optim.ClippedAdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))], lr=1e-3)
    with pytest.raises(ValueError, match='one parameter group'):
        optim.ClippedAdamW([dict(params=[torch.nn.Parameter(torch.zeros(3))]), dict(params=[torch.nn.Parameter(torch.zeros(2))])], lr=1e-3)
    with pytest.raises(ValueError, match='betas'):
        optim.ClippedAdamW([torch.nn.Parameter(torch.zeros(3))], lr=1e-3, betas=(1.0, 0.999))
    assert hasattr(torch.autograd.graph, 'increment_version') and optim._bump is torch.autograd.graph.increment_version
    t = torch.zeros(2)
    v = t._version
    optim._bump(t)
    assert t._version == v + 1


def test_training_pairs_have_the_reference_format_and_exact_poses(rpe):
    from oracle import se3 as ose3
    from rpe_amd import synth
    batches = list(synth.training_pairs(5, 2, 64, 96, batch=2))
    assert len(batches) == 2 and all(len(b) == 9 for b in batches)
    ref, trg, ref_r, trg_r, ref_m, trg_m, pose, K, bl = batches[0]
    assert all(tuple(x.shape) == (2, 3, 64, 96) and x.dtype == torch.float32 for x in (ref, trg, ref_r, trg_r))
    assert all(tuple(m.shape) == (2, 1, 64, 96) and m.dtype == torch.bool for m in (ref_m, trg_m))
    assert tuple(pose.shape) == (2, 7) and tuple(K.shape) == (2, 3, 3) and tuple(bl.shape) == (2,)
    again = list(synth.training_pairs(5, 2, 64, 96, batch=2))
    assert all(torch.equal(a, b) for x, y in zip(batches, again) for a, b in zip(x, y))
    # gt_pose = exp(xi) of the motion the frames were rendered with: unit quaternion, and exp(log(.)) returns it
    assert float((pose[:, 3:].norm(dim=1) - 1).abs().max()) < 1e-6
    back = ose3.se3_exp(ose3.se3_log(pose.double()))
    assert float((back - pose.double()).abs().max()) < 1e-6
    xi = ose3.se3_log(pose.double())
    R, t, vec = synth._se3_exp(xi[0].numpy())
    assert float((torch.from_numpy(vec) - pose[0].double()).abs().max()) < 1e-7
    assert float((ose3.se3_matrix(pose.double())[0, :3, :3] - torch.from_numpy(R)).abs().max()) < 1e-6


def test_kernels_build_for_gfx950_without_scratch(tmp_path):
    import subprocess
    src = os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'optim.hip')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '-fPIC', '-ffp-contract=off', '-Rpass-analysis=kernel-resource-usage',
                        '-c', src, '-o', str(tmp_path / 'optim.o')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    assert len(names) == len(scratch) == 2 and any('k_grad_norm' in n for n in names) and any('k_adamw' in n for n in names), names
    assert scratch == [0, 0], dict(zip(names, scratch))
    makefile = open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'build/optim\.o: CXXFLAGS \+= -ffp-contract=off', makefile)
