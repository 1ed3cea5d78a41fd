"""CPU: the on-the-fly correlation route on fp16 feature maps (RAFT's alt_corr_fp16; csrc/corr_alt.hip) -- its three entry points are
declared, bound and exported, its two launch list kinds agree between the header, the binding and csrc/oplist.hip, its scratch size obeys
the stated bounds on the grid of tests/test_corr_alt_host.py, bad arguments are refused without a GPU, and the config key needs
alternate_corr while alternate_corr + mixed_precision stays refused."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ('rpe_corr_alt_bytes_ex', 'rpe_corr_alt_prepare_ex', 'rpe_corr_alt_lookup_dt')
F32, F16 = 0, 2


def _header():
    return open(os.path.join(ROOT, 'include', 'rpe.h')).read()


def test_alt16_abi_declared_bound_exported(rpe):
    from rpe_amd import _lib
    L, header = rpe.lib(), _header()
    for name in NEW:
        assert re.search(r'\b' + name + r'\(', header) and name in _lib.SIGNATURES and hasattr(L, name), name
    assert (_lib.F32, _lib.F16) == (F32, F16)
    assert int(re.search(r'#define RPE_F32 (\d+)', header).group(1)) == F32 and int(re.search(r'#define RPE_F16 (\d+)', header).group(1)) == F16
    assert L.rpe_abi_minor() == 4 and int(re.search(r'#define RPE_ABI_MINOR (\d+)', header).group(1)) == 4


def test_alt16_kinds_agree_on_both_sides(rpe):
    from rpe_amd import _lib
    header = _header()
    assert int(re.search(r'#define RPE_OP_CORR_ALT_PREPARE_EX (\d+)', header).group(1)) == _lib.OP_CORR_ALT_PREPARE_EX == 39
    assert int(re.search(r'#define RPE_OP_CORR_ALT_LOOKUP_DT (\d+)', header).group(1)) == _lib.OP_CORR_ALT_LOOKUP_DT == 40
    kinds = [int(m) for m in re.findall(r'#define RPE_OP_\w+ (\d+)', header)]
    assert max(kinds) == 40 and len(kinds) == len(set(kinds))           # the next free numbers, none reused
    assert _lib.ALL_LIST_OPS[39] == ('rpe_corr_alt_prepare_ex', _lib.CorrAltPrepareExArgs)
    assert _lib.ALL_LIST_OPS[40] == ('rpe_corr_alt_lookup_dt', _lib.CorrAltLookupDtArgs)
    assert _lib.KIND_OF_ENTRY['rpe_corr_alt_prepare_ex'] == 39 and _lib.KIND_OF_ENTRY['rpe_corr_alt_lookup_dt'] == 40
    assert 39 not in _lib.LIST_OPS and 40 not in _lib.LIST_OPS           # (behind the event ops, like the encoder kinds)
    # struct sizes pinned on both sides, and the binding's argtypes are the struct's fields plus the stream
    assert ctypes.sizeof(_lib.CorrAltPrepareExArgs) == 48 and _lib.CorrAltPrepareExArgs.feature_dtype.offset == 36 and _lib.CorrAltPrepareExArgs.scratch.offset == 40
    assert ctypes.sizeof(_lib.CorrAltLookupDtArgs) == 64 and _lib.CorrAltLookupDtArgs.feature_dtype.offset == 48 and _lib.CorrAltLookupDtArgs.out.offset == 56
    src = open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'oplist.hip')).read()
    for st, size, kind in (('rpe_corr_alt_prepare_ex_args', 48, 'RPE_OP_CORR_ALT_PREPARE_EX'), ('rpe_corr_alt_lookup_dt_args', 64, 'RPE_OP_CORR_ALT_LOOKUP_DT')):
        assert f'static_assert(sizeof({st}) == {size},' in src and f'case {kind}:' in src and f'typedef struct {st} ' in header
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    L = rpe.lib()
    for kind in (39, 40):
        entry, struct = _lib.ALL_LIST_OPS[kind]
        assert list(getattr(L, entry).argtypes) == [t for _, t in struct._fields_] + [ctypes.c_void_p], entry
        params = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % entry, text).group(1)
        assert len(params.split(',')) == len(struct._fields_) + 1, entry


def test_alt16_bytes_on_the_grid_of_the_f32_route(rpe):
    L = rpe.lib()
    pad = int(re.search(r'#define RPE_CORR_ALT_PAD (\d+)', _header()).group(1))
    n = 0
    for h8 in (0, 1, 2, 3, 4, 5, 7, 8, 12, 15, 16, 17, 64):
        for w8 in (0, 1, 2, 3, 4, 6, 9, 16, 20, 31, 80):
            for levels in (0, 1, 2, 3, 4, 5):
                for b in (0, 1, 3):
                    for c in (256, 48, 16):
                        f32 = L.rpe_corr_alt_bytes(b, c, h8, w8, levels)
                        assert L.rpe_corr_alt_bytes_ex(b, c, h8, w8, levels, F32) == f32
                        b16 = L.rpe_corr_alt_bytes_ex(b, c, h8, w8, levels, F16)
                        assert (b16 == 0) == (f32 == 0), (b, c, h8, w8, levels, b16, f32)
                        if f32:
                            n += 1
                            assert 2 * (b * c * h8 * w8 * 2) <= b16 <= b * c * h8 * w8 * 2 * (1 + 4 / 3) + pad * levels, (b, c, h8, w8, levels, b16)
                            assert b16 <= 0.5 * f32 + pad * levels and b16 % 256 == 0
                        for dt in (1, 3, -1, 4):                            # RPE_F64, RPE_F32X3 and numbers that are no dtype
                            assert L.rpe_corr_alt_bytes_ex(b, c, h8, w8, levels, dt) == 0
    assert n > 300                                              # (the grid does hold supported geometries)
    for c in (0, -16, 8, 24, 272):                              # channel counts rpe_corr_build refuses
        assert L.rpe_corr_alt_bytes_ex(1, c, 16, 16, 4, F16) == 0
    # 1280 x 1024, 32 pairs: 1.56 GB -> about 0.78 GB
    assert L.rpe_corr_alt_bytes_ex(32, 256, 128, 160, 4, F16) * 2 == L.rpe_corr_alt_bytes(32, 256, 128, 160, 4)


def test_alt16_bad_arguments_return_badarg_without_a_gpu(rpe):
    L = rpe.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)          # never dereferenced: the argument checks fail first
    for dt in (F16, F32):                                       # (RPE_F32 forwards to the f32 forms: the same refusals)
        assert L.rpe_corr_alt_prepare_ex(null, one, 1, 256, 8, 16, 3, dt, one, null) == -1
        assert L.rpe_corr_alt_prepare_ex(one, null, 1, 256, 8, 16, 3, dt, one, null) == -1
        assert L.rpe_corr_alt_prepare_ex(one, one, 1, 256, 8, 16, 3, dt, null, null) == -1
        assert L.rpe_corr_alt_prepare_ex(one, one, 1, 24, 8, 16, 3, dt, one, null) == -1
        assert L.rpe_corr_alt_prepare_ex(one, one, 1, 256, 8, 16, 4, dt, one, null) == -1                       # the fourth level would be 1 x 2
        assert L.rpe_corr_alt_prepare_ex(one, one, 1, 256, 8, 16, 3, dt, ctypes.c_void_p(20), null) == -1       # scratch not 16-byte aligned
        assert L.rpe_corr_alt_lookup_dt(one, one, 1, 256, 8, 16, 3, 3, 8, 16, dt, one, null) == -1              # radius 4 only
        assert L.rpe_corr_alt_lookup_dt(one, one, 1, 256, 1, 16, 3, 4, 1, 16, dt, one, null) == -1
        assert L.rpe_corr_alt_lookup_dt(one, null, 1, 256, 8, 16, 3, 4, 8, 16, dt, one, null) == -1
        assert L.rpe_corr_alt_lookup_dt(null, one, 1, 256, 8, 16, 3, 4, 8, 16, dt, one, null) == -1
        assert L.rpe_corr_alt_lookup_dt(one, one, 1, 256, 8, 16, 3, 4, 8, 16, dt, null, null) == -1
        assert L.rpe_corr_alt_lookup_dt(ctypes.c_void_p(20), one, 1, 256, 8, 16, 3, 4, 8, 16, dt, one, null) == -1
        assert L.rpe_corr_alt_lookup_dt(one, one, 1, 256, 8, 16, 3, 4, 8, 15, dt, one, null) == -1              # map_w < w8
        assert L.rpe_corr_alt_lookup_dt(one, one, 1, 256, 8, 16, 3, 4, 7, 16, dt, one, null) == -1              # map_h < h8
    for dt in (1, 3):                                           # a feature_dtype the route does not have, every other argument good
        assert L.rpe_corr_alt_prepare_ex(one, one, 1, 256, 8, 16, 3, dt, one, null) == -1
        assert L.rpe_corr_alt_lookup_dt(one, one, 1, 256, 8, 16, 3, 4, 8, 16, dt, one, null) == -1
    # through a launch list the same checks apply (run_one carries the two kinds)
    from rpe_amd import _lib
    a = _lib.CorrAltLookupDtArgs(16, 16, 1, 256, 8, 16, 3, 4, 8, 15, F16, 16)
    op = _lib.Op(_lib.OP_CORR_ALT_LOOKUP_DT, 0, ctypes.cast(ctypes.pointer(a), ctypes.c_void_p))
    streams, failed = (ctypes.c_void_p * 1)(None), ctypes.c_int(-5)
    assert L.rpe_run_ops(ctypes.pointer(op), 1, streams, 1, ctypes.byref(failed)) == -1 and failed.value == 0
    p = _lib.CorrAltPrepareExArgs(16, 16, 1, 256, 8, 16, 3, 1, 16)
    op = _lib.Op(_lib.OP_CORR_ALT_PREPARE_EX, 0, ctypes.cast(ctypes.pointer(p), ctypes.c_void_p))
    assert L.rpe_run_ops(ctypes.pointer(op), 1, streams, 1, ctypes.byref(failed)) == -1 and failed.value == 0


def test_alt_corr_fp16_config_key(rpe):
    from rpe_amd import raft, synth
    from rpe_amd._lib import RpeError
    with pytest.raises(RpeError):
        raft.RAFT(synth.model_config(64, 96, alt_corr_fp16=True))                                  # needs alternate_corr
    net = raft.RAFT(synth.model_config(64, 96, alternate_corr=True, alt_corr_fp16=True))
    assert net.alt_corr_fp16 is True and net.alternate_corr is True
    assert raft.RAFT(synth.model_config(64, 96, alternate_corr=True)).alt_corr_fp16 is False
    assert raft.RAFT(synth.model_config(64, 96)).alt_corr_fp16 is False
    cfg = synth.model_config(64, 96)
    assert cfg['alt_corr_fp16'] is False and list(cfg)[-1] == 'alt_corr_fp16'
    del cfg['alt_corr_fp16']
    assert raft.RAFT(cfg).alt_corr_fp16 is False
    with pytest.raises(RpeError):
        raft.RAFT(synth.model_config(64, 96, alternate_corr=True, mixed_precision=True))           # stays refused
    with pytest.raises(RpeError):
        raft.RAFT(synth.model_config(64, 96, alternate_corr=True, mixed_precision=True, alt_corr_fp16=True))


def test_alt_corr_fp16_refused_with_the_bf16x3_switches(rpe, monkeypatch):
    from rpe_amd import raft, synth
    from rpe_amd._lib import RpeError
    for switch in ('CORR_BF16X3', 'CONV_BF16X3'):
        monkeypatch.setattr(raft, switch, True)
        with pytest.raises(RpeError):
            raft.RAFT(synth.model_config(64, 96, alternate_corr=True, alt_corr_fp16=True))
        monkeypatch.undo()
