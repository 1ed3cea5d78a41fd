"""CPU: the on-the-fly correlation route (RAFT's alternate_corr; csrc/corr_alt.hip) -- its ABI is declared, bound and exported, its launch
list kinds agree on both sides, its scratch size obeys the stated bounds, and the flag is refused together with mixed_precision."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ('rpe_corr_alt_bytes', 'rpe_corr_alt_prepare', 'rpe_corr_alt_lookup')


def _header():
    return open(os.path.join(ROOT, 'include', 'rpe.h')).read()


def test_alt_abi_declared_bound_exported(rpe):
    from rpe_amd import _lib
    L, header = rpe.lib(), _header()
    for name in NEW:
        assert re.search(r'\b' + name + r'\(', header) and name in _lib.SIGNATURES and hasattr(L, name), name
    assert int(re.search(r'#define RPE_OP_CORR_ALT_PREPARE (\d+)', header).group(1)) == _lib.OP_CORR_ALT_PREPARE == 20
    assert int(re.search(r'#define RPE_OP_CORR_ALT_LOOKUP (\d+)', header).group(1)) == _lib.OP_CORR_ALT_LOOKUP == 21
    assert _lib.LIST_OPS[20] == ('rpe_corr_alt_prepare', _lib.CorrAltPrepareArgs) and _lib.LIST_OPS[21] == ('rpe_corr_alt_lookup', _lib.CorrAltLookupArgs)
    assert ctypes.sizeof(_lib.CorrAltPrepareArgs) == 48 and _lib.CorrAltPrepareArgs.scratch.offset == 40
    assert ctypes.sizeof(_lib.CorrAltLookupArgs) == 48 and _lib.CorrAltLookupArgs.out.offset == 40
    src = open(os.path.join(ROOT, 'robust-pose-estimator_amd', 'csrc', 'oplist.hip')).read()
    for st, kind in (('rpe_corr_alt_prepare_args', 'RPE_OP_CORR_ALT_PREPARE'), ('rpe_corr_alt_lookup_args', 'RPE_OP_CORR_ALT_LOOKUP')):
        assert f'static_assert(sizeof({st}) == 48,' in src and f'case {kind}:' in src


def test_alt_bytes_zero_exactly_where_the_pyramid_is(rpe):
    L = rpe.lib()
    n = 0
    for h8 in (0, 1, 2, 3, 4, 5, 7, 8, 12, 15, 16, 17, 64):
        for w8 in (0, 1, 2, 3, 4, 6, 9, 16, 20, 31, 80):
            for levels in (0, 1, 2, 3, 4, 5):
                for b in (0, 1, 3):
                    pyr = L.rpe_corr_pyramid_bytes_ex(b, h8, w8, levels, 0)
                    alt = L.rpe_corr_alt_bytes(b, 256, h8, w8, levels)
                    assert (alt == 0) == (pyr == 0), (b, h8, w8, levels, alt, pyr)
                    n += pyr != 0
    assert n > 100                                              # (the grid does hold supported geometries)
    for c in (0, -16, 8, 24, 272):                              # channel counts rpe_corr_build refuses
        assert L.rpe_corr_alt_bytes(1, c, 16, 16, 4) == 0
    assert L.rpe_corr_alt_bytes(1, 16, 16, 16, 4) > 0


def test_alt_bytes_bounds(rpe):
    L = rpe.lib()
    pad = int(re.search(r'#define RPE_CORR_ALT_PAD (\d+)', _header()).group(1))
    b, c, h8, w8 = 2, 256, 128, 160
    alt, pyr = L.rpe_corr_alt_bytes(b, c, h8, w8, 4), L.rpe_corr_pyramid_bytes_ex(b, h8, w8, 4, 0)
    assert 0 < 20 * alt < pyr, (alt, pyr)
    for (b, c, h8, w8) in ((2, 256, 128, 160), (1, 256, 8, 16), (3, 256, 12, 20), (1, 16, 17, 19), (32, 256, 64, 80), (5, 48, 9, 23)):
        for levels in (1, 2, 3, 4):
            alt = L.rpe_corr_alt_bytes(b, c, h8, w8, levels)
            if alt == 0:
                assert L.rpe_corr_pyramid_bytes_ex(b, h8, w8, levels, 0) == 0
                continue
            assert alt <= b * c * h8 * w8 * 4 * (1 + 4 / 3) + pad * levels, (b, c, h8, w8, levels, alt)
            assert alt >= b * c * h8 * w8 * 4 * 2                # both maps at level 0 are in it


def test_alt_bad_arguments_return_badarg_without_a_gpu(rpe):
    L = rpe.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)          # never dereferenced: the argument checks fail first
    assert L.rpe_corr_alt_prepare(null, one, 1, 256, 8, 16, 4, one, null) == -1
    assert L.rpe_corr_alt_prepare(one, one, 1, 256, 8, 16, 4, null, null) == -1
    assert L.rpe_corr_alt_prepare(one, one, 1, 24, 8, 16, 4, one, null) == -1
    assert L.rpe_corr_alt_prepare(one, one, 1, 256, 8, 16, 4, ctypes.c_void_p(20), null) == -1      # scratch not 16-byte aligned
    assert L.rpe_corr_alt_lookup(one, one, 1, 256, 8, 16, 4, 3, one, null) == -1                    # radius 4 only
    assert L.rpe_corr_alt_lookup(one, one, 1, 256, 1, 16, 4, 4, one, null) == -1
    assert L.rpe_corr_alt_lookup(one, null, 1, 256, 8, 16, 4, 4, one, null) == -1


def test_alternate_corr_is_f32_only(rpe):
    from rpe_amd import raft, synth
    from rpe_amd._lib import RpeError
    with pytest.raises(RpeError):
        raft.RAFT(synth.model_config(64, 96, alternate_corr=True, mixed_precision=True))
    assert raft.RAFT(synth.model_config(64, 96, alternate_corr=True)).alternate_corr is True
    assert raft.RAFT(synth.model_config(64, 96)).alternate_corr is False
    cfg = synth.model_config(64, 96)
    del cfg['alternate_corr']
    assert raft.RAFT(cfg).alternate_corr is False
