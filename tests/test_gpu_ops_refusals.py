"""GPU: bad arguments to the convolution / flow / stem / instance-norm wrappers of ops.py are refused in Python, as RpeError, before
anything goes to the library (``CountingLib.calls == 0``).  Tiny tensors; every case was refused the same way before the wrappers'
checks were put on shared helpers (ops._f32, ops._opt_slices, ops._conv_desc)."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def t(rpe):
    """Good arguments: batch 1, 8 channels, 4x8 maps (the pyramid: 16x16, the smallest square one with four levels)."""
    from rpe_amd import ops
    torch.manual_seed(0)
    e = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device='cuda')
    r = lambda *s: torch.randn(*s, device='cuda')
    n = types.SimpleNamespace(ops=ops, e=e)
    n.x, n.out, n.half = e(1, 8, 4, 8), e(1, 8, 4, 8), e(1, 4, 4, 8)
    n.vec, n.vec16 = e(8), e(16)
    n.pc, n.pw = ops.PackedConv(r(8, 8, 3, 3), r(8)), ops.PackedWino(r(8, 8, 3, 3), r(8))
    n.p1, n.p1d = ops.PackedConv1x1(r(8, 8, 1, 1), r(8)), ops.PackedWino1d(r(8, 8, 1, 5), r(8))
    n.tiles = ops.lib().rpe_conv_stats_tiles(8, 4, 8, 1)
    n.wtiles = ops.lib().rpe_conv_wino_stats_tiles(4, 8)
    n.w2, n.two = r(2, 8, 3, 3), e(1, 2, 4, 8)
    n.pyr, n.plc = ops.CorrPyramid(1, 16, 16), ops.PackedLookupConv(r(256, 324, 1, 1), r(256))
    n.co, n.cor = e(1, 2, 16, 16), e(1, 256, 16, 16)
    n.ps, n.image, n.sout = ops.PackedStem(r(64, 3, 7, 7)), e(1, 3, 8, 16), e(1, 64, 4, 8)
    n.stiles = ops.lib().rpe_stem_tiles(8, 16, 2)
    n.rec, n.mom = e(1, 8, 2, 3), e(1, 8, 2)
    return n


F64 = torch.float64
CASES = {
    # conv_fused
    'fused-x-dtype': lambda t: t.ops.conv_fused(t.x.double(), t.pc, 0, t.out),
    'fused-x-not-contiguous': lambda t: t.ops.conv_fused(t.e(1, 8, 8, 4).transpose(2, 3), t.pc, 0, t.out),
    'fused-x-channels': lambda t: t.ops.conv_fused(t.half, t.pc, 0, t.out),
    'fused-out-shape': lambda t: t.ops.conv_fused(t.x, t.pc, 0, t.e(1, 8, 4, 4)),
    'fused-out-few-channels': lambda t: t.ops.conv_fused(t.x, t.pc, 1, t.half),
    'fused-out2-few-channels': lambda t: t.ops.conv_fused(t.x, t.pc, 1, t.out, out2=t.half),
    'fused-out-dtype': lambda t: t.ops.conv_fused(t.x, t.pc, 0, t.out.double()),
    'fused-bias-dtype': lambda t: t.ops.conv_fused(t.x, t.pc, 0, t.out, bias=t.vec.double()),
    'fused-bias-not-contiguous': lambda t: t.ops.conv_fused(t.x, t.pc, 0, t.out, bias=t.vec16[::2]),
    'fused-scale-length': lambda t: t.ops.conv_fused(t.x, t.pc, 0, t.out, scale=t.vec16),
    'fused-add-channels': lambda t: t.ops.conv_fused(t.x, t.pc, 0, t.out, add=t.half),
    'fused-stats-shape': lambda t: t.ops.conv_fused(t.x, t.pc, 0, t.out, stats=t.e(1, 8, t.tiles + 1, 3)),
    'fused-stats-dtype': lambda t: t.ops.conv_fused(t.x, t.pc, 0, t.out, stats=t.e(1, 8, t.tiles, 3, dtype=F64)),
    'fused-pre-norm-shape': lambda t: t.ops.conv_fused(t.x, t.pc, 0, t.out, pre_norm=t.e(1, 8, 3)),
    'fused-gate-zr-without-out2': lambda t: t.ops.conv_fused(t.x, t.pc, 2, t.half, hidden=t.half, gate_channels=4),
    'fused-gate-zr-few-hidden': lambda t: t.ops.conv_fused(t.x, t.pc, 2, t.half, out2=t.half, hidden=t.two, gate_channels=4),
    'fused-gate-h-without-zgate': lambda t: t.ops.conv_fused(t.x, t.pc, 3, t.out, hidden=t.out),
    'fused-gate-h-without-hidden': lambda t: t.ops.conv_fused(t.x, t.pc, 3, t.out, zgate=t.out),
    # conv_wino
    'wino-mode': lambda t: t.ops.conv_wino(t.x, t.pw, 4, t.out),
    'wino-x-dtype': lambda t: t.ops.conv_wino(t.x.double(), t.pw, 0, t.out),
    'wino-x-channels': lambda t: t.ops.conv_wino(t.half, t.pw, 0, t.out),
    'wino-out-few-channels': lambda t: t.ops.conv_wino(t.x, t.pw, 0, t.half),
    'wino-out2-shape': lambda t: t.ops.conv_wino(t.x, t.pw, 0, t.out, out2=t.e(1, 8, 4, 4)),
    'wino-residual-few-channels': lambda t: t.ops.conv_wino(t.x, t.pw, 0, t.out, residual=t.half),
    'wino-bias-not-contiguous': lambda t: t.ops.conv_wino(t.x, t.pw, 0, t.out, bias=t.vec16[::2]),
    'wino-stats-type': lambda t: t.ops.conv_wino(t.x, t.pw, 0, t.out, stats=t.e(1, t.wtiles, 8, 3)),
    'wino-stats-shape': lambda t: t.ops.conv_wino(t.x, t.pw, 0, t.out, stats=t.ops.TileMajorStats(t.e(1, t.wtiles + 1, 8, 3))),
    'wino-pre-norm-shape': lambda t: t.ops.conv_wino(t.x, t.pw, 0, t.out, pre_norm=t.e(1, 4, 2)),
    'wino-pre-norm-dtype': lambda t: t.ops.conv_wino(t.x, t.pw, 0, t.out, pre_norm=t.e(1, 8, 2, dtype=F64)),
    # conv1x1, conv_wino1d
    'conv1x1-x-channels': lambda t: t.ops.conv1x1(t.half, t.p1, 0, t.out),
    'conv1x1-out-not-contiguous': lambda t: t.ops.conv1x1(t.x, t.p1, 0, t.e(1, 8, 8, 4).transpose(2, 3)),
    'conv1x1-out-few-channels': lambda t: t.ops.conv1x1(t.x, t.p1, 1, t.half),
    'wino1d-x-dtype': lambda t: t.ops.conv_wino1d(t.x.double(), t.p1d, 0, t.out),
    'wino1d-out-shape': lambda t: t.ops.conv_wino1d(t.x, t.p1d, 0, t.e(1, 8, 8, 8)),
    'wino1d-gate-h-without-hidden': lambda t: t.ops.conv_wino1d(t.x, t.p1d, 3, t.out, zgate=t.out),
    # flow_update, flow_seed
    'flow-update-weight-shape': lambda t: t.ops.flow_update(t.x, t.w2[:, :4].contiguous(), None, t.two, t.two),
    'flow-update-coords-shape': lambda t: t.ops.flow_update(t.x, t.w2, None, t.e(1, 2, 4, 4), t.two),
    'flow-update-flow-out-not-contiguous': lambda t: t.ops.flow_update(t.x, t.w2, None, t.two, t.two, flow_out=t.e(1, 2, 8, 4).transpose(2, 3)),
    'flow-update-dst1-shape': lambda t: t.ops.flow_update(t.x, t.w2, None, t.two, t.two, dst1=t.e(1, 3, 4, 8)),
    'flow-update-dst2-dtype': lambda t: t.ops.flow_update(t.x, t.w2, None, t.two, t.two, dst2=t.two.double()),
    'flow-seed-channels': lambda t: t.ops.flow_seed(t.e(1, 3, 4, 8), coords_out=t.two),
    'flow-seed-dtype': lambda t: t.ops.flow_seed(t.two.double(), coords_out=t.two),
    'flow-seed-coords-out-shape': lambda t: t.ops.flow_seed(t.two, coords_out=t.e(1, 2, 4, 4)),
    'flow-seed-dst2-shape': lambda t: t.ops.flow_seed(t.two, coords_out=t.two, dst2=t.x),
    'flow-seed-dst1-not-contiguous': lambda t: t.ops.flow_seed(t.two, coords_out=t.two, dst1=t.e(1, 2, 4, 16)[..., ::2]),
    # CorrPyramid.lookup_conv1x1
    'lookup-conv-coords-shape': lambda t: t.pyr.lookup_conv1x1(t.two, t.plc, t.cor),
    'lookup-conv-coords-not-contiguous': lambda t: t.pyr.lookup_conv1x1(t.co.transpose(2, 3), t.plc, t.cor),
    'lookup-conv-out-channels': lambda t: t.pyr.lookup_conv1x1(t.co, t.plc, t.cor[:, :128]),
    'lookup-conv-out2-dtype': lambda t: t.pyr.lookup_conv1x1(t.co, t.plc, t.cor, out2=t.cor.double()),
    # stem_conv
    'stem-image-channels': lambda t: t.ops.stem_conv(t.e(1, 2, 8, 16), t.ps, out=t.sout),
    'stem-image-dtype': lambda t: t.ops.stem_conv(t.image.double(), t.ps, out=t.sout),
    'stem-out-shape': lambda t: t.ops.stem_conv(t.image, t.ps, out=t.e(1, 64, 8, 16)),
    'stem-stats-shape': lambda t: t.ops.stem_conv(t.image, t.ps, out=t.sout, stats=t.e(1, 64, t.stiles + 1, 3)),
    'stem-stats-dtype': lambda t: t.ops.stem_conv(t.image, t.ps, out=t.sout, stats=t.e(1, 64, t.stiles, 3, dtype=F64)),
    # instnorm_finalize, instnorm_apply
    'finalize-channels': lambda t: t.ops.instnorm_finalize(t.rec, 32, channels=4),
    'finalize-dtype': lambda t: t.ops.instnorm_finalize(t.rec.double(), 32),
    'finalize-record-size': lambda t: t.ops.instnorm_finalize(t.e(1, 8, 2, 2), 32),
    'finalize-not-contiguous': lambda t: t.ops.instnorm_finalize(t.e(1, 8, 3, 2).transpose(2, 3), 32),
    'apply-moments-shape': lambda t: t.ops.instnorm_apply(t.x, t.e(1, 4, 2)),
    'apply-moments-dtype': lambda t: t.ops.instnorm_apply(t.x, t.mom.double()),
    'apply-records-channels': lambda t: t.ops.instnorm_apply(t.x, t.e(1, 4, 2, 3)),
    'apply-tile-major-channels': lambda t: t.ops.instnorm_apply(t.x, t.ops.TileMajorStats(t.e(1, 2, 4, 3))),
    'apply-residual-shape': lambda t: t.ops.instnorm_apply(t.x, t.mom, residual=t.half),
    'apply-residual-norm-alone': lambda t: t.ops.instnorm_apply(t.x, t.mom, residual_norm=t.mom),
    'apply-residual-norm-shape': lambda t: t.ops.instnorm_apply(t.x, t.mom, residual=t.out, residual_norm=t.e(1, 8, 3)),
    'apply-x-dtype': lambda t: t.ops.instnorm_apply(t.x.double(), t.mom),
}


# case family -> the name the message begins with (conv1x1 and conv_wino1d delegate to conv_fused, and say so), and per case the
# argument (or, for a channel-count mismatch of x, the word "input") that the message names
WRAPPER = {'fused': 'conv_fused', 'wino': 'conv_wino', 'conv1x1': 'conv_fused', 'wino1d': 'conv_fused', 'flow-update': 'flow_update', 'flow-seed': 'flow_seed',
           'lookup-conv': 'corr lookup_conv1x1', 'stem': 'stem_conv', 'finalize': 'instnorm_finalize', 'apply': 'instnorm_apply'}
NAMED = {'x-channels': 'input', 'pre-norm-shape': 'pre_norm', 'pre-norm-dtype': 'pre_norm', 'gate-zr-without-out2': 'out2', 'gate-zr-few-hidden': 'hidden',
         'gate-h-without-zgate': 'zgate', 'gate-h-without-hidden': 'hidden', 'flow-out-not-contiguous': 'flow_out', 'coords-out-shape': 'coords_out',
         'channels': 'channels', 'record-size': 'stats', 'not-contiguous': 'stats', 'dtype': 'stats', 'moments-shape': 'stats', 'moments-dtype': 'stats',
         'records-channels': 'stats', 'tile-major-channels': 'stats', 'residual-norm-alone': 'residual_norm', 'residual-norm-shape': 'residual_norm'}


def _expected(case):
    family = max((f for f in WRAPPER if case.startswith(f + '-')), key=len)
    rest = case[len(family) + 1:]
    if family == 'flow-seed' and rest in ('channels', 'dtype'):
        return WRAPPER[family], 'flow_init'
    return WRAPPER[family], NAMED.get(rest, rest.split('-')[0])


@pytest.mark.parametrize('case', sorted(CASES))
def test_bad_argument_is_refused_before_the_library(rpe, t, case):
    from rpe_amd import _lib
    with _lib.CountingLib() as count:
        with pytest.raises(rpe.RpeError) as refusal:
            CASES[case](t)
    message, (wrapper, argument) = str(refusal.value), _expected(case)
    print(case, '->', message)
    assert count.calls == 0, count.names
    assert message.startswith(wrapper + ':') and argument in message[len(wrapper):], (wrapper, argument, message)
