"""CPU: which descriptors the eight rpe_conv_desc entry points refuse, and with which code, without a GPU -- every rule of each entry
point, and which of RPE_E_BADARG / RPE_E_UNSUPPORTED wins when a descriptor breaks one of each.  Every row is a refusal: the pointers are
fake (never dereferenced, nothing is launched), so the module skips itself where a device exists (a wrongly accepted row must not reach
one).  The packed-size queries are pinned beside them.

Rules that no refused descriptor can isolate are not rows: (h * w) % 4 of the two x3 Winograd kernels follows from w % 4, which they check
first; rpe_conv1x1 and rpe_conv_wino place no 16-byte rule on their destinations / input."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='fake device pointers: only where nothing can be launched')

OK, B, U = 0, -1, -3                                     # RPE_OK, RPE_E_BADARG, RPE_E_UNSUPPORTED
LINEAR, RELU, GATE_ZR, GATE_H, TANH = 0, 1, 2, 3, 4
P, P8, P4 = 0x1000, 0x1008, 0x1004                       # fake pointers: 16-byte aligned | 8-byte only | 4-byte only

BASE = dict(x=P, packed=P, out=P, b=1, cin=16, cout=64, h=8, w=8, mode=RELU)
ZR = dict(mode=GATE_ZR, out2=P, hidden=P, gate_channels=32)          # a complete GATE_ZR / GATE_H descriptor (cout = 64)
GH = dict(mode=GATE_H, hidden=P, zgate=P)


def _absent(*more):
    """The shared presence rule (RPE_E_BADARG), and its precedence over an unsupported kernel size."""
    rows = [({f: None}, B) for f in ('x', 'packed', 'out')] + [({f: 0}, B) for f in ('b', 'cin', 'cout', 'h', 'w')]
    return rows + [(dict(out=None, kh=7, kw=7), B), (dict(w=0, kh=7, kw=7), B)] + list(more)


def _each(fields, code, **with_):
    return [(dict(with_, **{f: P}), code) for f in fields]


def _misaligned(pairs, ptr, stride, **with_):
    """(pointer field, batch-stride field): the pointer off its alignment, and the stride of a present tensor off it."""
    rows = []
    for f, s in pairs:
        rows.append((dict(with_, **{f: ptr}), U))
        if s:
            rows.append((dict(with_, **{f: P, s: stride}), U))
    return rows


GRU, ENC = ('add', 'hidden', 'zgate'), ('scale', 'residual', 'stats', 'pre_norm')
GATE_RULES = [(dict(ZR, out2=None), B), (dict(ZR, hidden=None), B), (dict(ZR, gate_channels=0), B), (dict(ZR, gate_channels=16), B),
              (dict(GH, hidden=None), B), (dict(GH, zgate=None), B)]
X, OUT, OUT2, RES = ('x', 'x_batch_stride'), ('out', 'out_batch_stride'), ('out2', 'out2_batch_stride'), ('residual', 'residual_batch_stride')
ADD, HID, ZG = ('add', 'add_batch_stride'), ('hidden', 'hidden_batch_stride'), ('zgate', 'zgate_batch_stride')


def _wino3x3(cin_bad, odd_w):
    """The three 3x3 Winograd entry points share everything but the channel step, the width rule and the alignment class."""
    return _absent() + [(dict(kh=5, kw=5), U), (dict(kw=1), U), (dict(kh=1), U), (dict(stride=2), U), (dict(cin=cin_bad), U), (dict(h=7), U),
                        (dict(w=odd_w), U), (dict(mode=GATE_ZR), U), (dict(mode=TANH), U), (dict(mode=-1), U),
                        (dict(pre_norm=P, cin=144), U)] + _each(GRU, U)


def _wino1d(cin_bad):
    tensors = (X, ('packed', None), OUT, OUT2, ADD, HID, ZG)
    return _absent((dict(kh=3, kw=3, mode=-1), U), (dict(mode=TANH, scale=P), B)) + [
        (dict(kh=3, kw=3), U), (dict(kh=5, kw=5), U), (dict(kh=1, kw=1), U), (dict(stride=2), U), (dict(cin=cin_bad), U), (dict(w=6), U),
        (dict(mode=-1), B), (dict(mode=TANH), B)] + GATE_RULES + _each(ENC, U) + _misaligned(tensors, P8, 2)


def _conv1x1(extra):
    return _absent() + [(dict(kh=3, kw=3), U), (dict(kw=3), U), (dict(kh=3), U), (dict(stride=2), U), (dict(mode=GATE_ZR), U),
                        (dict(mode=GATE_H), U), (dict(mode=5), U), (dict(mode=-1), U), (dict(h=3, w=2), U), (dict(h=1, w=2), U)
                        ] + _each(GRU + ENC, U) + _misaligned((X, ('packed', None)), P8, 2) + extra


# entry point -> (overrides of BASE that make an accepted descriptor of it, [(further overrides, expected code)])
TABLE = {
    'rpe_conv_fused': (dict(kh=3, kw=3), _absent((dict(kw=2, mode=9), U), (dict(w=6, mode=9), U)) + [
        (dict(kh=0), U), (dict(kh=2), U), (dict(kw=2), U), (dict(kw=7), U), (dict(w=6), U), (dict(x=P8), U), (dict(x_batch_stride=2), U),
        (dict(mode=-1), B), (dict(mode=5), B),
        (dict(mode=TANH, stride=2), U), (dict(mode=TANH, cout=96), U)] + _each(ENC, U, mode=TANH) + GATE_RULES
        + _each(ENC[:3], B, **ZR) + _each(ENC[:3], B, **GH) + [
        (dict(stride=3), U), (dict(pre_norm=P, stride=2), U), (dict(pre_norm=P, kh=1, kw=5), U), (dict(GH, pre_norm=P), U),
        (dict(stride=2, h=7), U), (dict(GH, stride=2), U), (dict(stride=2, kh=5, kw=1), U), (dict(stride=2, kh=3, kw=1), U),
        (dict(stride=2, stats=P, stats_tiles=5), B),                   # one record per 32 output pixels: 1 here
        (dict(scale=P, kh=1, kw=5), U), (dict(stats=P, kh=1, kw=1), U)]),    # encoder epilogues: 3x3 only
    'rpe_conv1x1': (dict(kh=1, kw=1), _conv1x1([(dict(h=8192, w=8192), U)])),                        # 64 hw + 4096 >= 2^32
    'rpe_conv1x1_x3': (dict(kh=1, kw=1), _conv1x1([(dict(mode=TANH), U), (dict(h=16384, w=8192), U),          # 16 hw >= 2^31
                                                   (dict(cin=20, h=8192, w=4096), U)]                         # ragged cin: 64 hw >= 2^31
                                         + _misaligned((OUT, OUT2), P8, 2))),
    'rpe_conv_wino': (dict(kh=3, kw=3), _wino3x3(18, 7) + _misaligned((('packed', None),), P8, 0)
                      + _misaligned((OUT, OUT2, RES), P4, 1)),                                          # 8-byte destinations
    'rpe_conv_wino24': (dict(kh=3, kw=3), _wino3x3(18, 6) + _misaligned((X, OUT, OUT2, RES, ('packed', None)), P8, 2)),
    'rpe_conv_wino_x3': (dict(kh=3, kw=3), _wino3x3(20, 6) + _misaligned((X, OUT, OUT2, RES, ('packed', None)), P8, 2)),
    'rpe_conv_wino1d': (dict(kh=1, kw=5), _wino1d(18)),
    'rpe_conv_wino1d_x3': (dict(kh=5, kw=1), _wino1d(20)),
}
ROWS = [(entry, over, code) for entry, (_, rows) in TABLE.items() for over, code in rows]
assert len(TABLE) == 8 and all(code in (B, U) for _, _, code in ROWS), 'every row must be a refusal'


def _id(row):
    return row[0][4:] + ':' + ','.join(f'{k}={v:#x}' if v in (P, P8, P4) else f'{k}={v}' for k, v in row[1].items())


@pytest.mark.parametrize('row', ROWS, ids=_id)
def test_refused_descriptor_returns_its_code(rpe, row):
    from rpe_amd import _lib
    entry, over, code = row
    fields = {**BASE, **TABLE[entry][0], **over}
    desc = _lib.ConvDesc(**{k: v for k, v in fields.items() if v is not None})
    assert getattr(rpe.lib(), entry)(ctypes.byref(desc), None) == code


@pytest.mark.parametrize('entry', list(TABLE))
def test_null_descriptor_is_badarg(rpe, entry):
    assert getattr(rpe.lib(), entry)(None, None) == B


SHAPES = ((96, 32), (40, 16), (96, 20), (0, 16), (64, 0))
SIZES = {                                                # values of the library before the entry points shared their host side
    'rpe_conv_packed_floats/3/3': (38912, 20480, 38912, 0, 0),
    'rpe_conv_packed_floats/1/5': (22528, 12288, 22528, 0, 0),
    'rpe_conv1x1_packed_floats': (4096, 2048, 4096, 0, 0),
    'rpe_conv1x1_x3_packed_bytes': (24576, 12288, 24576, 0, 0),
    'rpe_conv_wino_packed_floats': (65536, 16384, 40960, 0, 0),
    'rpe_conv_wino24_packed_floats': (98304, 24576, 61440, 0, 0),
    'rpe_conv_wino_x3_packed_bytes': (393216, 98304, 0, 0, 0),                       # (cin = 20: not a multiple of the 16-channel step)
    'rpe_conv_wino1d_packed_floats': (32768, 8192, 20480, 0, 0),
    'rpe_conv_wino1d_x3_packed_bytes': (196608, 98304, 0, 0, 0),
}


@pytest.mark.parametrize('query', list(SIZES))
def test_packed_size_queries(rpe, query):
    name, *khw = query.split('/')
    got = tuple(getattr(rpe.lib(), name)(cout, cin, *map(int, khw)) for cout, cin in SHAPES)
    assert got == SIZES[query]
