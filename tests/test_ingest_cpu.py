"""CPU: the one-call input side -- rpe_ingest_stereo declared, bound and exported with RPE_ABI_MINOR unchanged, every bad-argument
case refused without a GPU, the host classes refusing to run without one, and the resize geometry helper against ResizeStereo's own
arithmetic at the sizes the GPU tests use."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NAME = 'rpe_ingest_stereo'
NONE, MAPS, SHIFT = 0, 1, 2
# (per-eye h, w) -> size (W, H): exact 1/2; non-integer scale with a horizontal crop; scale near 1 with a vertical crop; odd source width
# and an output width that is no multiple of 64
SIZES = [((1024, 1280), (640, 512)), ((1080, 1920), (640, 512)), ((576, 720), (640, 512)), ((301, 413), (200, 120))]


def test_ingest_abi_declared_bound_exported(rpe):
    from rpe_amd import _lib, preprocess
    L = rpe.lib()
    header = open(os.path.join(ROOT, 'include', 'rpe.h')).read()
    assert re.search(r'\bint ' + NAME + r'\(', header) and NAME in _lib.SIGNATURES and hasattr(L, NAME)
    assert int(re.search(r'#define RPE_ABI_MINOR (\d+)', header).group(1)) == 4 == L.rpe_abi_minor()
    assert NAME in re.search(r'added without a new minor.*?\*/', header, re.S).group(0)            # named among the uncounted additions
    for k, v in (('NONE', NONE), ('MAPS', MAPS), ('SHIFT', SHIFT)):
        assert int(re.search(r'#define RPE_INGEST_RECT_' + k + r' (\d+)', header).group(1)) == v == getattr(preprocess, 'RECT_' + k)


def _call(L, **kw):
    one, null = ctypes.c_void_p(16), ctypes.c_void_p(0)               # never dereferenced: the argument checks fail first
    a = dict(frames=one, right=null, n=1, h=64, w=80, bgr=0, user_mask=null, thr=735, rh=32, rw=40, top=0, left=4, oh=32, ow=32, mode=NONE,
             lmx=null, lmy=null, rmx=null, rmy=null, tx=0.0, ty=0.0, limg=one, rimg=one, mask=one, stream=null)
    a.update(kw)
    return L.rpe_ingest_stereo(*a.values())


def test_bad_arguments_return_badarg_without_a_gpu(rpe):
    L = rpe.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    for bad in (dict(frames=null), dict(limg=null), dict(rimg=null), dict(mask=null),                  # null pointers
                dict(n=0), dict(n=-1), dict(h=0), dict(w=-3), dict(n=65536),                           # sizes
                dict(rh=0), dict(rw=-1), dict(oh=0), dict(ow=0), dict(top=-1), dict(left=-1),
                dict(top=1), dict(left=9), dict(oh=33), dict(ow=41),                                   # a crop that does not fit
                dict(mode=3), dict(mode=-1),                                                           # unknown mode
                dict(mode=MAPS), dict(mode=MAPS, lmx=one, lmy=one, rmx=one), dict(mode=MAPS, lmy=one, rmx=one, rmy=one),   # maps missing
                dict(mode=SHIFT, tx=float('nan')), dict(mode=SHIFT, ty=float('nan')),
                dict(limg=ctypes.c_void_p(20)), dict(mask=ctypes.c_void_p(18))):                       # out_w % 4 == 0: 16-byte stores
        assert _call(L, **bad) == -1, bad
    # a reduction whose tile footprint does not fit the LDS is refused as unsupported, not launched
    assert _call(L, h=64 * 40, w=80 * 40) == -3


def test_host_classes_refuse_without_a_gpu(rpe):
    from rpe_amd import _lib, preprocess, trajectory
    assert callable(trajectory.track_host_frames)
    if torch.cuda.is_available():
        return                                                        # (the refusals below are those of a machine without one)
    with pytest.raises(_lib.RpeError):
        preprocess.HostFrameIngest((640, 512))
    with pytest.raises(_lib.RpeError):
        preprocess.ingest_stereo(torch.zeros(2 * 64, 80, 3, dtype=torch.uint8), (40, 32))
    with pytest.raises(_lib.RpeError):
        preprocess.ingest_stereo((torch.zeros(64, 80, 3, dtype=torch.uint8),) * 2, (40, 32), stacked=False)


@pytest.mark.parametrize('hw,size', SIZES)
def test_geometry_is_resize_stereo_s(rpe, hw, size):
    """ingest_geometry against the arithmetic of ResizeStereo.__call__ / _resize_with_crop (dataset/transforms.py:25-39), restated."""
    from rpe_amd import preprocess
    (h, w), rs = hw, preprocess.ResizeStereo(size)
    th, tw = rs.size
    scale = max(th / h, tw / w)
    rh, rw = int(scale * h), int(scale * w)
    want = (rh, rw, int(round((rh - th) / 2.0)), int(round((rw - tw) / 2.0)), th, tw)
    assert preprocess.ingest_geometry(h, w, size) == want
    assert want[2] + th <= rh and want[3] + tw <= rw


def test_geometry_refuses_what_resize_stereo_refuses(rpe):
    from rpe_amd import _lib, preprocess
    # int() truncation can leave the resized image one pixel short of the crop: ResizeStereo refuses (torchvision would zero-pad)
    cases = [(h, w) for h in range(30, 90) for w in range(30, 90) if int(max(32 / h, 40 / w) * h) < 32 or int(max(32 / h, 40 / w) * w) < 40]
    assert cases
    with pytest.raises(_lib.RpeError):
        preprocess.ingest_geometry(*cases[0], (40, 32))
