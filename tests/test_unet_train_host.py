"""CPU: the host side of the TinyUNet training route (csrc/unet_train.hip) -- the size queries, the order of the gradient blob, the
argument checks that answer before anything touches the device, and the route switch's default."""
import ctypes

import pytest
import torch

WIDTHS = (16, 32, 64)


def param_shapes(cin):
    """The documented order (csrc/unet_train_host.h), restated: per encoder stage conv1.weight, conv1.bias, norm.weight, norm.bias,
    conv2.weight, conv2.bias; per decoder stage upconv.weight, upconv.bias, conv1.weight, conv1.bias, norm.weight, norm.bias,
    conv2.weight, conv2.bias; head.weight, head.bias."""
    shapes, c_in = [], cin
    for c in WIDTHS:
        shapes += [(c, c_in, 3, 3), (c,), (c,), (c,), (c, c, 3, 3), (c,)]
        c_in = c
    for c in WIDTHS[:0:-1]:
        c2 = c // 2
        shapes += [(c, c2, 2, 2), (c2,), (c2, c, 3, 3), (c2,), (c2,), (c2,), (c2, c2, 3, 3), (c2,)]
    return shapes + [(1, 16, 1, 1), (1,)]


@pytest.mark.parametrize('cin', [264, 272, 8])
def test_gradient_blob_offsets_follow_the_documented_order(rpe, cin):
    from rpe_amd import ops, unet
    L = rpe.lib()
    shapes = param_shapes(cin)
    assert len(shapes) == ops.UNET_TRAIN_NPARAM == 36
    off = 0
    for k, shape in enumerate(shapes):
        assert L.rpe_unet_train_grad_offset(cin, k) == off, k
        off += int(torch.Size(shape).numel())
    assert L.rpe_unet_train_grad_offset(cin, 36) == off == L.rpe_unet_train_grad_floats(cin)
    assert L.rpe_unet_train_grad_offset(cin, 37) == 0 and L.rpe_unet_train_grad_offset(cin, -1) == 0
    # the module hands its parameters over in that order, and they are all of them
    net = unet.TinyUNet(cin, (352, 352))
    params = unet.train_params(net)
    assert [tuple(p.shape) for p in params] == shapes
    assert {id(p) for p in params} == {id(p) for p in net.parameters()}
    assert L.rpe_unet_train_grad_floats(cin) == sum(p.numel() for p in net.parameters())


def test_workspace_size_is_monotone_and_refuses_small_grids(rpe):
    L = rpe.lib()
    q = L.rpe_unet_train_workspace_bytes
    assert q(1, 264, 44, 44, 352, 352) > 0
    for h8, w8 in ((43, 44), (44, 43), (43, 43), (8, 8), (0, 44)):
        assert q(1, 264, h8, w8, 352, 352) == 0, (h8, w8)
    assert q(0, 264, 44, 44, 352, 352) == 0 and q(1, 0, 44, 44, 352, 352) == 0 and q(1, 260, 44, 44, 352, 352) == 0
    assert q(1, 264, 44, 44, 0, 352) == 0
    sizes = [q(n, 264, 44, 44, 352, 352) for n in (1, 2, 4, 16)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4
    grids = [q(2, 272, s, s + 8, 512, 640) for s in range(44, 81, 3)]
    assert grids == sorted(grids) and len(set(grids)) == len(grids)
    assert q(2, 272, 64, 80, 512, 640) > q(2, 264, 64, 80, 512, 640)
    # the saved activations of one row at 80x64 are a few MB: the query is in bytes, not floats
    assert 4 * 2 * 16 * 78 * 62 < q(1, 264, 64, 80, 512, 640) < 64 << 20


def test_bad_arguments_return_status_without_a_gpu(rpe):
    L = rpe.lib()
    one, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    src = (ctypes.c_void_p * 1)(16)
    ch = (ctypes.c_int * 1)(264)
    bs = (ctypes.c_longlong * 1)(264 * 44 * 44)
    prm = (ctypes.c_void_p * 36)(*([16] * 36))
    st = (ctypes.c_void_p * 5)(*([16] * 5))
    f5 = (ctypes.c_float * 5)(*([0.1] * 5))
    fwd = lambda **k: L.rpe_unet_train_forward(k.get('src', src), k.get('ch', ch), k.get('bs', bs), k.get('nsrc', 1), k.get('prm', prm), st, st, None,
                                               f5, f5, 31, k.get('n', 1), k.get('h8', 44), 44, 352, 352, 0, k.get('out', one), k.get('ws', one), null)
    assert fwd(out=null) == -1 and fwd(ws=null) == -1 and fwd(n=0) == -1 and fwd(nsrc=5) == -1 and fwd(src=None) == -1
    assert fwd(prm=(ctypes.c_void_p * 36)(*([16] * 35 + [None]))) == -1
    assert fwd(bs=(ctypes.c_longlong * 1)(44 * 44)) == -1                    # rows would overlap
    assert fwd(h8=43) == -3                                                  # below the 44x44 grid
    assert fwd(ch=(ctypes.c_int * 1)(260), bs=bs) == -3                      # channels % 8
    bwd = lambda **k: L.rpe_unet_train_backward(k.get('g', one), k.get('out', one), src, ch, bs, 1, prm, 31, 1, k.get('h8', 44), 44, 352, 352,
                                                k.get('sigmoid', 0), k.get('gp', one), null, one, null)
    assert bwd(g=null) == -1 and bwd(gp=null) == -1 and bwd(out=null, sigmoid=1) == -1 and bwd(h8=40) == -3


def test_the_route_is_off_by_default_and_then_never_touches_the_training_kernels(rpe, monkeypatch):
    """unet.TRAIN_HIP is False: TinyUNet.forward in train mode runs forward_train on torch ops (here on the CPU) and makes no library
    call; PoseNet leaves the heads' own switch alone unless config['train_heads_hip'] asks."""
    from rpe_amd import _lib, ops, pose_net, synth, unet
    assert unet.TRAIN_HIP is False and unet.TinyUNet.train_hip is None

    def refuse(*a, **k):
        raise AssertionError('the training kernels were called with the route off')
    monkeypatch.setattr(ops, 'unet_train_forward', refuse)
    monkeypatch.setattr(ops, 'unet_train_backward', refuse)
    torch.manual_seed(0)
    net = unet.TinyUNet(8, (352, 352)).train()
    x = torch.randn(2, 8, 44, 44)
    with _lib.CountingLib() as counter:
        y = net(x)
        y.sum().backward()
    assert counter.calls == 0 and tuple(y.shape) == (2, 1, 352, 352)
    assert all(p.grad is not None for p in net.parameters())
    assert torch.equal(y, net.forward_train(x))              # (batch statistics: the running state does not enter)
    off = pose_net.PoseNet(synth.model_config(352, 352))
    on = pose_net.PoseNet(dict(synth.model_config(352, 352), train_heads_hip=True))
    assert not off.train_heads_hip and off.weight_head_2d[0].train_hip is None and off.weight_head_3d[0].train_hip is None
    assert on.train_heads_hip and on.weight_head_2d[0].train_hip is True and on.weight_head_3d[0].train_hip is True
    # with the switch on and no GPU the route fails loudly instead of falling back to torch ops
    monkeypatch.undo()
    if not torch.cuda.is_available():
        net.train_hip = True
        with pytest.raises(rpe.RpeError):
            net(x)


@pytest.mark.parametrize('n,cin,h8,w8', [(1, 264, 44, 44), (3, 272, 45, 47), (3, 264, 52, 60), (2, 8, 64, 80)])
def test_workspace_offsets_follow_the_plan(rpe, n, cin, h8, w8):
    """rpe_unet_train_workspace_offset / _extent: 46 buffers in the order they lie in memory, each on a multiple of 64 floats, each ending
    where the next begins (rounded up to 64 floats: no overlap and no gap the plan does not make), the last inside the workspace."""
    from rpe_amd import ops
    L = rpe.lib()
    assert len(ops.UNET_TRAIN_WS_NAMES) == len(set(ops.UNET_TRAIN_WS_NAMES)) == 46
    ext = (ctypes.c_int * 4)()
    offs, floats = [], []
    for k, name in enumerate(ops.UNET_TRAIN_WS_NAMES):
        offs.append(L.rpe_unet_train_workspace_offset(n, cin, h8, w8, k))
        assert L.rpe_unet_train_workspace_extent(n, cin, h8, w8, k, ext) == 0
        rows, c, h, w = ext
        assert rows == (1 if name.startswith(('mean', 'invstd')) else 32 if name == 'wpart' else n) and min(c, h, w) >= 1, name
        floats.append(rows * c * h * w * (2 if name == 'wpart' else 1))
    assert offs[0] == 0 and all(o % 64 == 0 for o in offs)
    assert all(b > a for a, b in zip(offs, offs[1:]))
    assert all(a + (f + 63) // 64 * 64 == b for a, f, b in zip(offs, floats, offs[1:]))
    assert 4 * (offs[-1] + floats[-1]) + 256 <= L.rpe_unet_train_workspace_bytes(n, cin, h8, w8, 8 * h8, 8 * w8)
    # a few extents, from the architecture: valid 3x3 convolutions, 2x2 pooling, the head map
    shape = lambda name: (L.rpe_unet_train_workspace_extent(n, cin, h8, w8, ops.UNET_TRAIN_WS_NAMES.index(name), ext), tuple(ext))[1]
    assert shape('a1.0') == (n, 16, h8 - 2, w8 - 2) and shape('skip.0') == (n, 16, h8 - 4, w8 - 4)
    assert shape('pool.0') == (n, 16, (h8 - 4) // 2, (w8 - 4) // 2) and shape('mean.4') == (1, 16, 1, 1)
    assert shape('hm') == shape('g_hm') and shape('hm')[1] == 1 and shape('wpart') == (32, max(16 * cin, 64 * 64) * 9, 1, 1)


def test_workspace_offset_refuses_what_the_plan_does_not_hold(rpe):
    L = rpe.lib()
    none = ctypes.c_size_t(-1).value
    q = L.rpe_unet_train_workspace_offset
    ext = (ctypes.c_int * 4)()
    assert q(1, 264, 44, 44, 45) not in (0, none)
    for args in ((1, 264, 44, 44, 46), (1, 264, 44, 44, -1), (1, 264, 43, 44, 0), (1, 264, 44, 43, 0), (1, 264, 8, 8, 3), (0, 264, 44, 44, 0),
                 (1, 260, 44, 44, 0), (1, 0, 44, 44, 0)):
        assert q(*args) == none, args
        assert L.rpe_unet_train_workspace_extent(*args, ext) in (-1, -3), args
    assert L.rpe_unet_train_workspace_extent(1, 264, 44, 44, 46, ext) == -1 and L.rpe_unet_train_workspace_extent(1, 264, 43, 44, 0, ext) == -3
    assert L.rpe_unet_train_workspace_extent(1, 264, 44, 44, 0, None) == -1
