"""GPU: RAFT's ``pad_maps`` -- the update loop on the tuned kernels over zero-padded maps at 1/8 map sizes they refuse.

Kernel level: every valid-extent entry point (rpe_conv_wino_v, rpe_conv_wino24_v, rpe_conv_wino1d_v with its three epilogues on both axes,
rpe_conv1x1_v, rpe_stem_conv_v, rpe_conv3x3_to2_flow_v) on a 12 x 16 map with the valid extent 11 x 13 (an odd last row, a quad that
straddles the extent), batch 2, the channel counts of the real layers, outputs pre-filled with NaN: inside the extent the bits of the plain
entry point on the same zero-padded input, outside it exactly zero.  The pitched lookups, up-sampling and rectangle copy against their
dense forms.

Loop level: images 136 x 144 (grid 17 x 18: odd rows, rows of 4.5 quads) and 128 x 144 (16 x 18: even rows, partial quad).  The issue's
88 x 104 / 96 x 104 have 11- / 12-row grids whose fourth correlation level would be 1 x 1, which the pyramid (and the oracle's sampler)
refuse; 17 x 18 is the smallest grid with four levels, an odd height and w8 % 4 != 0.  Bars: those of
tests/test_gpu_pipeline.py::test_map_sizes_the_tuned_kernels_refuse_run_on_the_generic_kernel (flow 1e-3 px, hidden 5e-3), and against
float64 truth at most 1.5x the generic route's own error (both routes are f32 sums of the same products in another order).

Measured on an MI355X: see NOTES.md, "Padded update loop"."""
import pytest
import torch

from oracle import pose_net as opn
from oracle import raft as oraft

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FLOW_BAR, HIDDEN_BAR = 1e-3, 5e-3           # test_map_sizes_the_tuned_kernels_refuse_run_on_the_generic_kernel's
B, MH, MW, HV, WV = 2, 12, 16, 11, 13
NAN = float('nan')


def _padded_input(c, gen, scale=1.0):
    x = torch.zeros(B, c, MH, MW, device=DEV)
    x[:, :, :HV, :WV] = scale * torch.randn(B, c, HV, WV, generator=gen, device=DEV)
    return x


def _check(name, got, want):
    """Inside the valid extent the plain kernel's bits; outside exactly zero (no NaN, no act(bias))."""
    assert torch.equal(got[:, :, :HV, :WV], want[:, :, :HV, :WV]), f'{name}: valid region differs from the plain kernel'
    pad = got.clone()
    pad[:, :, :HV, :WV] = 0
    assert torch.equal(pad, torch.zeros_like(pad)), f'{name}: padding is not exactly zero (max |.| {float(pad.abs().nan_to_num(1e9).max()):.3g})'
    outside = want.clone()
    outside[:, :, :HV, :WV] = 0
    return float(outside.abs().max())       # what the plain kernel leaves in the padding


@pytest.fixture(scope='module')
def gen(rpe):
    g = torch.Generator(device=DEV)
    g.manual_seed(77)
    return g


@pytest.mark.parametrize('kind', ['wino', 'wino24'])
@pytest.mark.parametrize('cin,cout,two', [(256, 192, False), (128, 64, False), (256, 126, True), (128, 256, False)])
def test_winograd_3x3_valid_extent(rpe, gen, kind, cin, cout, two):
    from rpe_amd import ops
    w = torch.randn(cout, cin, 3, 3, generator=gen, device=DEV) / (3 * cin ** 0.5)
    bias = 0.5 + torch.rand(cout, generator=gen, device=DEV)                    # relu(bias) > 0: a leak would show
    pw = (ops.PackedWino if kind == 'wino' else ops.PackedWino24)(w, bias)
    x = _padded_input(cin, gen)
    want = ops.conv_wino(x, pw, ops.CONV_RELU, torch.empty(B, cout, MH, MW, device=DEV))
    out = torch.full((B, cout, MH, MW), NAN, device=DEV)
    out2 = torch.full((B, cout + 2, MH, MW), NAN, device=DEV) if two else None
    ops.conv_wino(x, pw, ops.CONV_RELU, out, out2=None if out2 is None else out2[:, :cout], valid=(HV, WV))
    assert _check(kind, out, want) > 0
    if two:
        _check(kind + ' out2', out2[:, :cout], want)
        assert bool(out2[:, cout:].isnan().all())                                # channels behind the slice untouched
    # the whole map as the valid extent IS the plain launch
    assert torch.equal(ops.conv_wino(x, pw, ops.CONV_RELU, torch.empty_like(want), valid=(MH, MW)), want)


@pytest.mark.parametrize('vert', [False, True])
def test_gru_gate_epilogues_valid_extent(rpe, gen, vert):
    """z | r and q of one GRU half with non-zero bias and a non-zero context term: sigmoid / tanh of those would fill the padding."""
    from rpe_amd import ops
    c = 128
    shape = (5, 1) if vert else (1, 5)
    wzr = torch.randn(2 * c, 2 * c, *shape, generator=gen, device=DEV) / (5 * 2 * c) ** 0.5
    wq = torch.randn(c, 2 * c, *shape, generator=gen, device=DEV) / (5 * 2 * c) ** 0.5
    pzr, pq = ops.PackedWino1d(wzr), ops.PackedWino1d(wq)
    hx = _padded_input(2 * c, gen)
    ctx_zr = torch.randn(B, 2 * c, MH, MW, generator=gen, device=DEV) + 0.7     # non-zero in the padding too (the hoisted term's bias)
    ctx_q = torch.randn(B, c, MH, MW, generator=gen, device=DEV) - 0.6
    bzr, bq = torch.rand(2 * c, generator=gen, device=DEV) + 0.3, torch.rand(c, generator=gen, device=DEV) + 0.3

    def half(valid, fill):
        z = torch.full((B, c, MH, MW), fill, device=DEV)
        rhx = torch.full((B, 2 * c, MH, MW), fill, device=DEV)
        rhx[:, c:] = hx[:, c:]
        hnew = torch.full((B, c, MH, MW), fill, device=DEV)
        ops.conv_wino1d(hx, pzr, ops.CONV_GATE_ZR, z, out2=rhx[:, :c], add=ctx_zr, hidden=hx[:, :c], gate_channels=c, bias=bzr, valid=valid)
        zin = z if valid is None else z.nan_to_num(0.0)
        rin = rhx if valid is None else rhx.nan_to_num(0.0)
        ops.conv_wino1d(rin, pq, ops.CONV_GATE_H, hnew, add=ctx_q, hidden=hx[:, :c], zgate=zin, bias=bq, valid=valid)
        lin = torch.full((B, c, MH, MW), fill, device=DEV)
        ops.conv_wino1d(hx, pq, ops.CONV_LINEAR, lin, bias=bq, valid=valid)
        return z, rhx[:, :c], hnew, lin
    want, got = half(None, 0.0), half((HV, WV), NAN)
    for name, g, w_ in zip(('z', 'r*h', 'h', 'linear'), got, want):
        leak = _check(f'wino1d {name} vert={vert}', g, w_)
        assert leak > 0 or name in ('r*h', 'h'), name                             # (r * 0 and (1 - z) 0 + z tanh(.) with the plain z)


def test_conv1x1_valid_extent(rpe, gen):
    from rpe_amd import ops
    w = torch.randn(256, 324, 1, 1, generator=gen, device=DEV) / 18
    bias = 0.5 + torch.rand(256, generator=gen, device=DEV)
    layer = ops.Conv1x1(w, bias)
    x = _padded_input(324, gen)
    want = ops.conv1x1(x, layer.gemm, ops.CONV_RELU, torch.empty(B, 256, MH, MW, device=DEV))
    out = torch.full((B, 256, MH, MW), NAN, device=DEV)
    layer(x, ops.CONV_RELU, out, valid=(HV, WV))
    assert _check('conv1x1', out, want) > 0
    assert torch.equal(layer(x, ops.CONV_RELU, torch.empty_like(want)), want)   # (and the small-launch route agrees with the GEMM, as ever)


def test_convf1_and_flow_update_valid_extent(rpe, gen):
    from rpe_amd import ops
    w = torch.randn(128, 2, 7, 7, generator=gen, device=DEV) / 10
    bias = 0.5 + torch.rand(128, generator=gen, device=DEV)
    ps = ops.PackedStem(w)
    flow = _padded_input(2, gen, 3.0)
    kw = dict(bias=bias, relu=True, div=1.0, mul=1.0, sub=0.0)
    want = ops.stem_conv(flow, ps, out=torch.empty(B, 128, MH, MW, device=DEV), **kw)
    out = ops.stem_conv(flow, ps, out=torch.full((B, 128, MH, MW), NAN, device=DEV), valid=(HV, WV), **kw)
    assert _check('convf1', out, want) > 0
    # flow head output layer + coords bookkeeping (both kernels: one pixel per thread here, four per thread from 256 workgroups on)
    for b in (B, 256):
        x = torch.zeros(b, 256, MH, MW, device=DEV)
        x[:, :, :HV, :WV] = torch.rand(b, 256, HV, WV, generator=gen, device=DEV)
        w2 = torch.randn(2, 256, 3, 3, generator=gen, device=DEV) / 48
        b2 = torch.tensor([0.4, -0.3], device=DEV)
        grid = torch.stack(torch.meshgrid(torch.arange(MH, device=DEV), torch.arange(MW, device=DEV), indexing='ij')[::-1]).float()[None].repeat(b, 1, 1, 1)
        coords = grid.clone()
        coords[:, :, :HV, :WV] += torch.randn(b, 2, HV, WV, generator=gen, device=DEV)
        f = lambda fill, ch=2: torch.full((b, ch, MH, MW), fill, device=DEV)
        c_want, fl_want = f(0.0), f(0.0)
        ops.flow_update(x, w2, b2, coords, c_want, flow_out=fl_want)
        c_got, fl_got, d1, d2 = f(NAN), f(NAN), f(NAN, 6), f(NAN, 4)
        ops.flow_update(x, w2, b2, coords, c_got, flow_out=fl_got, dst1=d1[:, 4:], dst2=d2[:, 2:], valid=(HV, WV))
        assert _check('flow', fl_got, fl_want) > 0
        assert torch.equal(d1[:, 4:], fl_got) and torch.equal(d2[:, 2:], fl_got) and bool(d1[:, :4].isnan().all())
        assert torch.equal(c_got[:, :, :HV, :WV], c_want[:, :, :HV, :WV])
        pad = (c_got - grid)
        pad[:, :, :HV, :WV] = 0
        assert torch.equal(pad, torch.zeros_like(pad))                            # coords stay the grid outside the extent


@pytest.mark.parametrize('alt', [False, True])
def test_pitched_lookup_upsampling_and_copy(rpe, gen, alt):
    from rpe_amd import ops
    h8, w8, mh, mw, c = 17, 18, 18, 20, 256
    f1, f2 = (torch.randn(B, c, h8, w8, generator=gen, device=DEV) for _ in range(2))
    pyr = ops.AltCorr(B, c, h8, w8, device=DEV) if alt else ops.CorrPyramid(B, h8, w8, device=DEV)
    pyr.build(f1, f2)
    coords = torch.stack(torch.meshgrid(torch.arange(h8, device=DEV), torch.arange(w8, device=DEV), indexing='ij')[::-1]).float()[None].repeat(B, 1, 1, 1)
    coords = coords + 2.5 * torch.randn(B, 2, h8, w8, generator=gen, device=DEV)
    want = pyr.lookup(coords)
    cpad = torch.full((B, 2, mh, mw), NAN, device=DEV)                           # nothing outside the rectangle is read ...
    ops.copy_rect(coords, cpad, h8, w8)
    out = torch.full((B, 324, mh, mw), 7.0, device=DEV)
    pyr.lookup(cpad, out=out, map_size=(mh, mw))
    assert torch.equal(out[:, :, :h8, :w8], want)
    out[:, :, :h8, :w8] = 7.0
    assert bool((out == 7.0).all())                                              # ... or written
    if alt:
        return
    flow, mask = torch.randn(B, 2, h8, w8, generator=gen, device=DEV), torch.randn(B, 576, h8, w8, generator=gen, device=DEV)
    fp, mp = torch.zeros(B, 2, mh, mw, device=DEV), torch.full((B, 576, mh, mw), NAN, device=DEV)
    ops.copy_rect(flow, fp, h8, w8), ops.copy_rect(mask, mp, h8, w8)
    assert torch.equal(ops.upsample_convex(fp, mp, size=(h8, w8)), ops.upsample_convex(flow, mask))
    wide = torch.randn(B, 8, mh, mw, generator=gen, device=DEV)
    crop = ops.copy_rect(wide[:, 2:5], torch.empty(B, 3, h8, w8, device=DEV), h8, w8)      # a channel slice out of a padded map
    assert torch.equal(crop, wide[:, 2:5, :h8, :w8])


# ------------------------------------------------------------------------------------------------------------------ loop level
ITERS = 4


@pytest.fixture(scope='module')
def nets(rpe):
    from rpe_amd import raft, synth
    cfg = synth.model_config(136, 144, iters=ITERS)
    off = synth.init_synthetic_weights(raft.RAFT(cfg)).eval().to(DEV)
    on = raft.RAFT(dict(cfg, pad_maps=True)).eval().to(DEV)
    on.load_state_dict(off.state_dict())
    om = oraft.RAFT(cfg)
    om.load_state_dict({k: v.cpu() for k, v in off.state_dict().items()})
    om.eval()
    return dict(off=off, on=on, oracle=om, synth=synth, raft=raft)


@pytest.mark.parametrize('h,w', [(136, 144), (128, 144)])
def test_forward_against_the_generic_route_the_oracle_and_float64(nets, monkeypatch, h, w):
    import copy
    fr = nets['synth'].stereo_frames(31, 1, h, w)
    i1, i2 = fr['image1l'], fr['image2l']
    with torch.no_grad():
        oflow, ohid, _ = nets['oracle'](i1.clone(), i2.clone(), iters=ITERS)
        # float64 truth: the oracle in double, its own .float() casts (feature maps, lookup output) made casts to double for this one call
        o64 = copy.deepcopy(nets['oracle']).double()
        monkeypatch.setattr(torch.Tensor, 'float', lambda t: t.double())
        tflow, thid, _ = o64(i1.double(), i2.double(), iters=ITERS)
        monkeypatch.undo()
        assert tflow[-1].dtype == thid.dtype == torch.float64
    res = {}
    for name in ('off', 'on'):
        flows, hid, _ = nets[name](i1.to(DEV), i2.to(DEV))
        assert flows[-1].shape == (1, 2, h, w) and hid.shape == (1, 128, h // 8, w // 8) and hid.is_contiguous()
        res[name] = (flows[-1].cpu(), hid.cpu())
    ws = list(nets['on']._ws.values())[-1]                                        # (the workspace of the pass just run)
    assert ws['valid'] == (h // 8, w // 8) and tuple(ws['hx'].shape[-2:]) == nets['raft'].padded_size(h // 8, w // 8)
    d_route = float((res['on'][0] - res['off'][0]).abs().max()), float((res['on'][1] - res['off'][1]).abs().max())
    d_or = float((res['on'][0] - oflow[-1]).abs().max()), float((res['on'][1] - ohid).abs().max())
    e = {n: (float((res[n][0].double() - tflow[-1]).abs().max()), float((res[n][1].double() - thid).abs().max())) for n in res}
    print(f'{h}x{w}: pad_maps vs generic flow {d_route[0]:.2e} px hidden {d_route[1]:.2e}; vs oracle {d_or[0]:.2e} / {d_or[1]:.2e}; '
          f'vs float64: flow on {e["on"][0]:.3e} off {e["off"][0]:.3e} (ratio {e["on"][0] / e["off"][0]:.2f}), '
          f'hidden on {e["on"][1]:.3e} off {e["off"][1]:.3e} (ratio {e["on"][1] / e["off"][1]:.2f})')
    assert d_route[0] < FLOW_BAR and d_route[1] < HIDDEN_BAR and d_or[0] < FLOW_BAR and d_or[1] < HIDDEN_BAR
    assert e['on'][0] <= 1.5 * e['off'][0] and e['on'][1] <= 1.5 * e['off'][1]
    # the invariant, after a pass: every map a tuned kernel reads is exactly zero outside the content
    h8, w8 = ws['valid']
    for k in ('hx', 'rhx', 'cat', 'corr', 'flow', 'inp'):
        t = ws[k].clone()
        t[:, :, :h8, :w8] = 0
        assert torch.equal(t, torch.zeros_like(t)), k


def _routes(nets, **kw):
    raft = nets['raft']
    old = {k: getattr(raft, k) for k in kw}
    for k, v in kw.items():
        setattr(raft, k, v)
    return old


def test_dispatch_routes_batch_rows_and_warm_start(nets):
    raft = nets['raft']
    fr = nets['synth'].stereo_frames(32, 3, 136, 144)
    i1, i2 = fr['image1l'].to(DEV), fr['image2l'].to(DEV)
    on, off = nets['on'], nets['off']
    outs = {}
    for name, sw in (('launch by launch', dict(FRAME_OPLISTS=False, LOOP_OPLIST=False)), ('launch list', dict(FRAME_OPLISTS=False, LOOP_OPLIST=True)),
                     ('recorded', dict(FRAME_OPLISTS=True, LOOP_OPLIST=True)), ('replayed', dict(FRAME_OPLISTS=True, LOOP_OPLIST=True))):
        old = _routes(nets, **sw)
        try:
            outs[name] = on(i1, i2, ret_lowres=True)
        finally:
            _routes(nets, **old)
    ref = outs['launch by launch']
    for name, o in outs.items():
        assert torch.equal(o[0][-1], ref[0][-1]) and torch.equal(o[1], ref[1]) and torch.equal(o[3], ref[3]), name
    assert ref[3].shape == (3, 2, 17, 18) and ref[3].is_contiguous()
    # a row's result does not depend on its batch
    one = on(i1[1:2], i2[1:2], ret_lowres=True)
    assert torch.equal(one[0][-1], ref[0][-1][1:2]) and torch.equal(one[1], ref[1][1:2]) and torch.equal(one[3], ref[3][1:2])
    # warm start: runs, and matches the generic route to the same bar
    init = ref[3].clone()
    warm_on, warm_off = on(i1, i2, flow_init=init, ret_lowres=True), off(i1, i2, flow_init=init, ret_lowres=True)
    d = float((warm_on[0][-1] - warm_off[0][-1]).abs().max()), float((warm_on[1] - warm_off[1]).abs().max())
    print(f'warm start, pad_maps vs generic: flow {d[0]:.2e} px, hidden {d[1]:.2e}')
    assert d[0] < FLOW_BAR and d[1] < HIDDEN_BAR and not torch.equal(warm_on[0][-1], ref[0][-1])
    # the module switch does what the config key does
    old = _routes(nets, PAD_MAPS=True)
    try:
        sw = off(i1, i2)
    finally:
        _routes(nets, **old)
    assert torch.equal(sw[0][-1], ref[0][-1]) and torch.equal(sw[1], ref[1])


def test_tuned_sizes_are_untouched_by_the_flag(nets, rpe):
    """128 x 192 images (grid 16 x 24, which the tuned kernels take; the issue's 64 x 96 has an 8 x 12 grid without a fourth pyramid level):
    identical outputs and identical launch name lists with the flag on and off."""
    from rpe_amd import _lib
    fr = nets['synth'].stereo_frames(33, 1, 128, 192)
    i1, i2 = fr['image1l'].to(DEV), fr['image2l'].to(DEV)
    old = _routes(nets, FRAME_OPLISTS=False, LOOP_OPLIST=False)
    try:
        got = {}
        for name in ('off', 'on'):
            nets[name](i1, i2)                                                    # (packings are made on first use)
            with _lib.CountingLib() as count:
                out = nets[name](i1, i2)
            got[name] = (out, list(count.names))
    finally:
        _routes(nets, **old)
    assert torch.equal(got['on'][0][0][-1], got['off'][0][0][-1]) and torch.equal(got['on'][0][1], got['off'][0][1])
    assert got['on'][1] == got['off'][1] and not any(n.endswith('_v') or n == 'rpe_copy_rect' for n in got['on'][1])


def test_posenet_at_352x360(rpe, monkeypatch):
    """2 pairs, 12 iterations through PoseNet.infer.  Flow and hidden state of its RAFT against the CPU oracle with the existing odd-size
    test's bars (as that test, on oracle.flow: the oracle's TinyUNet cannot run a 44 x 45 grid -- its centre crop needs even sizes -- so
    the oracle has no infer at this size); the pose against the flag-off pass with the pipeline test's pose bar.  And no rpe_conv_direct
    call from the update loop: every such call of the flag-on pass is made inside an encoder pass, and the encoders make as many as in
    the flag-off pass."""
    from rpe_amd import _lib, pose_net, raft, synth
    h, w = 352, 360
    cfg = synth.model_config(h, w, iters=12, lbgfs_iters=8)
    off = synth.init_synthetic_weights(pose_net.PoseNet(cfg)).eval().to(DEV)
    on = pose_net.PoseNet(dict(cfg, pad_maps=True)).eval().to(DEV)
    on.load_state_dict(off.state_dict())
    om = opn.PoseNet(cfg)
    om.load_state_dict({k: v.cpu() for k, v in off.state_dict().items()})
    om.eval()
    fr = synth.stereo_frames(6, 2, h, w)
    a = synth.infer_args(fr)
    with torch.no_grad():
        oflows, ohid, _ = om.flow(fr['image1l'], fr['image2l'])
    ga = {k: v.to(DEV) for k, v in a.items()}
    state = dict(count=None, enc=0)
    forward = raft.BasicEncoder.forward

    def counted_forward(self, *args, **kw):
        before = len(state['count'].names)
        out = forward(self, *args, **kw)
        state['enc'] += sum(n == 'rpe_conv_direct' for n in state['count'].names[before:])
        return out
    res = {}
    for name, model in (('on', on), ('off', off)):
        for _ in range(4):                                                        # (packings; recordings are made, or given up on, by now)
            model.infer(**ga)
        monkeypatch.setattr(raft.BasicEncoder, 'forward', counted_forward)
        with _lib.CountingLib() as count:
            state.update(count=count, enc=0)
            got = model.infer(**ga)
        monkeypatch.setattr(raft.BasicEncoder, 'forward', forward)
        res[name] = (got, sum(n == 'rpe_conv_direct' for n in count.names), state['enc'])
    flows, hid, _ = on.flow(fr['image1l'].to(DEV), fr['image2l'].to(DEV))
    assert list(on.flow._ws.values())[-1]['valid'] == (44, 45)
    d, dh = float((flows[-1].cpu() - oflows[-1]).abs().max()), float((hid.cpu() - ohid).abs().max())
    pose_d = float((res['on'][0].data - res['off'][0].data).abs().max())
    print(f'352x360: flow vs oracle {d:.2e} px, hidden {dh:.2e}, pose on vs off {pose_d:.2e}; rpe_conv_direct calls per infer (all / inside the encoders): '
          f'pad_maps {res["on"][1]} / {res["on"][2]}, generic {res["off"][1]} / {res["off"][2]}')
    assert d < FLOW_BAR and dh < HIDDEN_BAR and pose_d < 1e-5
    assert res['on'][2] == res['off'][2] > 0                                      # the encoders stay on the generic route, unchanged
    assert res['on'][1] == res['on'][2] and res['off'][1] > res['off'][2]         # the update loop: none with the flag, some without


def test_flag_off_calls_the_wrappers_as_before(nets, monkeypatch):
    """With the flag off the host code makes the calls it always made: wrappers with the signatures of before this route (bench.py --full
    puts such timing wrappers around CorrPyramid.lookup, conv_fused and conv_wino) still take them, at a tuned size and at one the tuned
    kernels refuse, on both dispatch routes."""
    from rpe_amd import ops
    real = dict(lookup=ops.CorrPyramid.lookup, stem=ops.stem_conv, flow=ops.flow_update)
    monkeypatch.setattr(ops.CorrPyramid, 'lookup', lambda self, coords, out=None, prepare=False: real['lookup'](self, coords, out, prepare))
    monkeypatch.setattr(ops, 'stem_conv', lambda image, ps, bias=None, scale=None, relu=True, stats=False, div=255.0, mul=2.0, sub=1.0, out=None, prepare=False:
                        real['stem'](image, ps, bias, scale, relu, stats, div, mul, sub, out, prepare))
    monkeypatch.setattr(ops, 'flow_update', lambda x, weight, bias, coords, coords_out, flow_out=None, dst1=None, dst2=None, prepare=False:
                        real['flow'](x, weight, bias, coords, coords_out, flow_out, dst1, dst2, prepare))
    for h, w in ((128, 192), (136, 144)):
        fr = nets['synth'].stereo_frames(34, 1, h, w)
        i1, i2 = fr['image1l'].to(DEV), fr['image2l'].to(DEV)
        for sw in (dict(FRAME_OPLISTS=False, LOOP_OPLIST=False), dict(FRAME_OPLISTS=False, LOOP_OPLIST=True)):
            old = _routes(nets, **sw)
            try:
                nets['off']._ws = None                                            # (launchers are rebuilt through the wrappers)
                assert nets['off'](i1, i2)[0][-1].shape == (1, 2, h, w)
            finally:
                _routes(nets, **old)
    nets['off']._ws = None
