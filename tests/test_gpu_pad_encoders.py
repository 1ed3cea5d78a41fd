"""GPU: RAFT's ``pad_encoders`` -- layer2, layer3 and the output layer of both encoders on the tuned kernels over zero-padded maps at image
sizes whose 1/8 map they refuse.

Kernel level: the encoders' valid-extent entry points (rpe_enc_conv_wino_v, rpe_enc_conv_wino24_v, rpe_enc_conv_s2_v, rpe_enc_conv_s2_m96_v,
rpe_instnorm_apply_v) on a 12 x 16 map with the valid extent 11 x 13 (an odd last row, a quad that straddles the extent), batch 2, outputs
pre-filled with NaN: inside the extent the bits of the plain entry point on the same zero-padded input, outside it exactly zero (and the
plain kernel leaves something there); the moments over the content only, against float64; the loader-side normalisation against float64
on the cropped input with the generic route's own error as the bar (x 1.5: both are f32 sums of the same products in another order).

Statistics, measured on an MI355X (error of (mean, 1/std) against float64 moments of the kernel's own output; valid-extent records on the
padded map / the plain kernel's records on an unpadded 12 x 16 map): see NOTES.md, "Padded encoders".

Encoder and network level: BasicEncoder alone (instance and batch norm, split_act on and off) at 88 x 104, 96 x 112, 88 x 96 against the
generic route and oracle.raft's encoder in float64; the dispatch routes; RAFT.forward at 136 x 152 with both flags; a tuned size."""
import copy

import pytest
import torch
import torch.nn.functional as F

from oracle import raft as oraft

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FLOW_BAR, HIDDEN_BAR = 1e-3, 5e-3           # tests/test_gpu_pad_maps.py's
B, MH, MW, HV, WV = 2, 12, 16, 11, 13
NAN = float('nan')
EPS = 1e-5


@pytest.fixture(scope='module')
def gen(rpe):
    g = torch.Generator(device=DEV)
    g.manual_seed(91)
    return g


def _padded_input(c, gen, mh=MH, mw=MW, hv=HV, wv=WV, shift=0.0):
    x = torch.zeros(B, c, mh, mw, device=DEV)
    x[:, :, :hv, :wv] = shift + torch.randn(B, c, hv, wv, generator=gen, device=DEV)
    return x


def _check(name, got, want, hv=HV, wv=WV):
    """Inside the valid extent the plain kernel's bits; outside exactly zero.  Returns what the plain kernel leaves in the padding."""
    assert torch.equal(got[:, :, :hv, :wv], want[:, :, :hv, :wv]), f'{name}: valid region differs from the plain kernel'
    pad = got.clone()
    pad[:, :, :hv, :wv] = 0
    assert torch.equal(pad, torch.zeros_like(pad)), f'{name}: padding is not exactly zero (max |.| {float(pad.abs().nan_to_num(1e9).max()):.3g})'
    outside = want.clone()
    outside[:, :, :hv, :wv] = 0
    return float(outside.abs().max())


def _moments64(t):
    """float64 (mean, 1/sqrt(var + eps)) per plane of t (b, c, h, w), biased variance."""
    t = t.double()
    return torch.stack((t.mean((2, 3)), 1.0 / torch.sqrt(t.var((2, 3), unbiased=False) + EPS)), -1)


def _packing(ops, kind, w, bias):
    return (ops.PackedWino if kind == 'wino' else ops.PackedWino24)(w, bias)


@pytest.mark.parametrize('kind', ['wino', 'wino24'])
@pytest.mark.parametrize('c', [64, 96, 128])
def test_winograd_encoder_epilogues_valid_extent(rpe, gen, kind, c):
    from rpe_amd import ops
    w = torch.randn(c, c, 3, 3, generator=gen, device=DEV) / (3 * c ** 0.5)
    bias = 0.5 + torch.rand(c, generator=gen, device=DEV)
    scale = 0.5 + torch.rand(c, generator=gen, device=DEV)
    pw = _packing(ops, kind, w, bias)
    x = _padded_input(c, gen)
    new = lambda: torch.full((B, c, MH, MW), NAN, device=DEV)
    # (a) folded batch norm + ReLU + residual
    res = _padded_input(c, gen)
    want = ops.conv_wino(x, pw, ops.CONV_RELU, new(), scale=scale, residual=res)
    got = ops.conv_wino(x, pw, ops.CONV_RELU, new(), scale=scale, residual=res, enc_valid=(HV, WV))
    assert _check(f'{kind} affine + residual', got, want) > 0
    assert torch.equal(ops.conv_wino(x, pw, ops.CONV_RELU, new(), scale=scale, residual=res, enc_valid=(MH, MW)), want)
    # (b) raw output + moments
    st_p, st_v, st_f = (ops.conv_wino_stats_buffer(B, c, MH, MW, DEV) for _ in range(3))
    for s in (st_p, st_v, st_f):
        s.tensor.fill_(NAN)
    want = ops.conv_wino(x, pw, ops.CONV_LINEAR, new(), stats=st_p)
    got = ops.conv_wino(x, pw, ops.CONV_LINEAR, new(), stats=st_v, enc_valid=(HV, WV))
    assert _check(f'{kind} raw + stats', got, want) > 0
    full = ops.conv_wino(x, pw, ops.CONV_LINEAR, new(), stats=st_f, enc_valid=(MH, MW))
    assert torch.equal(full, want) and torch.equal(st_f.tensor, st_p.tensor)                  # the full extent IS the plain launch, records included
    rec = st_v.tensor
    assert bool(torch.isfinite(rec).all()) and float(rec[..., 0].sum(1).min()) == float(rec[..., 0].sum(1).max()) == HV * WV
    mi = ops.instnorm_finalize(st_v, HV * WV, eps=EPS, channels=c)
    truth = _moments64(got[:, :, :HV, :WV])
    # the plain kernel's statistics on an UNPADDED 12 x 16 map, against float64 of its own output: the bar's yardstick
    xu = torch.randn(B, c, MH, MW, generator=gen, device=DEV)
    st_u = ops.conv_wino_stats_buffer(B, c, MH, MW, DEV)
    yu = ops.conv_wino(xu, pw, ops.CONV_LINEAR, new(), stats=st_u)
    mu = ops.instnorm_finalize(st_u, MH * MW, eps=EPS, channels=c)
    tu = _moments64(yu)
    err = [float(((mi.double() - truth)[..., k] / truth[..., k].abs().clamp_min(1.0)).abs().max()) for k in (0, 1)]
    ref = [float(((mu.double() - tu)[..., k] / tu[..., k].abs().clamp_min(1.0)).abs().max()) for k in (0, 1)]
    print(f'{kind} c={c}: statistics error valid-extent mean {err[0]:.2e} inv {err[1]:.2e}; plain unpadded mean {ref[0]:.2e} inv {ref[1]:.2e}; '
          f'ratios {err[0] / ref[0]:.2f} {err[1] / ref[1]:.2f}')
    assert err[0] <= 1.5 * ref[0] and err[1] <= 1.5 * ref[1]
    # (c) raw output + moments with the loader-side normalisation: mean < 0 so that relu((0 - mean) * inv) > 0 in the padding
    pre = torch.stack((-0.5 - torch.rand(B, c, generator=gen, device=DEV), 0.5 + torch.rand(B, c, generator=gen, device=DEV)), -1).contiguous()
    st_c = ops.conv_wino_stats_buffer(B, c, MH, MW, DEV)
    got = ops.conv_wino(x, pw, ops.CONV_LINEAR, new(), stats=st_c, pre_norm=pre, enc_valid=(HV, WV))
    _check(f'{kind} pre_norm padding', got, got)
    xn = torch.relu((x[:, :, :HV, :WV] - pre[..., 0, None, None]) * pre[..., 1, None, None])
    truth = F.conv2d(xn.double(), w.double(), bias.double(), padding=1)
    e_v = float((got[:, :, :HV, :WV].double() - truth).abs().max())
    e_g = float((ops.conv_direct(xn.contiguous(), w, bias, 1, 1).double() - truth).abs().max())
    leak = ops.conv_wino(x, pw, ops.CONV_LINEAR, new(), pre_norm=pre)                          # the plain kernel reads relu(-mean * inv) there
    e_leak = float((leak[:, :, :HV, :WV].double() - truth).abs().max())
    print(f'{kind} c={c}: pre_norm error vs float64 valid-extent {e_v:.2e}, generic {e_g:.2e} (ratio {e_v / e_g:.2f}); plain kernel on the padded map {e_leak:.2e}')
    assert e_v <= 1.5 * e_g and e_leak > 100 * e_g
    assert bool(torch.isfinite(st_c.tensor).all())
    m_c = ops.instnorm_finalize(st_c, HV * WV, eps=EPS, channels=c)
    assert float((m_c.double() - _moments64(got[:, :, :HV, :WV])).abs().max()) < 1e-4
    # batch independence: row 1 alone, bit for bit, records included
    st_1 = ops.conv_wino_stats_buffer(1, c, MH, MW, DEV)
    one = ops.conv_wino(x[1:2].contiguous(), pw, ops.CONV_LINEAR, torch.full((1, c, MH, MW), NAN, device=DEV), stats=st_1, pre_norm=pre[1:2].contiguous(),
                        enc_valid=(HV, WV))
    assert torch.equal(one, got[1:2]) and torch.equal(st_1.tensor, st_c.tensor[1:2])


def test_statistics_with_a_tile_wholly_outside_the_extent(rpe, gen):
    """A 24 x 32 map with 11 x 13 of content: most 16 x 8 patches lie wholly outside -- zero-count records, finite moments."""
    from rpe_amd import ops
    c = 64
    w = torch.randn(c, c, 3, 3, generator=gen, device=DEV) / (3 * c ** 0.5)
    x = _padded_input(c, gen, 24, 32)
    for kind in ('wino', 'wino24'):
        pw = _packing(ops, kind, w, torch.rand(c, generator=gen, device=DEV))
        st = ops.conv_wino_stats_buffer(B, c, 24, 32, DEV)
        st.tensor.fill_(NAN)
        out = ops.conv_wino(x, pw, ops.CONV_LINEAR, torch.full((B, c, 24, 32), NAN, device=DEV), stats=st, enc_valid=(HV, WV))
        rec = st.tensor
        assert bool(torch.isfinite(rec).all()) and int((rec[..., 0] == 0).sum()) > 0 and bool((rec[..., 1:][rec[..., 0] == 0] == 0).all())
        mi = ops.instnorm_finalize(st, HV * WV, eps=EPS, channels=c)
        assert bool(torch.isfinite(mi).all())
        assert float((mi.double() - _moments64(out[:, :, :HV, :WV])).abs().max()) < 1e-4, kind


@pytest.mark.parametrize('cin,cout,k', [(64, 96, 3), (96, 128, 3), (64, 96, 1)])
def test_stride2_valid_extent(rpe, gen, cin, cout, k):
    """Input 24 x 32 with 22 x 26 of content -> output 12 x 16 with 11 x 13; both tile classes where the layer has both (3x3 to 96 channels)."""
    from rpe_amd import ops
    w = torch.randn(cout, cin, k, k, generator=gen, device=DEV) / (k * cin ** 0.5)
    bias = 0.5 + torch.rand(cout, generator=gen, device=DEV)
    scale = 0.5 + torch.rand(cout, generator=gen, device=DEV)
    pc = ops.PackedConv(w, bias)
    x = _padded_input(cin, gen, 24, 32, 22, 26)
    new = lambda b=B: torch.full((b, cout, MH, MW), NAN, device=DEV)
    entries = ('rpe_conv_fused', 'rpe_conv_fused_m96') if (k, cout) == (3, 96) else ('rpe_conv_fused',)
    outs = []
    for entry in entries:
        kw = dict(stride=2, entry=entry)
        want = ops.conv_fused(x, pc, ops.CONV_RELU, new(), scale=scale, **kw)                  # folded batch norm + ReLU
        got = ops.conv_fused(x, pc, ops.CONV_RELU, new(), scale=scale, enc_valid=(HV, WV), **kw)
        assert _check(f'{entry} affine', got, want) > 0
        assert torch.equal(ops.conv_fused(x, pc, ops.CONV_RELU, new(), scale=scale, enc_valid=(MH, MW), **kw), want)
        st_p, st_v, st_f = (ops.conv_stats_buffer(B, cout, 24, 32, DEV, stride=2).fill_(NAN) for _ in range(3))
        want = ops.conv_fused(x, pc, ops.CONV_LINEAR, new(), stats=st_p, **kw)                 # raw output + moments
        got = ops.conv_fused(x, pc, ops.CONV_LINEAR, new(), stats=st_v, enc_valid=(HV, WV), **kw)
        assert _check(f'{entry} raw + stats', got, want) > 0
        assert torch.equal(ops.conv_fused(x, pc, ops.CONV_LINEAR, new(), stats=st_f, enc_valid=(MH, MW), **kw), want) and torch.equal(st_f, st_p)
        assert bool(torch.isfinite(st_v).all()) and float(st_v[..., 0].sum(2).min()) == float(st_v[..., 0].sum(2).max()) == HV * WV
        mi = ops.instnorm_finalize(st_v, HV * WV, eps=EPS, channels=cout)
        truth = _moments64(got[:, :, :HV, :WV])
        xu = torch.randn(B, cin, 24, 32, generator=gen, device=DEV)
        st_u = ops.conv_stats_buffer(B, cout, 24, 32, DEV, stride=2)
        yu = ops.conv_fused(xu, pc, ops.CONV_LINEAR, new(), stats=st_u, **kw)
        mu, tu = ops.instnorm_finalize(st_u, MH * MW, eps=EPS, channels=cout), _moments64(yu)
        err = [float(((mi.double() - truth)[..., j] / truth[..., j].abs().clamp_min(1.0)).abs().max()) for j in (0, 1)]
        ref = [float(((mu.double() - tu)[..., j] / tu[..., j].abs().clamp_min(1.0)).abs().max()) for j in (0, 1)]
        print(f'{entry} {cin}->{cout} {k}x{k}: statistics error valid-extent mean {err[0]:.2e} inv {err[1]:.2e}; plain unpadded {ref[0]:.2e} {ref[1]:.2e}')
        assert err[0] <= 1.5 * ref[0] and err[1] <= 1.5 * ref[1]
        st_1 = ops.conv_stats_buffer(1, cout, 24, 32, DEV, stride=2)
        one = ops.conv_fused(x[1:2].contiguous(), pc, ops.CONV_LINEAR, new(1), stats=st_1, enc_valid=(HV, WV), **kw)
        assert torch.equal(one, got[1:2]) and torch.equal(st_1, st_v[1:2])                      # batch independence
        outs.append((got, st_v))
    if len(outs) == 2:                                                                          # the two tile classes stay bit-identical
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize('inplace', [False, True])
def test_instnorm_apply_valid_extent(rpe, gen, inplace):
    from rpe_amd import ops
    c = 96
    mi = torch.stack((-0.5 - torch.rand(B, c, generator=gen, device=DEV), 0.5 + torch.rand(B, c, generator=gen, device=DEV)), -1).contiguous()
    rmi = torch.stack((-0.5 - torch.rand(B, c, generator=gen, device=DEV), 0.5 + torch.rand(B, c, generator=gen, device=DEV)), -1).contiguous()
    x, res = _padded_input(c, gen), _padded_input(c, gen)
    for name, kw in (('relu', dict(relu=True)), ('residual', dict(relu=True, residual=res)),
                     ('raw residual + relu', dict(relu=True, residual=res, residual_norm=rmi, residual_relu=True)),
                     ('raw residual', dict(relu=True, residual=res, residual_norm=rmi, residual_relu=False))):
        want = ops.instnorm_apply(x.clone(), mi, out=torch.full_like(x, NAN), **kw)
        xin = x.clone()
        out = xin if inplace else torch.full_like(x, NAN)
        got = ops.instnorm_apply(xin, mi, out=out, valid=(HV, WV), **kw)
        assert got is out and _check(f'instnorm_apply {name}', got, want) > 0
        full = ops.instnorm_apply(x.clone(), mi, out=torch.full_like(x, NAN), valid=(MH, MW), **kw)
        assert torch.equal(full, want), name
    assert torch.equal(ops.instnorm_apply(x[1:2].clone(), mi[1:2].contiguous(), valid=(HV, WV)), ops.instnorm_apply(x.clone(), mi, valid=(HV, WV))[1:2])


# ---- encoder and network level

SIZES = [(88, 104), (96, 112), (88, 96)]


@pytest.fixture(scope='module')
def encs(rpe):
    from rpe_amd import raft, synth
    torch.manual_seed(5)
    out = {}
    for norm in ('instance', 'batch'):
        enc = raft.BasicEncoder(output_dim=256, norm_fn=norm).eval()
        if norm == 'batch':                                       # frozen batch norm with statistics that are not the identity
            for m in enc.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.uniform_(-0.2, 0.2); m.running_var.uniform_(0.5, 1.5); m.weight.data.uniform_(0.5, 1.5); m.bias.data.uniform_(-0.2, 0.2)
        om = oraft.BasicEncoder(output_dim=256, norm_fn=norm).eval()
        om.load_state_dict(enc.state_dict())
        out[norm] = (enc.to(DEV), om.double())
    return dict(encs=out, raft=raft, synth=synth)


def _switch(raft, **kw):
    old = {k: getattr(raft, k) for k in kw}
    for k, v in kw.items():
        setattr(raft, k, v)
    return old


@pytest.mark.parametrize('h,w', SIZES)
@pytest.mark.parametrize('norm,split', [('instance', False), ('batch', True), ('batch', False), ('instance', True)])
def test_encoder_against_the_generic_route_and_float64(encs, h, w, norm, split):
    from rpe_amd import _lib
    raft = encs['raft']
    enc, om = encs['encs'][norm]
    img = encs['synth'].stereo_frames(41, 2, h, w)['image1l']
    with torch.no_grad():
        truth = om(2 * (img.double() / 255.0) - 1.0)
        if split:
            truth = torch.cat((torch.tanh(truth[:, :128]), torch.relu(truth[:, 128:])), 1)
    x = img.to(DEV)
    old = _switch(raft, FRAME_OPLISTS=False)
    try:
        res, direct = {}, {}
        for flag in (False, True):
            enc.pad_encoders = flag
            with torch.no_grad():
                enc(x, raw255=True, split_act=split)              # (packings are made on first use)
                with _lib.CountingLib() as count:
                    res[flag] = enc(x, raw255=True, split_act=split)
            direct[flag] = (count.names.count('rpe_conv_direct'), sum(n.startswith('rpe_enc_conv') for n in count.names))
    finally:
        _switch(raft, **old)
        enc.pad_encoders = False
    h8, w8 = h // 8, w // 8
    assert res[True].shape == res[False].shape == (2, 256, h8, w8) and res[True].is_contiguous()
    # no generic convolution under the switch; without it the encoder pays for every w8 % 4 != 0 (a grid of odd rows alone, 88 x 96, only
    # leaves Winograd for the implicit GEMM).  On the parent commit the key is ignored and no encoder form runs: this fails there.
    assert direct[True][0] == 0 and direct[True][1] > 0 and direct[False][1] == 0 and (direct[False][0] > 0 or (w // 8) % 4 == 0)
    e = {f: float((res[f].cpu().double() - truth).abs().max()) for f in res}
    print(f'{norm} split={split} {h}x{w}: error vs float64 padded {e[True]:.3e} generic {e[False]:.3e} (ratio {e[True] / e[False]:.2f}); '
          f'padded vs generic {float((res[True] - res[False]).abs().max()):.2e}; rpe_conv_direct calls off {direct[False][0]}')
    assert e[True] <= 1.5 * e[False]
    # the invariant, after the pass: every padded intermediate is exactly zero outside its content
    ws = enc._ws
    hp, wp = raft.padded_size(h8, w8)
    assert ws['valid'] == (h8, w8) and tuple(ws['out'].shape[-2:]) == (hp, wp) and tuple(ws['p2'].shape[-2:]) == (4 * hp, 4 * wp)
    for k, f in (('p2', 4), ('l2', 2), ('l3', 1), ('out', 1)):
        t = ws[k].clone()
        assert tuple(t.shape[-2:]) == (f * hp, f * wp), k
        t[:, :, :f * h8, :f * w8] = 0
        assert torch.equal(t, torch.zeros_like(t)), k


@pytest.mark.parametrize('norm', ['instance', 'batch'])
def test_encoder_dispatch_routes_and_module_switch(encs, norm):
    raft = encs['raft']
    enc, _ = encs['encs'][norm]
    x = encs['synth'].stereo_frames(42, 2, 88, 104)['image1l'].to(DEV)
    outs = {}
    try:
        enc.pad_encoders = True
        for name, sw in (('call by call', False), ('recorded', True), ('replayed', True), ('replayed again', True)):
            old = _switch(raft, FRAME_OPLISTS=sw)
            try:
                with torch.no_grad():
                    outs[name] = enc(x, raw255=True, split_act=norm == 'batch')
            finally:
                _switch(raft, **old)
        key = [k for k in enc._recorded._progs if k[-1].pad_encoders]
        assert key and enc._recorded._progs[key[-1]].complete
        with torch.no_grad():
            outs['row 1 alone'] = torch.cat((outs['call by call'][:1], enc(x[1:2], raw255=True, split_act=norm == 'batch')))
        enc.pad_encoders = False
        old = _switch(raft, PAD_ENCODERS=True, FRAME_OPLISTS=False)
        try:
            with torch.no_grad():
                outs['module switch'] = enc(x, raw255=True, split_act=norm == 'batch')
        finally:
            _switch(raft, **old)
    finally:
        enc.pad_encoders = False
    for name, o in outs.items():
        assert torch.equal(o, outs['call by call']), name


ITERS = 4


@pytest.fixture(scope='module')
def nets(rpe):
    from rpe_amd import raft, synth
    cfg = synth.model_config(136, 152, iters=ITERS)
    off = synth.init_synthetic_weights(raft.RAFT(cfg)).eval().to(DEV)
    on = raft.RAFT(dict(cfg, pad_maps=True, pad_encoders=True)).eval().to(DEV)
    on.load_state_dict(off.state_dict())
    om = oraft.RAFT(cfg)
    om.load_state_dict({k: v.cpu() for k, v in off.state_dict().items()})
    om.eval()
    return dict(off=off, on=on, oracle=om, synth=synth, raft=raft)


def test_forward_at_136x152_with_both_flags(nets, monkeypatch):
    from rpe_amd import _lib
    h, w = 136, 152
    fr = nets['synth'].stereo_frames(43, 1, h, w)
    i1, i2 = fr['image1l'], fr['image2l']
    with torch.no_grad():
        oflow, ohid, _ = nets['oracle'](i1.clone(), i2.clone(), iters=ITERS)
        o64 = copy.deepcopy(nets['oracle']).double()
        monkeypatch.setattr(torch.Tensor, 'float', lambda t: t.double())
        tflow, thid, _ = o64(i1.double(), i2.double(), iters=ITERS)
        monkeypatch.undo()
    res, direct = {}, {}
    old = _switch(nets['raft'], FRAME_OPLISTS=False, LOOP_OPLIST=False)
    try:
        for name in ('off', 'on'):
            nets[name](i1.to(DEV), i2.to(DEV))
            with _lib.CountingLib() as count:
                flows, hid, _ = nets[name](i1.to(DEV), i2.to(DEV))
            res[name], direct[name] = (flows[-1].cpu(), hid.cpu()), count.names.count('rpe_conv_direct')
    finally:
        _switch(nets['raft'], **old)
    assert direct['on'] == 0 and direct['off'] > 0
    d_or = float((res['on'][0] - oflow[-1]).abs().max()), float((res['on'][1] - ohid).abs().max())
    e = {n: (float((res[n][0].double() - tflow[-1]).abs().max()), float((res[n][1].double() - thid).abs().max())) for n in res}
    print(f'{h}x{w}: both flags vs oracle flow {d_or[0]:.2e} px hidden {d_or[1]:.2e}; vs float64: flow on {e["on"][0]:.3e} off {e["off"][0]:.3e} '
          f'(ratio {e["on"][0] / e["off"][0]:.2f}), hidden on {e["on"][1]:.3e} off {e["off"][1]:.3e} (ratio {e["on"][1] / e["off"][1]:.2f})')
    assert d_or[0] < FLOW_BAR and d_or[1] < HIDDEN_BAR
    assert e['on'][0] <= 1.5 * e['off'][0] and e['on'][1] <= 1.5 * e['off'][1]
    # the recorded route gives the call-by-call bits
    a = nets['on'](i1.to(DEV), i2.to(DEV))
    b = nets['on'](i1.to(DEV), i2.to(DEV))
    assert torch.equal(a[0][-1].cpu(), res['on'][0]) and torch.equal(b[0][-1].cpu(), res['on'][0]) and torch.equal(b[1].cpu(), res['on'][1])


def test_tuned_size_is_untouched_by_the_switch(nets):
    """128 x 192 (grid 16 x 24, which the tuned kernels take): identical outputs and identical launch names with the switches on and off."""
    from rpe_amd import _lib
    fr = nets['synth'].stereo_frames(44, 1, 128, 192)
    i1, i2 = fr['image1l'].to(DEV), fr['image2l'].to(DEV)
    old = _switch(nets['raft'], FRAME_OPLISTS=False, LOOP_OPLIST=False)
    try:
        got = {}
        for name in ('off', 'on'):
            nets[name](i1, i2)
            with _lib.CountingLib() as count:
                out = nets[name](i1, i2)
            got[name] = (out, list(count.names))
    finally:
        _switch(nets['raft'], **old)
    assert torch.equal(got['on'][0][0][-1], got['off'][0][0][-1]) and torch.equal(got['on'][0][1], got['off'][0][1])
    assert got['on'][1] == got['off'][1] and not any(n.endswith('_v') or n == 'rpe_copy_rect' for n in got['on'][1])
