"""GPU: RAFT with ``alt_corr_fp16`` -- the on-the-fly correlation (``alternate_corr``) on fp16 feature maps.

Images 128 x 160 (1/8 map 16 x 20, four levels down to 2 x 2), 2 pairs, seeded synthetic weights, 4 GRU iterations.
  * key False (or absent): flow and hidden state are the bits of the alternate_corr model, and no launch list holds one of the new kinds;
  * key True: the lists hold the new kinds and no f32 alt kind;
  * accuracy: D16 = max|flow(mixed_precision pyramid model) - flow(f32 model)|, Dalt = max|flow(alt_corr_fp16 model) - flow(f32 model)|, all on
    the GPU with the same weights and inputs.  Dalt > 1e-6 (the rounding is visible) and Dalt <= 4 D16: the pooled maps carry a full fp16
    rounding at levels 1-3, where the pyramid route's error is averaged down by 2^l -- about 1.8x the rms error over the four levels --
    and the margin doubles that because the maximum passes through four nonlinear GRU iterations;
  * pad_maps with the key on at 136 x 144 (1/8 map 17 x 18: odd rows, rows of 4.5 quads): runs, and agrees with the same model without
    pad_maps to the bars of tests/test_gpu_pad_maps.py (flow 1e-3 px, hidden 5e-3).  (A 120 x 136 image has a 15 x 17 map whose fourth
    correlation level would be 1 x 2, which every correlation route and the oracle's sampler refuse; 17 x 18 is the smallest map with
    four levels, an odd height and w8 % 4 != 0 -- the size tests/test_gpu_pad_maps.py runs its loop at.)

Measured on an MI355X (Dalt / D16): see NOTES.md, "On-the-fly correlation"."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
H, W, ITERS, PAIRS = 128, 160, 4, 2
FLOW_BAR, HIDDEN_BAR = 1e-3, 5e-3           # tests/test_gpu_pad_maps.py's


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope='module')
def nets(rpe):
    from rpe_amd import raft, synth
    cfg = synth.model_config(H, W, iters=ITERS)
    f32 = synth.init_synthetic_weights(raft.RAFT(cfg)).eval().to(DEV)
    sd = f32.state_dict()

    def make(**kw):
        c = dict(cfg, **kw)
        if kw.get('alt_corr_fp16', False) is None:
            del c['alt_corr_fp16']
        net = raft.RAFT(c).eval().to(DEV)
        net.load_state_dict(sd)
        return net
    fr = synth.stereo_frames(21, PAIRS, H, W)
    return dict(f32=f32, mp=make(mixed_precision=True), no_key=make(alternate_corr=True, alt_corr_fp16=None), off=make(alternate_corr=True, alt_corr_fp16=False),
                on=make(alternate_corr=True, alt_corr_fp16=True), i1=fr['image1l'].to(DEV), i2=fr['image2l'].to(DEV), make=make, synth=synth)


def _tracker_passes(net, i1, i2, n=3):
    """The pass as a tracker makes it (encoder outputs given, batch <= 4): recorded front, the loop's launch list, recorded tail."""
    f = net.encode_features((i1, i2))
    fm, cn = (f[:PAIRS].contiguous(), f[PAIRS:].contiguous()), net.encode_context(i1)
    for _ in range(n):
        out = net(None, None, fmaps=fm, cnet=cn)
    return out


def _list_kinds(net):
    """Every op kind in the launch lists the model holds: the recorded fronts and tails, and the update loop's program."""
    kinds = set()
    for post in net._recorded._progs.values():
        for rec in (post.pre, post):
            kinds |= {k for k, _, _ in rec._items}
    for ws in net._ws.values():
        if '_program' in ws:
            kinds |= {k for k, _, _ in ws['_program'][1][0]._items}
    return kinds


def test_key_off_is_the_alternate_corr_model_bit_for_bit(nets):
    from rpe_amd import _lib, ops
    new = {_lib.OP_CORR_ALT_PREPARE_EX, _lib.OP_CORR_ALT_LOOKUP_DT}
    i1, i2 = nets['i1'], nets['i2']
    outs = {name: nets[name](i1, i2) for name in ('no_key', 'off')}
    assert _same(outs['off'][0][-1], outs['no_key'][0][-1]) and _same(outs['off'][1], outs['no_key'][1])
    assert outs['off'][0][-1].shape == (PAIRS, 2, H, W) and outs['off'][1].shape == (PAIRS, 128, H // 8, W // 8)
    rec = {name: _tracker_passes(nets[name], i1, i2) for name in ('no_key', 'off')}
    assert _same(rec['off'][0][-1], rec['no_key'][0][-1]) and _same(rec['off'][1], rec['no_key'][1])
    for name in ('no_key', 'off'):
        net = nets[name]
        kinds = _list_kinds(net)
        assert isinstance(net._pyr, ops.AltCorr) and net._pyr.fp16 is False
        assert len(net._recorded._progs) > 0                       # (the pass was recorded: its prepare is in a list)
        assert {_lib.OP_CORR_ALT_PREPARE, _lib.OP_CORR_ALT_LOOKUP} <= kinds and not kinds & new, (name, sorted(kinds))
    with _lib.CountingLib() as c:
        nets['off'](i1, i2)
    assert not any(n.endswith('_prepare_ex') or n.endswith('_lookup_dt') for n in c.names)


def test_key_on_runs_the_fp16_kinds_only(nets):
    from rpe_amd import _lib, ops
    i1, i2 = nets['i1'], nets['i2']
    net = nets['on']
    direct = net(i1, i2)
    rec = _tracker_passes(net, i1, i2)
    assert _same(rec[0][-1], direct[0][-1]) and _same(rec[1], direct[1])           # recorded and replayed = launch by launch
    kinds = _list_kinds(net)
    assert isinstance(net._pyr, ops.AltCorr) and net._pyr.fp16 is True and net._pyr.nbytes * 2 <= nets['off']._pyr.nbytes + 4096
    assert len(net._recorded._progs) > 0
    assert {_lib.OP_CORR_ALT_PREPARE_EX, _lib.OP_CORR_ALT_LOOKUP_DT} <= kinds, sorted(kinds)
    assert not kinds & {_lib.OP_CORR_ALT_PREPARE, _lib.OP_CORR_ALT_LOOKUP, _lib.OP_CORR_ALT_LOOKUP_EX, _lib.OP_CORR_BUILD, _lib.OP_CORR_LOOKUP}, sorted(kinds)
    f = net.encode_features((i1, i2))
    fm, cn = (f[:PAIRS].contiguous(), f[PAIRS:].contiguous()), net.encode_context(i1)
    with _lib.CountingLib() as c:
        net(None, None, fmaps=fm, cnet=cn)
        net(i1, i2)
    assert not any(n in ('rpe_corr_alt_prepare', 'rpe_corr_alt_lookup', 'rpe_corr_alt_lookup_ex', 'rpe_corr_build_ex', 'rpe_corr_lookup') for n in c.names)
    # the key decides the scratch: the same module with the key flipped gets a new AltCorr
    net.alt_corr_fp16 = False
    try:
        back = net(i1, i2)
        assert net._pyr.fp16 is False and _same(back[0][-1], nets['off'](i1, i2)[0][-1])
    finally:
        net.alt_corr_fp16 = True
    again = net(i1, i2)
    assert net._pyr.fp16 is True and _same(again[0][-1], direct[0][-1])


def test_accuracy_against_the_mixed_precision_pyramid_model(nets):
    i1, i2 = nets['i1'], nets['i2']
    flow = {name: nets[name](i1, i2)[0][-1] for name in ('f32', 'mp', 'on', 'off')}
    d16 = float((flow['mp'] - flow['f32']).abs().max())
    dalt = float((flow['on'] - flow['f32']).abs().max())
    dalt32 = float((flow['off'] - flow['f32']).abs().max())
    print(f'RAFT {H}x{W}, {PAIRS} pairs, {ITERS} iterations, final flow against the f32 pyramid model: D16 (mixed_precision) {d16:.3e} px, '
          f'Dalt (alt_corr_fp16) {dalt:.3e} px, ratio Dalt / D16 = {dalt / d16:.2f}; f32 alternate_corr {dalt32:.3e} px; '
          f'flow scale {float(flow["f32"].abs().max()):.2f} px')
    assert bool(torch.isfinite(flow['on']).all())
    assert d16 > 1e-6 and dalt > 1e-6                                              # the rounding is visible
    assert dalt <= 4 * d16, (dalt, d16)


def test_pad_maps_with_the_key_on(nets):
    h, w = 136, 144
    fr = nets['synth'].stereo_frames(22, PAIRS, h, w)
    i1, i2 = fr['image1l'].to(DEV), fr['image2l'].to(DEV)
    plain, padded = nets['make'](alternate_corr=True, alt_corr_fp16=True), nets['make'](alternate_corr=True, alt_corr_fp16=True, pad_maps=True)
    a, b = plain(i1, i2), padded(i1, i2)
    ws = list(padded._ws.values())[-1]
    assert ws['valid'] == (17, 18) and tuple(ws['hx'].shape[-2:]) != (17, 18) and padded._pyr.fp16 is True and plain._pyr.fp16 is True
    assert b[0][-1].shape == (PAIRS, 2, h, w) and b[1].shape == (PAIRS, 128, 17, 18)
    d, dh = float((a[0][-1] - b[0][-1]).abs().max()), float((a[1] - b[1]).abs().max())
    print(f'{h}x{w}, alt_corr_fp16: pad_maps vs generic route flow {d:.2e} px, hidden {dh:.2e}')
    assert bool(torch.isfinite(b[0][-1]).all()) and d < FLOW_BAR and dh < HIDDEN_BAR
