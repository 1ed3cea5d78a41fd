"""GPU: the backward of the correlation (csrc/corr_backward.hip; ops.corr_lookup_backward, ops.corr_build_backward, raft_grad.update_step_backward's
``ret_d_corr``, RAFT.forward(grad_corr=True), PoseNet.forward(grad_corr=True)).  Truth is the float64 restatement tests/corr_grad_ref.py (pinned
to autograd through oracle.raft.CorrBlock by tests/test_corr_grad_ref_cpu.py) or float64 autograd, on the CPU.

Bound of the lookup's adjoint, per cell of G, u = 2^-24.  One call forms acc = sum of at most four non-zero terms w d with w = fl(wx wy): one
rounding in w and one per fused multiply-add, each at most u times the sum S of the call's absolute terms, 5 u S; G += acc rounds once more,
at most u times the running absolute sum, and adds exactly into the zero of the first call.  Over n calls: (4 + n) u sum S.  The weights
themselves are exact functions of the forward's float32 tap positions, which differ from the exact positions by at most
p = u (6 |v| + size) (corr_grad_ref.position_error derives it from csrc/sampling.h); a weight moves by at most p, a term by at most
|d| (px |wy| + |wx| py + px py), summed: E.  Bound = (4 + n) u (sum S + sum E) + sum E.

Bound of the build's adjoint, per element: a plain sum of K products in f32 plus the partials' f64 sum and the scale: (K + partials + 2) u
sum |a| |b|; F2cat's pooled values carry up to 3 roundings per level (9), d_fmap2's pool adjoints one per level (4, applied to sum |a| |b|)."""
import pytest
import torch

import corr_grad_ref as ref
import update_block_ref as ubref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = ref.U
MAPS = [(16, 16), (21, 23), (17, 40)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _coords(b, h8, w8, seed):
    """float32 (b,2,h8,w8): targets uniform over the map plus a margin of 6, every fraction in [0.02, 0.98] -- so c / 2^l is at least 2.5e-3 from
    an integer at every level --, and in row 0 the planted queries: integers, the last row and column, x = -0.5, two windows wholly outside
    every level, and (w8 - 1 + 4, h8 - 1 + 4), of whose window only a corner is inside."""
    g = _gen(seed)
    def axis(size):
        whole = torch.floor(torch.rand(b, h8 * w8, generator=g) * (size + 11) - 6)
        return whole + 0.02 + 0.96 * torch.rand(b, h8 * w8, generator=g)
    x, y = axis(w8), axis(h8)
    plants = [(3.0, 5.0), (w8 - 1.0, h8 - 1.0), (-0.5, 2.5), (-50.5, -50.5), (w8 + 60.5, h8 + 60.5), (w8 - 1.0 + 4, h8 - 1.0 + 4)]
    for q, (px, py) in enumerate(plants):
        x[0, 7 * q + 1], y[0, 7 * q + 1] = px, py
    co = torch.stack((x, y), 1).reshape(b, 2, h8, w8).float()
    planted = torch.zeros(b, h8 * w8, dtype=torch.bool)
    planted[0, [7 * q + 1 for q in range(len(plants))]] = True
    for l in range(4):                                                  # asserted on the generated input itself
        v = co.double().reshape(b, 2, -1) / 2 ** l
        away = (v - torch.round(v)).abs().min(1).values
        assert bool((away[~planted] >= 1e-3).all()), l
    return co, [7 * q + 1 for q in (3, 4)]


def _guarded(b, h8, w8):
    n, pad = b * h8 * w8 * ref.volume_cells(h8, w8), 4096
    buf = torch.full((n + 2 * pad,), 7.25, device=DEV)
    G = buf[pad:pad + n].view(b, h8 * w8, -1)
    G.zero_()
    return buf, G, pad


@pytest.mark.parametrize('h8,w8', MAPS)
def test_lookup_adjoint_against_float64(rpe, h8, w8):
    from rpe_amd import ops
    b, g = 2, _gen(h8 * 100 + w8)
    calls = [(_coords(b, h8, w8, 11 * k + h8), torch.randn(b, 324, h8, w8, generator=g)) for k in range(3)]
    buf, G, pad = _guarded(b, h8, w8)
    assert tuple(G.shape) == tuple(ops.corr_grad_volume(b, h8, w8).shape)
    truth, S, E = None, 0, 0
    for n, ((co, outside), d) in enumerate(calls, 1):
        ops.corr_lookup_backward(co.to(DEV), d.to(DEV), G)
        truth = ref.lookup_adjoint(co.double(), d.double(), truth)
        s, e = ref.lookup_adjoint_bounds(co, d)
        S, E = S + s, E + e
        if n in (1, 3):
            bound = (4 + n) * U * (S + E) + E
            err = (G.cpu().double() - truth).abs()
            print(f'lookup adjoint {h8}x{w8} after {n} call(s): max err {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, '
                  f'max |truth| {float(truth.abs().max()):.3e}')
            assert bool((err <= bound).all())
        if n == 1:
            assert not bool(G[0, outside].any()) and float(truth[0, outside].abs().max()) == 0.0      # windows wholly outside: exactly zero
            first = G.clone()
    assert bool((buf[:pad] == 7.25).all()) and bool((buf[-pad:] == 7.25).all())
    # two runs give the same bits; row 0 of the b = 2 call is the b = 1 call
    (co, _), d = calls[0]
    again = ops.corr_lookup_backward(co.to(DEV), d.to(DEV), ops.corr_grad_volume(b, h8, w8))
    one = ops.corr_lookup_backward(co[:1].to(DEV), d[:1].to(DEV), ops.corr_grad_volume(1, h8, w8))
    assert torch.equal(again, first) and torch.equal(one[0], first[0])


def _build_case(h8, w8, c, seed, b=2):
    g = _gen(seed)
    G = torch.randn(b, h8 * w8, ref.volume_cells(h8, w8), generator=g)
    return G, torch.randn(b, c, h8, w8, generator=g), torch.randn(b, c, h8, w8, generator=g)


def _chunks(K):
    kc = max(512, ((K + 7) // 8 + 31) // 32 * 32)
    return (K + kc - 1) // kc


def _check_build(tag, got, G, f1, f2):
    h8, w8 = f1.shape[2:]
    nq, S = G.shape[1], G.shape[2]
    t1, t2, tcat = ref.build_adjoint(G.double(), f1, f2)
    a1, a2, acat = ref.build_adjoint_abs(G, f1, f2)
    s1, s2, scat = ref.build_adjoint(G, f1, f2)                                 # float32 on the CPU, beside it
    bcat = (nq + _chunks(nq) + 2) * U * acat
    bounds = dict(d_fmap1=(S + _chunks(S) + 2 + 9) * U * a1, dF2cat=bcat, d_fmap2=ref.pool_adjoints(bcat, h8, w8) + 4 * U * a2)
    for name, g, t, s in (('d_fmap1', got[0], t1, s1), ('d_fmap2', got[1], t2, s2), ('dF2cat', got[2], tcat, scat)):
        err = (g.cpu().double() - t).abs()
        print(f'{tag} {name}: GPU {ubref.ratio(g, t):.3e}  float32 on the CPU {ubref.ratio(s, t):.3e}  max err / bound {float((err / bounds[name].clamp_min(1e-300)).max()):.3f}')
        assert bool((err <= bounds[name]).all()), name


@pytest.mark.parametrize('c', [8, 256])
@pytest.mark.parametrize('h8,w8', MAPS)
def test_build_adjoint_within_the_derived_bound(rpe, h8, w8, c):
    """A random dense G.  (16,16): one chunk per GEMM; (21,23): S = 622 splits in two, the 483 queries do not; (17,40): both split."""
    from rpe_amd import ops
    G, f1, f2 = _build_case(h8, w8, c, 7 * h8 + w8 + c)
    Gd, f1d, f2d = G.to(DEV), f1.to(DEV), f2.to(DEV)
    got = ops.corr_build_backward(Gd, f1d, f2d, ret_df2cat=True)
    _check_build(f'build adjoint {h8}x{w8} c={c}', got, G, f1, f2)
    again = ops.corr_build_backward(Gd, f1d, f2d, ret_df2cat=True)
    two = ops.corr_build_backward(Gd, f1d, f2d)
    one = ops.corr_build_backward(Gd[:1].contiguous(), f1d[:1].contiguous(), f2d[:1].contiguous(), ret_df2cat=True)
    for a, b, o in zip(got, again, one):
        assert torch.equal(a, b) and torch.equal(a[0], o[0])
    assert torch.equal(two[0], got[0]) and torch.equal(two[1], got[1])


def test_build_adjoint_gives_nothing_to_dropped_rows_and_columns(rpe):
    """(21,23): 21 and 23 are odd, so level 0's last row and column are under no pooled cell.  With G non-zero on the pooled levels only --
    the cells whose pool adjoints pass that row and column by -- d_fmap2 is exactly zero there; with G non-zero on levels 2 and 3 only it is
    also exactly zero under level 1's dropped column (11 is odd: columns 20 and 21).  The rest matches."""
    from rpe_amd import ops
    h8, w8, c = 21, 23, 8
    G, f1, f2 = _build_case(h8, w8, c, 99)
    G[:, :, :h8 * w8] = 0.0
    got = ops.corr_build_backward(G.to(DEV), f1.to(DEV), f2.to(DEV), ret_df2cat=True)
    _check_build('pooled levels only', got, G, f1, f2)
    assert not bool(got[1][:, :, 20].any()) and not bool(got[1][:, :, :, 22].any()) and bool(got[1][:, :, :20, :22].abs().min() > 0)
    G[:, :, :h8 * w8 + 110] = 0.0
    got = ops.corr_build_backward(G.to(DEV), f1.to(DEV), f2.to(DEV), ret_df2cat=True)
    _check_build('levels 2 and 3 only', got, G, f1, f2)
    assert not bool(got[1][:, :, 20:].any()) and not bool(got[1][:, :, :, 20:].any())


def _hx(net, flow):
    b, _, hh, ww = net.shape
    return torch.cat((net, torch.full((b, 126, hh, ww), 1e30), flow), 1).to(DEV)


def test_ret_d_corr_against_float64_and_flag_off_bits(rpe):
    from rpe_amd.raft_grad import update_step_backward as step
    shape, seed = (1, 8, 12), 41
    P, c = ubref.make_params(seed), ubref.make_case(*shape, seed)
    assert ubref.relu_margin(c, P) > 1e-5

    def d_corr(dtype):
        corr = c['corr'][0].to(dtype).requires_grad_(True)
        net = ubref.step(c['net'].to(dtype), c['inp'].to(dtype), corr, c['flow'][0].to(dtype), {k: v.to(dtype) for k, v in P.items()})
        return torch.autograd.grad((net * c['d_net'].to(dtype)).sum(), corr)[0]
    w64, w32 = d_corr(torch.float64), d_corr(torch.float32)
    params = tuple(P[k].to(DEV) for k in ubref.PARAMS)
    args = (_hx(c['net'], c['flow'][0]), c['inp'].to(DEV), c['corr'][0].to(DEV), c['d_net'].to(DEV), params)
    on, off, plain = step(*args, ret_d_corr=True), step(*args, ret_d_corr=False), step(*args)
    assert len(on) == 4 and len(off) == len(plain) == 3 and tuple(on[3].shape) == (1, 324, 8, 12)
    for r in (on, off):
        assert torch.equal(r[0], plain[0]) and torch.equal(r[1], plain[1]) and len(r[2]) == 22 and all(torch.equal(a, b) for a, b in zip(r[2], plain[2]))
    r, r32 = ubref.ratio(on[3], w64), ubref.ratio(w32, w64)
    print(f'd_corr {shape}: GPU {r:.3e}  float32 on the CPU {r32:.3e}  ratio {r / r32:.2f}')
    assert bool(torch.isfinite(on[3]).all()) and r <= 2.0 * r32


# ------------------------------------------------------------------------------------------------------------------------ through time
@pytest.fixture(scope='module')
def raft_model(rpe):
    from rpe_amd import raft, synth
    return synth.init_synthetic_weights(raft.RAFT(synth.model_config(128, 136, iters=3))).eval().to(DEV)


def _whole_pass(f1, f2, net0, inp, coords, flows, Pu, Pt, gup, dtype):
    """(d fmap1, d fmap2) of sum(flow_up * gup) by autograd in ``dtype``: oracle CorrBlock (build and pooling) and its sampler at the detached
    coordinates (CorrBlock.__call__ without its final cast to float32), update_block_ref.step per iteration, raft_tail_ref.tail."""
    import raft_tail_ref as tref
    from oracle.raft import CorrBlock, bilinear_sampler
    f1, f2 = f1.to(dtype).requires_grad_(True), f2.to(dtype).requires_grad_(True)
    blk = CorrBlock(f1, f2)
    d = torch.arange(-4, 5, dtype=dtype)
    delta = torch.stack(torch.meshgrid(d, d, indexing='ij'), dim=-1).view(1, 9, 9, 2)
    Pu, Pt = {k: v.to(dtype) for k, v in Pu.items()}, {k: v.to(dtype) for k, v in Pt.items()}
    net, inp = net0.to(dtype), inp.to(dtype)
    b, _, h8, w8 = net.shape
    for co, fl in zip(coords, flows):
        cen = co.to(dtype).permute(0, 2, 3, 1).reshape(b * h8 * w8, 1, 1, 2)
        win = [bilinear_sampler(lvl, cen / 2 ** i + delta).view(b, h8, w8, -1) for i, lvl in enumerate(blk.corr_pyramid)]
        net = ubref.step(net, inp, torch.cat(win, -1).permute(0, 3, 1, 2), fl.to(dtype), Pu)
    up = tref.tail(net, flows[-1].to(dtype), Pt)[0]
    return torch.autograd.grad((up * gup.to(dtype)).sum(), [f1, f2])


def test_grad_corr_through_time_against_float64(rpe, raft_model):
    """RAFT.forward(grad_corr=True) at 128 x 136 (maps 16 x 17), 3 iterations, 2 pairs: fmap1.grad and fmap2.grad within twice the float32 CPU
    figure of float64 autograd over the whole restated pass; everything grad_update returns keeps its bits."""
    import raft_tail_ref as tref
    model, g = raft_model, _gen(17)
    im1, im2 = (255.0 * torch.rand(2, 3, 128, 136, generator=g)).to(DEV), (255.0 * torch.rand(2, 3, 128, 136, generator=g)).to(DEV)
    gup = torch.randn(2, 2, 128, 136, generator=g).to(DEV)
    fh, mk = model.head_params()
    upd = model.update_params()
    for p in fh + mk + upd:
        p.requires_grad_(True)
    try:
        def run(**kw):
            for p in model.parameters():
                p.grad = None
            r = model(im1, im2, ret_lowres=True, **kw)
            node = r[0][-1].grad_fn
            (r[0][-1] * gup).sum().backward()
            return r, node, [p.grad.clone() for p in fh + mk + upd]
        ra, node, pa = run(grad_corr=True)
        rb, _, pb = run(grad_update=True)
        assert len(ra) == 8 and len(rb) == 6 and all(t.is_leaf and t.requires_grad for t in ra[6:])
        assert tuple(ra[6].shape) == tuple(ra[7].shape) == (2, 256, 16, 17)
        assert torch.equal(ra[0][-1], rb[0][-1]) and all(torch.equal(a, b) for a, b in zip(ra[1:6], rb[1:]))          # flows, hidden, context, low, net_0, inp
        assert all(torch.equal(ra[i].grad, rb[i].grad) for i in (1, 4, 5))                                           # hidden.grad, net_0.grad, inp.grad
        assert len(pa) == 30 and all(torch.equal(a, b) for a, b in zip(pa, pb))
        f1, f2 = ra[6], ra[7]
        assert bool(torch.isfinite(f1.grad).all()) and bool(torch.isfinite(f2.grad).all()) and float(f1.grad.abs().max()) > 0 and float(f2.grad.abs().max()) > 0
        states = node.passes[0].states
        coords, flows = [co.cpu() for _, co in states], [st[:, 254:].cpu() for st, _ in states]
        Pu = {k: p.detach().cpu() for k, p in zip(ubref.PARAMS, upd)}
        Pt = {k: p.detach().cpu() for k, p in zip(tref.PARAMS, fh + mk)}
        args = (f1.detach().cpu(), f2.detach().cpu(), ra[4].detach().cpu(), ra[5].detach().cpu(), coords, flows, Pu, Pt, gup.cpu())
        w64, w32 = _whole_pass(*args, torch.float64), _whole_pass(*args, torch.float32)
        missed = []
        for name, got, t64, t32 in (('fmap1.grad', f1.grad, w64[0], w32[0]), ('fmap2.grad', f2.grad, w64[1], w32[1])):
            r, r32 = ubref.ratio(got, t64), ubref.ratio(t32, t64)
            print(f'through time {name}: GPU {r:.3e}  float32 on the CPU {r32:.3e}  ratio {r / r32:.2f}')
            if not r <= 2.0 * r32:
                missed.append((name, r, r32))
        assert not missed, missed
    finally:
        for p in model.parameters():
            p.requires_grad_(False)
            p.grad = None


# ---------------------------------------------------------------------------------------------------------------------------- PoseNet
def test_posenet_grad_corr_adds_the_feature_map_leaves(rpe):
    from rpe_amd import pose_net, synth
    h, w = 352, 352
    model = synth.init_synthetic_weights(pose_net.PoseNet(synth.model_config(h, w, iters=3, lbgfs_iters=100))).to(DEV)
    model.train().freeze_flow(True).freeze_flow(False, parts='update')
    a = {k: v.to(DEV) for k, v in synth.stereo_frames(3, 1, h, w).items()}
    target = torch.tensor([[0.004, -0.003, 0.002, 0.01, -0.008, 0.006]], device=DEV)

    def step(**kw):
        model.zero_grad(set_to_none=True)
        out = model(a['image1l'], a['image2l'], a['K'], a['baseline'], a['image2r'], a['image2r'], mask1=a['mask1'], mask2=a['mask2'],
                    ret_confmap=True, ret_flows=True, **kw)
        (out[0] - target).abs().sum().backward()
        return out, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        off, g_off = step()
        on, g_on = step(grad_corr=True)
        model.freeze_flow(True)
        frozen, g_frozen = step(grad_corr=True)                         # the update-block route although nothing of it trains
    assert 'fmap1' not in off[-1] and set(on[-1]) == set(off[-1]) | {'fmap1', 'fmap2'}
    for x, y in zip(on[:3], off[:3]):
        assert torch.equal(x, y)
    assert set(g_on) == set(g_off) and all(torch.equal(g_on[k], g_off[k]) for k in g_on)
    for key in ('time_flow', 'stereo_flow1', 'stereo_flow2'):
        assert torch.equal(on[-1][key].grad, off[-1][key].grad)
    for key in ('hidden', 'net0', 'inp'):
        assert all(torch.equal(on[-1][key][p].grad, off[-1][key][p].grad) for p in ('time', 'stereo1', 'stereo2')), key
    for d in (on[-1], frozen[-1]):
        for key in ('fmap1', 'fmap2'):
            for p in ('time', 'stereo1', 'stereo2'):
                t = d[key][p]
                assert t.is_leaf and tuple(t.shape) == (1, 256, 44, 44) and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0.0, (key, p)
    assert all(torch.equal(on[-1]['fmap1'][p].grad, frozen[-1]['fmap1'][p].grad) for p in ('time', 'stereo1', 'stereo2'))
    assert torch.equal(frozen[0], on[0]) and not any(k.startswith('flow.') for k in g_frozen)


def test_grad_corr_refusals_launch_nothing(rpe):
    from rpe_amd import _lib, pose_net, raft, synth
    img = torch.zeros(1, 3, 128, 160, device=DEV)
    model = raft.RAFT(dict(synth.model_config(128, 160), alternate_corr=True)).eval().to(DEV)
    with _lib.CountingLib() as count, pytest.raises(_lib.RpeError, match='alternate_corr'):
        model(img, img, grad_corr=True)
    assert count.calls == 0
    net = pose_net.PoseNet(synth.model_config(352, 352)).train().freeze_flow(True)
    with pytest.raises(NotImplementedError, match='encoders'):
        net.freeze_flow(False)
    with pytest.raises(_lib.RpeError, match='G must be'):
        ops_G = torch.zeros(1, 256, 339, device=DEV)
        from rpe_amd import ops
        ops.corr_lookup_backward(torch.zeros(1, 2, 16, 16, device=DEV), torch.zeros(1, 324, 16, 16, device=DEV), ops_G)
