"""GPU: the backward through time with a gradient at EVERY iteration's prediction -- raft_grad's node with GradPass.earlier, through
RAFT.grad_pass / RAFT.forward(all_flows=True, grad_all_flows=True).  128 x 128, 3 iterations, two passes over three images encoded once
(tests/test_gpu_raft_whole.py's arrangement).  Truth: float64 autograd on the CPU through the whole model under the LINEAR functional
sum_k <up_k, G_k> (tests/raft_seq_ref.py says why not L1); the bar is the project's -- an error relative to max |truth| of at most twice
that of the same autograd in float32 on the CPU.  ReLU decisions are discrete: SEED is the first from 53 on for which the float32 and
the float64 CPU references decide every ReLU input alike, the heads' pre-activations at every net_k included (searched on the CPU with
raft_whole_ref.forward_states: 53 .. 56 are skipped; asserted below on the states the GPU pass saved: a condition on the inputs)."""
import pytest
import torch

import raft_seq_ref as sref
import raft_whole_ref as wref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED, ITERS = 57, 3
ROWS = ((0, 1), (1, 2), (0, 1))
_SHARED = {}


def _model(seed=SEED, **cfg):
    from rpe_amd import raft, synth
    model = synth.init_synthetic_weights(raft.RAFT(synth.model_config(128, 128, iters=ITERS, **cfg))).eval()
    case = sref.make_case(model, seed, ITERS)
    model = model.to(DEV)
    for p in model.parameters():
        p.requires_grad_(True)
    return model, case


def _params(model):
    from rpe_amd import raft_grad
    fh, mk = model.head_params()
    params = raft_grad.encoder_params(model.fnet) + raft_grad.encoder_params(model.cnet) + list(fh + mk + model.update_params())
    assert len(params) == 124 and len({id(p) for p in params}) == 124
    return params


def _two_passes(model, case, weights, all_flows=True):
    """Rows of ONE batched pass over three images encoded once: A -> B and B -> C with contexts A, B; loss = sum_k weights[k] <up_k, G_k>
    over both passes.  ``all_flows=False``: the node without the extra outputs, the loss on the last prediction."""
    from rpe_amd import raft_grad
    A, B, C = (im.to(DEV) for im in case['images'])
    for p in model.parameters():
        p.grad = None
    with torch.no_grad():
        f = model.encode_features([A, B, C])
        cn = model.encode_context([A, B])
        kw = dict(all_flows=True, grad_all_flows=True) if all_flows else {}
        _, whole = model.grad_pass((f[:2], f[1:]), cn, stages='encoders', upsample=True, sources=(((A, B, C), 0, 2), ((A, B, C), 1, 3), ((A, B), 0, 2)), **kw)
    passes = [whole.rows(0, 1), whole.rows(1, 2)]
    enc = (model.fnet, model.cnet)
    if all_flows:
        outs, early = raft_grad.attach(passes, model.head_params(), model.update_params(), enc, ret_earlier=True)
        flows = [e + [o[0]] for e, o in zip(early, outs)]
        assert all(len(fl) == ITERS and all(x.grad_fn is fl[-1].grad_fn for x in fl) for fl in flows)
    else:
        flows = [[None] * (ITERS - 1) + [o[0]] for o in raft_grad.attach(passes, model.head_params(), model.update_params(), enc)]
    loss = sum(w * (fl[k] * case['g_ups'][k][i:i + 1].to(DEV)).sum() for i, fl in enumerate(flows) for k, w in enumerate(weights) if w)
    loss.backward()
    return whole, [None if p.grad is None else p.grad.clone() for p in _params(model)]


def _shared():
    """The GPU pass and the CPU truths, computed once."""
    if not _SHARED:
        model, case = _model()
        whole, got = _two_passes(model, case, (1, 1, 1))
        coords, flows = [co.cpu() for _, co in whole.states], [st[:, 254:].cpu() for st, _ in whole.states]
        args = (model, case['images'], *ROWS, coords, flows)
        ups64, p64, s64, nets64 = sref.forward(*args, torch.float64)
        ups32, p32, s32, nets32 = sref.forward(*args, torch.float32)
        _SHARED.update(model=model, case=case, whole=whole, got=got, t64=(ups64, p64), t32=(ups32, p32), same=wref.same_relu_decisions(s32, s64),
                       nets=(nets32, nets64))
    return _SHARED


NAMES = [f'fnet.p{i}' for i in range(32)] + [f'cnet.p{i}' for i in range(62)] + [f'heads.p{i}' for i in range(8)] + [f'update.p{i}' for i in range(22)]
FNET_CONV_BIAS = {f'fnet.p{i}' for i in range(1, 30, 2)}                  # cancelled by the instance norm: exact zeros


def _against_float64(tag, got, w64, w32, names=NAMES):
    missed, lo, hi = [], (float('inf'), None), (0.0, None)
    for name, g, t64, t32 in zip(names, got, w64, w32):
        assert g is not None and bool(torch.isfinite(g).all()), name
        if name in FNET_CONV_BIAS:
            assert not bool(g.any()) and float(t64.abs().max()) < 1e-9, name
            continue
        if float(t64.abs().max()) == 0.0:                               # (convf1 under a gradient on prediction 1 alone: its input, flow_0, is zero)
            assert not bool(g.any()), name
            continue
        assert float(g.abs().max()) > 0, name
        r, r32 = wref.ratio(g, t64), wref.ratio(t32, t64)
        q = r / max(r32, 1e-300)
        lo, hi = min(lo, (q, name)), max(hi, (q, name))
        print(f'{tag} {name}: GPU {r:.3e}  float32 on the CPU {r32:.3e}  ratio {q:.2f}')
        if not r <= 2.0 * r32:
            missed.append((name, r, r32))
    print(f'{tag}: ratios {lo[0]:.2f} ({lo[1]}) .. {hi[0]:.2f} ({hi[1]})')
    assert not missed, missed


def test_every_prediction_against_float64(rpe):
    """All 124 gradients under sum_k <up_k, G_k>, every G_k random; two runs, the same bits.
    One MI355X run: ratios 0.12 (cnet.p1) .. 1.58 (cnet.p54).  (With the steps' parameter gradients in a float32 chain and every weight
    gradient one chain over the map, update.p14 -- encoder.convc2.weight -- stood at 2.44: NOTES.md, "Sequence loss".)"""
    S = _shared()
    same, differ = S['same']
    assert same, f'seed {SEED}: float32 and float64 decide {differ} ReLU inputs differently'
    whole = S['whole']
    print(f'seq forward: net_N of the pass {wref.ratio(whole.hidden, S["nets"][1][-1]):.3e}  float32 on the CPU {wref.ratio(S["nets"][0][-1], S["nets"][1][-1]):.3e}')
    for k in range(ITERS - 1):                                          # the inputs of the earlier tails are what the truth's heads read
        assert wref.ratio(whole.states[k + 1][0][:, :128], S['nets'][1][k]) < 1e-3, k
    g_ups = S['case']['g_ups']
    w64, w32 = sref.grads(*S['t64'], g_ups), sref.grads(*S['t32'], g_ups)
    _against_float64('seq', S['got'], w64, w32)
    _, again = _two_passes(S['model'], S['case'], (1, 1, 1))
    for name, a, b in zip(NAMES, S['got'], again):
        assert torch.equal(a, b), name


def test_first_prediction_only_against_float64(rpe):
    """A gradient on prediction 1 of N alone: one tail, one step, the encoders.  Every gradient is non-zero but convf1's (its input is the
    zero flow of a cold start: exact zeros, as the truth's).  One MI355X run: ratios 0.07 (cnet.p9) .. 1.50 (fnet.p18)."""
    S = _shared()
    _, got = _two_passes(S['model'], S['case'], (1, 0, 0))
    g_ups = [S['case']['g_ups'][0], None, None]
    _against_float64('seq k=0', got, sref.grads(*S['t64'], g_ups), sref.grads(*S['t32'], g_ups))


def test_last_prediction_only_is_the_plain_node_to_the_bit(rpe):
    S = _shared()
    _, with_outputs = _two_passes(S['model'], S['case'], (0, 0, 1))
    _, plain = _two_passes(S['model'], S['case'], (0, 0, 1), all_flows=False)
    for name, a, b in zip(NAMES, with_outputs, plain):
        assert a is not None and torch.equal(a, b), name


def test_every_depth_runs(rpe):
    """RAFT.forward at each of the four depths: the gradients a depth reaches are there and finite, those it does not reach are absent,
    and what two depths share (the heads' sum of N tails; from 'update' on the update block's) is equal to the bit."""
    S = _shared()
    model, case = S['model'], S['case']
    A, B = case['images'][0].to(DEV), case['images'][1].to(DEV)
    params, seen = _params(model), {}
    plain = model(A, B, all_flows=True)[0]
    for depth, reach in (('heads', range(94, 102)), ('update', range(94, 124)), ('corr', range(94, 124)), ('encoders', range(0, 124))):
        for p in params:
            p.grad = None
        r = model(A, B, all_flows=True, grad_all_flows=True, **{'grad_' + depth: True})
        flows = r[0]
        assert len(flows) == ITERS and all(f.grad_fn is flows[-1].grad_fn for f in flows) and all(torch.equal(f, q) for f, q in zip(flows, plain))
        sum((f * case['g_ups'][k][:1].to(DEV)).sum() for k, f in enumerate(flows)).backward()
        for i, p in enumerate(params):
            assert (p.grad is not None) == (i in reach), (depth, NAMES[i])
            if p.grad is not None and NAMES[i] not in FNET_CONV_BIAS:
                assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (depth, NAMES[i])
        seen[depth] = [None if p.grad is None else p.grad.clone() for p in params]
    for depth in ('update', 'corr', 'encoders'):
        assert all(torch.equal(seen[depth][i], seen['heads'][i]) for i in range(94, 102)), depth
        assert all(torch.equal(seen[depth][i], seen['update'][i]) for i in range(102, 124)), depth


def test_pad_maps_against_the_generic_route(rpe):
    """136 x 144 (17 x 18 maps: no tuned kernel takes them; tests/test_gpu_pad_maps.py's odd size -- at 136 x 120 the correlation pyramid
    refuses the 17 x 15 map before anything runs), depth 'update': the padded loop's 30 gradients against the unpadded generic route's.  tests/test_gpu_pad_maps.py sets no tolerance for gradients, so the bar is (a)'s: the distance between the two routes,
    relative to max |generic|, at most twice the error of float32 autograd on the CPU against float64 (on the generic pass's states)."""
    from rpe_amd import raft, synth
    h, w = 136, 144
    g = wref.gen(SEED)
    base = synth.init_synthetic_weights(raft.RAFT(synth.model_config(h, w, iters=ITERS))).eval()
    wref.seed_batch_norms(base.cnet, g)
    images = [255.0 * torch.rand(1, 3, h, w, generator=g) for _ in range(2)]
    g_ups = [torch.randn(1, 2, h, w, generator=g) for _ in range(ITERS)]
    got, recs = {}, {}
    for pad in (False, True):
        model = synth.init_synthetic_weights(raft.RAFT(synth.model_config(h, w, iters=ITERS, pad_maps=pad))).eval()
        model.load_state_dict(base.state_dict())
        model = model.to(DEV)
        for p in model.parameters():
            p.requires_grad_(True)
        r = model(images[0].to(DEV), images[1].to(DEV), all_flows=True, grad_update=True, grad_all_flows=True)
        recs[pad] = r[0][-1].grad_fn.passes[0]
        sum((f * g_ups[k].to(DEV)).sum() for k, f in enumerate(r[0])).backward()
        fh, mk = model.head_params()
        got[pad] = [p.grad.clone() for p in fh + mk + model.update_params()]
        last = model
    assert recs[True].states[0][0].shape == recs[False].states[0][0].shape == (1, 256, 17, 18)
    rec = recs[False]
    coords, flows = [co.cpu() for _, co in rec.states], [st[:, 254:].cpu() for st, _ in rec.states]
    args = (last, images, (0,), (1,), (0,), coords, flows)
    ups64, p64, s64, _ = sref.forward(*args, torch.float64)
    ups32, p32, s32, _ = sref.forward(*args, torch.float32)
    w64, w32 = sref.grads(ups64, p64, g_ups)[94:], sref.grads(ups32, p32, g_ups)[94:]
    print('pad_maps: float32 and float64 decide alike', wref.same_relu_decisions(s32, s64))
    missed = []
    for name, a, b, t64, t32 in zip(NAMES[94:], got[True], got[False], w64, w32):
        r, r32, rg = wref.ratio(a, b.cpu()), wref.ratio(t32, t64), wref.ratio(b, t64)
        print(f'pad_maps {name}: padded against generic {r:.3e}  generic against float64 {rg:.3e}  float32 on the CPU {r32:.3e}  ratio {r / max(r32, 1e-300):.2f}')
        if not r <= 2.0 * r32:
            missed.append((name, r, r32))
    assert not missed, missed
