"""Test infrastructure: the CPU truth of whole-network training (tests/test_gpu_raft_whole.py) -- autograd in float64 or float32 through the
whole of RAFT for passes that share one encoder batch: oracle encoders on the distinct images, oracle CorrBlock sampled at the passes'
saved (detached) coordinates, update_block_ref's step per iteration, raft_tail_ref's heads and up-sampling applied to coords1 - coords0
as the model forms it, and a loss that reads the up-sampled flow, the
last hidden state and the context.  The construction of _chain_truth in tests/test_gpu_encoder_backward.py, at any batch, with every ReLU
input collected so that a case can be held to the condition that float32 and float64 take every ReLU decision alike."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import raft_tail_ref as tref
import update_block_ref as ubref


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ratio(got, want):
    return float((got.detach().cpu().double() - want.detach().double()).abs().max()) / max(float(want.detach().abs().max()), 1e-300)


def seed_batch_norms(module, g):
    """Every batch norm's weight, bias and running statistics moved away from 1, 0, 0, 1 with draws from ``g``, as
    test_the_chain_trains_both_encoders does."""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_((1 + 0.2 * torch.randn(m.weight.shape, generator=g)).to(m.weight.device))
                m.bias.copy_((0.2 * torch.randn(m.bias.shape, generator=g)).to(m.weight.device))
                m.running_mean.copy_((0.2 * torch.randn(m.bias.shape, generator=g)).to(m.weight.device))
                m.running_var.copy_((0.7 + 0.6 * torch.rand(m.bias.shape, generator=g)).to(m.weight.device))


def make_case(model, seed, n_images=3, n_pass=2, size=128):
    """One case from ``seed``, drawn on the CPU in a fixed order: cnet's batch norms (seed_batch_norms, in place on ``model``), then the
    images (1,3,size,size) 0..255 and, per pass, the gradients of the up-sampled flow, of hidden_out and of context_out."""
    g = gen(seed)
    seed_batch_norms(model.cnet, g)
    return dict(images=[255.0 * torch.rand(1, 3, size, size, generator=g) for _ in range(n_images)],
                g_up=torch.randn(n_pass, 2, size, size, generator=g), g_hid=torch.randn(n_pass, 128, size // 8, size // 8, generator=g),
                g_ctx=torch.randn(n_pass, 128, size // 8, size // 8, generator=g))


def _block(blk, x, pres):
    p1 = blk.norm1(blk.conv1(x))
    p2 = blk.norm2(blk.conv2(torch.relu(p1)))
    p3 = (x if blk.downsample is None else blk.downsample(x)) + torch.relu(p2)
    pres += [p1, p2, p3]
    return torch.relu(p3)


def _encoder(enc, x, pres, split_act):
    p0 = enc.norm1(enc.conv1(x))
    pres.append(p0)
    x = torch.relu(p0)
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for blk in layer:
            x = _block(blk, x, pres)
    x = enc.conv2(x)
    if split_act:
        half = x.shape[1] // 2
        pres.append(x[:, half:])
        x = torch.cat((torch.tanh(x[:, :half]), torch.relu(x[:, half:])), 1)
    return x


def _step(net, inp, corr, flow, P, pres):
    """update_block_ref.step with the motion encoder's five ReLU inputs collected."""
    pre = ubref.encoder_pre(flow, corr, P)
    pres += list(pre.values())
    x = torch.cat((inp, torch.relu(pre['cv']), flow), 1)
    for hf in ('1', '2'):
        hx = torch.cat((net, x), 1)
        z, r = torch.sigmoid(ubref._conv(hx, P, 'z' + hf)), torch.sigmoid(ubref._conv(hx, P, 'r' + hf))
        q = torch.tanh(ubref._conv(torch.cat((r * net, x), 1), P, 'q' + hf))
        net = (1 - z) * net + z * q
    return net


def oracle_encoders(model, dtype):
    from oracle.raft import BasicEncoder
    encs = []
    for kind, src in (('instance', model.fnet), ('batch', model.cnet)):
        e = BasicEncoder(output_dim=256, norm_fn=kind)
        e.load_state_dict({k: v.detach().cpu() for k, v in src.state_dict().items()})
        e = e.eval().to(dtype)
        for p in e.parameters():
            p.requires_grad_(True)
        encs.append(e)
    return encs


def whole_truth(model, images, rows1, rows2, rows_c, coords, flows, g_up, g_hid, g_ctx, dtype):
    """d loss / d (all 124 parameters) of  loss = sum(flow_up g_up) + sum(net_N g_hid) + sum(inp g_ctx)  over a batched pass by autograd in
    ``dtype``: ``images`` = the distinct images (CPU, 0..255), encoded ONCE by fnet; fmap1 / fmap2 = its rows ``rows1`` / ``rows2``, the
    context = cnet on the images ``rows_c``; ``coords`` / ``flows`` = per iteration the pass's saved coords1_k and flow_k (constants).
    -> (the gradients in the order fnet's 32, cnet's 62 (raft_grad.encoder_params), the eight heads', the 22 of UPDATE_PARAMS; the
    sign (> 0) of every ReLU input, in a fixed order; this forward's net_N)."""
    from oracle.raft import CorrBlock, bilinear_sampler
    from rpe_amd import raft_grad
    fnet, cnet = oracle_encoders(model, dtype)
    norm = lambda ims: 2 * (torch.cat(ims, 0).to(dtype) / 255.0) - 1.0
    pres = []
    f = _encoder(fnet, norm(images), pres, False)
    c = _encoder(cnet, norm([images[i] for i in rows_c]), pres, True)
    f1, f2 = f[list(rows1)], f[list(rows2)]
    net, inp = c[:, :128], c[:, 128:]
    leaf = lambda p: p.detach().cpu().to(dtype).requires_grad_(True)
    Pu = {k: leaf(p) for k, p in zip(ubref.PARAMS, model.update_params())}
    fh, mk = model.head_params()
    Pt = {k: leaf(p) for k, p in zip(tref.PARAMS, fh + mk)}
    blk = CorrBlock(f1, f2)
    dd = torch.arange(-4, 5, dtype=dtype)
    delta = torch.stack(torch.meshgrid(dd, dd, indexing='ij'), dim=-1).view(1, 9, 9, 2)
    b, _, h8, w8 = net.shape
    for co, fl in zip(coords, flows):
        cen = co.to(dtype).permute(0, 2, 3, 1).reshape(b * h8 * w8, 1, 1, 2)
        win = [bilinear_sampler(lvl, cen / 2 ** i + delta).view(b, h8, w8, -1) for i, lvl in enumerate(blk.corr_pyramid)]
        net = _step(net, inp, torch.cat(win, -1).permute(0, 3, 1, 2), fl.to(dtype), Pu, pres)
    # the last iteration's heads as the model applies them (oracle.raft.RAFT.forward): coords1 <- coords1 + delta, and the up-sampled
    # prediction reads coords1 - coords0 -- in float32 a rounding at the magnitude of the coordinates, not of the flow, which raft_tail_ref's
    # flow_prev + delta would skip; in float64 the two agree to 1e-15
    from oracle.raft import coords_grid
    a_f, a_m = tref.pre_activations(net, Pt)
    pres += [a_f, a_m]
    delta = F.conv2d(torch.relu(a_f), Pt['fh2_w'], Pt['fh2_b'], padding=1)
    mask = 0.25 * F.conv2d(torch.relu(a_m), Pt['m2_w'], Pt['m2_b'])
    up = tref.upsample_convex((coords[-1].to(dtype) + delta) - coords_grid(b, h8, w8).to(dtype), mask)
    loss = (up * g_up.to(dtype)).sum() + (net * g_hid.to(dtype)).sum() + (inp * g_ctx.to(dtype)).sum()
    params = raft_grad.encoder_params(fnet) + raft_grad.encoder_params(cnet) + [Pt[k] for k in tref.PARAMS] + [Pu[k] for k in ubref.PARAMS]
    return torch.autograd.grad(loss, params, allow_unused=True), [(p.detach() > 0) for p in pres], net.detach()


def same_relu_decisions(signs_a, signs_b):
    """Do two runs of whole_truth take every ReLU decision alike?  -> (yes / no, the number of inputs decided differently)."""
    differ = sum(int((a != b).sum()) for a, b in zip(signs_a, signs_b))
    return differ == 0, differ


@torch.no_grad()
def forward_states(model, images, rows1, rows2, rows_c, iters):
    """The pass's (coords1_k, flow_k), k = 1 .. iters, computed on the CPU in float32 by the same restatement (cold start): what a
    search for a case's seed uses in place of the states the GPU pass saves."""
    from oracle.raft import CorrBlock, coords_grid
    fnet, cnet = oracle_encoders(model, torch.float32)
    norm = lambda ims: 2 * (torch.cat(ims, 0) / 255.0) - 1.0
    f = _encoder(fnet, norm(images), [], False)
    c = _encoder(cnet, norm([images[i] for i in rows_c]), [], True)
    net, inp = c[:, :128], c[:, 128:]
    Pu = {k: p.detach().cpu() for k, p in zip(ubref.PARAMS, model.update_params())}
    fh, mk = model.head_params()
    Pt = {k: p.detach().cpu() for k, p in zip(tref.PARAMS, fh + mk)}
    blk = CorrBlock(f[list(rows1)], f[list(rows2)])
    b, _, h8, w8 = net.shape
    coords0 = coords_grid(b, h8, w8)
    coords1, out = coords0.clone(), []
    for _ in range(iters):
        flow = coords1 - coords0
        out.append((coords1.clone(), flow))
        net = ubref.step(net, inp, blk(coords1), flow, Pu)
        coords1 = tref.tail(net, flow, Pt)[1] + coords0
    return [co for co, _ in out], [fl for _, fl in out]
