"""Test infrastructure: the CPU truth of training RAFT on a loss over EVERY iteration's prediction (tests/test_gpu_raft_seq_backward.py) --
raft_whole_ref's restatement of the whole model with the output heads and the convex up-sampling applied behind every iteration as the
model applies them: prediction k reads (coords1_k + delta_k) - coords0 (in float32 a rounding at the magnitude of the coordinates), the
saved coords1_k and flow_k being constants of their iteration.  The loss is a LINEAR functional  sum_k <up_k, G_k>  with given G_k: an L1
loss differentiated through a float64 forward would take sign(pred - gt) of predictions that differ from the float32 ones, and no
tolerance holds where a sign flips.  The heads' two ReLU inputs at every net_k join the ReLU inputs whose decisions a case must take
alike in float32 and float64."""
import torch
import torch.nn.functional as F

import raft_tail_ref as tref
import raft_whole_ref as wref
import update_block_ref as ubref


def forward(model, images, rows1, rows2, rows_c, coords, flows, dtype):
    """The restated forward in ``dtype`` with autograd on -> (the N up-sampled predictions, the 124 parameters in whole_truth's order, the
    sign (> 0) of every ReLU input in a fixed order, every iteration's net_k detached)."""
    from oracle.raft import CorrBlock, bilinear_sampler, coords_grid
    from rpe_amd import raft_grad
    fnet, cnet = wref.oracle_encoders(model, dtype)
    norm = lambda ims: 2 * (torch.cat(ims, 0).to(dtype) / 255.0) - 1.0
    pres = []
    f = wref._encoder(fnet, norm(images), pres, False)
    c = wref._encoder(cnet, norm([images[i] for i in rows_c]), pres, True)
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
    grid = coords_grid(b, h8, w8).to(dtype)
    ups, nets = [], []
    for co, fl in zip(coords, flows):
        cen = co.to(dtype).permute(0, 2, 3, 1).reshape(b * h8 * w8, 1, 1, 2)
        win = [bilinear_sampler(lvl, cen / 2 ** i + delta).view(b, h8, w8, -1) for i, lvl in enumerate(blk.corr_pyramid)]
        net = wref._step(net, inp, torch.cat(win, -1).permute(0, 3, 1, 2), fl.to(dtype), Pu, pres)
        a_f, a_m = tref.pre_activations(net, Pt)
        pres += [a_f, a_m]
        d_flow = F.conv2d(torch.relu(a_f), Pt['fh2_w'], Pt['fh2_b'], padding=1)
        mask = 0.25 * F.conv2d(torch.relu(a_m), Pt['m2_w'], Pt['m2_b'])
        ups.append(tref.upsample_convex((co.to(dtype) + d_flow) - grid, mask))
        nets.append(net.detach())
    params = raft_grad.encoder_params(fnet) + raft_grad.encoder_params(cnet) + [Pt[k] for k in tref.PARAMS] + [Pu[k] for k in ubref.PARAMS]
    return ups, params, [(p.detach() > 0) for p in pres], nets


def grads(ups, params, g_ups):
    """d / d params of  sum_k <ups[k], g_ups[k]>  over the k whose g_ups[k] is not None; the graph stays for another functional."""
    loss = sum((u * g.to(u.dtype)).sum() for u, g in zip(ups, g_ups) if g is not None)
    return torch.autograd.grad(loss, params, allow_unused=True, retain_graph=True)


def make_case(model, seed, iters, n_images=3, n_pass=2, size=128):
    """raft_whole_ref.make_case's draws (cnet's batch norms in place, then the images), then one G_k (n_pass,2,size,size) per iteration."""
    case = wref.make_case(model, seed, n_images, n_pass, size)
    g = wref.gen(seed + 100003)
    case['g_ups'] = [torch.randn(n_pass, 2, size, size, generator=g) for _ in range(iters)]
    return case


def decides_alike(model, case, rows1, rows2, rows_c, iters, states=None):
    """Do float32 and float64 take every ReLU decision alike on this case?  ``states`` = (coords, flows) the GPU pass saved, else the
    CPU restatement's (raft_whole_ref.forward_states: what a search for a seed uses) -> (yes / no, inputs decided differently)."""
    coords, flows = states if states is not None else wref.forward_states(model, case['images'], rows1, rows2, rows_c, iters)
    with torch.no_grad():
        s32 = forward(model, case['images'], rows1, rows2, rows_c, coords, flows, torch.float32)[2]
        s64 = forward(model, case['images'], rows1, rows2, rows_c, coords, flows, torch.float64)[2]
    return wref.same_relu_decisions(s32, s64)
