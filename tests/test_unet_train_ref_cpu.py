"""CPU: the stage-by-stage restatement of csrc/unet_train.hip (tests/unet_train_ref.py) that tests/test_gpu_unet_train_edges.py holds
the kernels against.  Composition: the stages chained in float64 are ``forward_ref`` of tests/test_gpu_unet_train.py (TinyUNet.forward_train
itself on a grid that is a multiple of 4) and their adjoints are float64 autograd, to 1e-9 of each tensor's largest entry.  Mutation: the
check accepts the evaluation with the kernels' arithmetic (float64 sums rounded to float32 once, float32 elementwise stages) and rejects
each of ``MUTANTS`` at the stage it breaks, and nowhere else -- every stage is judged from the buffers on either side of it."""
import copy

import pytest
import torch

import unet_train_ref as R
from test_gpu_unet_train import forward_ref, make_net, run_cpu


def case(cin, h8, w8, n, seed, ties=False):
    out_sz = (8 * h8, 8 * w8)
    net = make_net(cin, out_sz, seed)
    g = torch.Generator().manual_seed(seed + 2000)
    x = torch.randn(n, cin, h8, w8, generator=g)
    return net, (R.plant_ties(x) if ties else x), torch.randn(n, 1, *out_sz, generator=g)


@pytest.mark.parametrize('train', [True, False], ids=['batch-stats', 'frozen'])
@pytest.mark.parametrize('h8,w8', [(44, 44), (45, 47)])
def test_stages_compose_to_forward_ref_and_float64_autograd(rpe, h8, w8, train):
    from rpe_amd import unet
    net, x, gout = case(8, h8, w8, 2, 5)
    net.train(train)
    truth = run_cpu(net, x, gout, torch.float64, train)
    if h8 % 4 == 0 and w8 % 4 == 0:
        with torch.no_grad():
            m1, m2 = copy.deepcopy(net).double().train(train), copy.deepcopy(net).double().train(train)
            assert torch.equal(forward_ref(m1, x.double()), m2.forward_train(x.double()))
    res = R.walk(R.inputs_of(net, x, gout, float32_constants=False), 'f64')
    names = {id(p): k for k, p in net.named_parameters()}
    order = [names[id(p)] for p in unet.train_params(net)]
    got = {'out': res['out'][0], 'grad.input': res['gin'][0]}
    got.update({'grad.' + k: res[f'grad.{i}'][0] for i, k in enumerate(order)})
    norm_names = [f'encoder.enc_blocks.{i}.norm' for i in range(3)] + [f'decoder.dec_blocks.{j}.norm' for j in range(2)]
    for k, nm in enumerate(norm_names):
        got[f'state.{nm}.running_mean'], got[f'state.{nm}.running_var'] = res[f'rm.{k}'][0], res[f'rv.{k}'][0]
    for k, t in truth.items():
        if k.endswith('num_batches_tracked'):
            continue
        scale = float(t.abs().max())
        if train and k.endswith('conv1.bias'):           # in front of a batch-statistics norm the true gradient is 0: judged on the weight's scale
            scale = float(truth[k[:-4] + 'weight'].abs().max())
        err = float((got[k].reshape(t.shape) - t).abs().max())
        assert err <= 1e-9 * scale, (k, err, scale)
    assert len(got) == len([k for k in truth if not k.endswith('num_batches_tracked')]) == 2 + 36 + 10


def test_the_sigmoid_composes_too(rpe):
    net, x, gout = case(8, 44, 44, 1, 6)
    net.train()
    m = copy.deepcopy(net).double()
    xi = x.double().requires_grad_(True)
    y = torch.sigmoid(forward_ref(m, xi))
    y.backward(gout.double())
    res = R.walk(R.inputs_of(net, x, gout, sigmoid=True, float32_constants=False), 'f64')
    assert float((res['out'][0] - y.detach()).abs().max()) <= 1e-9
    assert float((res['gin'][0] - xi.grad).abs().max()) <= 1e-9 * float(xi.grad.abs().max())


@pytest.fixture(scope='module')
def mutation_case(rpe):
    """45x47, n = 3, 264 channels, batch statistics, planted pool ties: odd maps, odd crop differences, two weight-gradient chunks at
    stage 0 and a 264 x 9-term convolution."""
    net, x, gout = case(264, 45, 47, 3, 9, ties=True)
    net.train()
    return R.inputs_of(net, x, gout, count=True)


def test_the_check_accepts_the_kernels_arithmetic_on_the_cpu(mutation_case):
    inp = mutation_case
    assert R.wchunks(3 * 43 * 45) == (4096, 2)
    run = R.buffers(R.walk(inp, 'kernel'))
    sk = run['skip.0'][..., :10, :10]
    assert bool((sk == sk[..., :1, :1]).all())                # the planted ties are there
    figs, bad = R.check_run(inp, run, 'cpu', beside=R.buffers(R.walk(inp, 'f32')))
    assert not bad, bad
    assert {f'grad.{k}' for k in range(36)} | {'out', 'gin', 'g_hm', 'rm.0', 'rv.4', 'nbt.0'} <= set(figs)
    for sigmoid in (True,):
        inp2 = dict(inp, sigmoid=sigmoid)
        _, bad = R.check_run(inp2, R.buffers(R.walk(inp2, 'kernel')), 'cpu sigmoid', verbose=False)
        assert not bad, bad
    frozen = dict(inp, train_mask=0)
    _, bad = R.check_run(frozen, R.buffers(R.walk(frozen, 'kernel')), 'cpu frozen', verbose=False)
    assert not bad, bad


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_each_mutant_is_rejected_by_the_stage_it_breaks(mutation_case, mutant):
    """The f32-accumulation mutant: one convolution of 264 x 9 terms added up in float32 (torch's float32 conv2d) in place of float64
    rounded once -- the bound u |t| + (k + 2) 2^-53 A sees it."""
    figs, bad = R.check_run(mutation_case, R.buffers(R.walk(mutation_case, 'kernel', mutant=mutant)), mutant, verbose=False)
    print(mutant, {k: figs[k] for k in bad})
    assert bad == [R.MUTANT_STAGE[mutant]], bad
