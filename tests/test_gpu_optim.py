"""GPU: rpe_grad_norm / rpe_adamw_step through optim.ClippedAdamW against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW on the CPU.

The table: tensors of 1, 2, 3, 5, CHUNK-1, CHUNK, CHUNK+1 and 2 CHUNK+5 elements (scalar heads and tails, exactly one chunk, one element
into the next, three chunks).  The CHUNK+1 parameter is a view 4 bytes into its storage, and so is its gradient (one phase: the float4
path behind a 3-element head); the 2 CHUNK+5 gradient is a view 8 bytes into its storage (another phase than its parameter: the
element-wise path; in the norm kernel a 2-element head); the 5-element gradient is strided (made contiguous by ``step``).

Truth is the same update in float64 on the CPU, the yardstick the same in float32 on the CPU; the bar is the project's (NOTES.md, "Whole-
network training"): error relative to max |truth| at most twice the float32 CPU run's.  Both errors are taken over ALL tensors of a kind
(parameters, exp_avg, exp_avg_sq) together: a 1- or 2-element tensor's float32 error is one or two rounding draws, zero as often as not,
and no multiple of it means anything; the small tensors' elements are in the maximum with everybody else's.  The per-tensor figures are
printed."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LR, BETAS, EPS, WD = 1e-2, (0.9, 0.999), 1e-8, 0.1
MAX_NORMS = (10.0, 1000.0, 50.0)              # the gradients' norms are ~72, ~215, ~357: clipped, not clipped, clipped


def _sizes():
    from rpe_amd import ops
    C = ops.optim_chunk()
    return (1, 2, 3, 5, C - 1, C, C + 1, 2 * C + 5)


def _values(seed, steps=3):
    g = torch.Generator().manual_seed(seed)
    sizes = _sizes()
    params = [torch.randn(n, generator=g) for n in sizes]
    grads = [[torch.randn(n, generator=g) * (0.5 + k) for n in sizes] for k in range(steps)]
    return params, grads


def _gpu_params(values):
    """Parameters on the GPU; index 6 is a view 4 bytes into its storage."""
    out = []
    for i, v in enumerate(values):
        if i == 6:
            base = torch.zeros(v.numel() + 1, device=DEV)
            p = torch.nn.Parameter(base[1:])
            assert p.data_ptr() % 16 == 4
            with torch.no_grad():
                p.copy_(v)
        else:
            p = torch.nn.Parameter(v.to(DEV))
        out.append(p)
    return out


def _set_grads(params, grads):
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            p.grad = None
        elif i in (6, 7):                                   # views 4 and 8 bytes into their storage
            lead = 1 if i == 6 else 2
            buf = torch.zeros(g.numel() + lead, device=DEV)
            buf[lead:] = g.to(DEV)
            p.grad = buf[lead:]
            assert p.grad.data_ptr() % 16 == 4 * lead
        elif i == 3:                                        # strided
            buf = torch.zeros(2 * g.numel(), device=DEV)
            buf[::2] = g.to(DEV)
            p.grad = buf[::2]
            assert not p.grad.is_contiguous()
        else:
            p.grad = g.to(DEV).clone()


def _make(values, **kw):
    from rpe_amd import optim
    params = _gpu_params(values)
    return params, optim.ClippedAdamW(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, **kw)


def _cpu_run(values, grads, max_norms, dtype, state=None):
    """clip_grad_norm_ + AdamW.step on the CPU in ``dtype`` -> (params, exp_avg, exp_avg_sq, norms)."""
    params = [torch.nn.Parameter(v.to(dtype).clone()) for v in values]
    opt = torch.optim.AdamW(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)
    if state is not None:
        opt.load_state_dict(state)
    norms = []
    for step_grads, mx in zip(grads, max_norms):
        for p, g in zip(params, step_grads):
            p.grad = None if g is None else g.to(dtype).clone()
        with_grad = [p for p in params if p.grad is not None]
        norms.append(torch.nn.utils.clip_grad_norm_(with_grad, mx if mx is not None else float('inf'), foreach=False).double())
        opt.step()
    st = [opt.state[p] for p in params]
    return [p.detach() for p in params], [s.get('exp_avg') for s in st], [s.get('exp_avg_sq') for s in st], norms


def _err(got, truth):
    """max |got - truth| over every tensor of the list, relative to max |truth| over the list."""
    pairs = [(g.detach().cpu().double().reshape(-1), t.double().reshape(-1)) for g, t in zip(got, truth) if t is not None]
    return max(float((g - t).abs().max()) for g, t in pairs) / max(float(t.abs().max()) for _, t in pairs)


def _check_bar(name, got, t64, t32):
    e, e32 = _err(got, t64), _err(t32, t64)
    for i, (g, a, b) in enumerate(zip(got, t64, t32)):
        if a is not None:
            print(f'  {name}[{i}] ({a.numel()} elements): GPU {_err([g], [a]):.3e}  float32 on the CPU {_err([b], [a]):.3e}')
    print(f'{name}: GPU {e:.3e}  float32 on the CPU {e32:.3e}  multiple {e / max(e32, 1e-300):.2f}')
    assert e <= 2.0 * e32, (name, e, e32)


def _moments(opt, params):
    return [opt.state[p].get('exp_avg') for p in params], [opt.state[p].get('exp_avg_sq') for p in params]


def _snapshot(opt, params):
    m, v = _moments(opt, params)
    return [t.detach().clone() for t in params] + [t.clone() for t in m + v if t is not None] + [opt.steps.clone(), opt.skipped.clone(), opt.last_norm.clone()]


def _run_gpu(values, grads, max_norms):
    params, opt = _make(values)
    norms = []
    for step_grads, mx in zip(grads, max_norms):
        _set_grads(params, step_grads)
        kept = [None if p.grad is None else p.grad.clone() for p in params]
        opt.param_groups[0]['max_norm'] = mx
        opt.step()
        for p, k in zip(params, kept):                      # the gradients are left as backward produced them
            assert k is None or torch.equal(p.grad, k)
        norms.append((opt.last_norm.clone(), opt.last_norm_f32.clone()))
    return params, opt, norms


def test_three_clipped_steps_against_float64(rpe):
    values, grads = _values(7)
    params, opt, norms = _run_gpu(values, grads, MAX_NORMS)
    p64, m64, v64, n64 = _cpu_run(values, grads, MAX_NORMS, torch.float64)
    p32, m32, v32, _ = _cpu_run(values, grads, MAX_NORMS, torch.float32)
    for k, ((nd, nf), truth) in enumerate(zip(norms, n64)):
        rel = abs(float(nd) - float(truth)) / float(truth)
        print(f'step {k}: norm {float(nd):.15e}  truth {float(truth):.15e}  relative {rel:.2e}  max_norm {MAX_NORMS[k]}')
        assert rel <= 1e-12
        assert float(nf) == float(torch.tensor(float(nd), dtype=torch.float64).float())
    assert float(norms[0][0]) > MAX_NORMS[0] and float(norms[1][0]) < MAX_NORMS[1] and float(norms[2][0]) > MAX_NORMS[2]      # clipped, not, clipped
    assert int(opt.steps) == 3 and int(opt.skipped) == 0
    m, v = _moments(opt, params)
    _check_bar('param', params, p64, p32)
    _check_bar('exp_avg', m, m64, m32)
    _check_bar('exp_avg_sq', v, v64, v32)
    # the clip is in the truth the bar was taken against: Adam's step hardly feels a gradient's scale (m / sqrt(v)), its first moment does
    _, mu, _, _ = _cpu_run(values, grads[:1], (None,), torch.float64)
    _, mc, _, _ = _cpu_run(values, grads[:1], MAX_NORMS[:1], torch.float64)
    assert _err(mu, mc) > 0.5


def test_two_runs_agree_to_the_bit(rpe):
    values, grads = _values(8)
    a_params, a_opt, a_norms = _run_gpu(values, grads, MAX_NORMS)
    b_params, b_opt, b_norms = _run_gpu(values, grads, MAX_NORMS)
    for x, y in zip(_snapshot(a_opt, a_params), _snapshot(b_opt, b_params)):
        assert torch.equal(x, y)
    for (x, xf), (y, yf) in zip(a_norms, b_norms):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64)) and torch.equal(xf, yf)


@pytest.mark.parametrize('where', ['nan-last-of-last', 'inf-first-of-first'])
def test_a_non_finite_gradient_skips_the_step(rpe, where):
    values, grads = _values(9)
    bad = [g.clone() for g in grads[1]]
    if where == 'nan-last-of-last':
        bad[-1][-1] = float('nan')
    else:
        bad[0][0] = float('inf')
    params, opt = _make(values, max_norm=MAX_NORMS[0])
    _set_grads(params, grads[0])
    opt.step()
    before = _snapshot(opt, params)
    versions = [p._version for p in params]
    _set_grads(params, bad)
    opt.step()
    after = _snapshot(opt, params)
    n = len(after) - 3
    for x, y in zip(before[:n], after[:n]):                 # every parameter and both moments keep their bits
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert int(opt.steps) == 1 and int(opt.skipped) == 1
    assert all(p._version > v for p, v in zip(params, versions))          # (bumped all the same: a repack of unchanged weights, never stale ones)
    _set_grads(params, grads[2])
    opt.step()
    clean_params, clean = _make(values, max_norm=MAX_NORMS[0])
    for k in (0, 2):
        _set_grads(clean_params, grads[k])
        clean.step()
    got, want = _snapshot(opt, params), _snapshot(clean, clean_params)
    for i, (x, y) in enumerate(zip(got, want)):
        if i != len(got) - 2:                               # (the skipped counters differ, by one)
            assert torch.equal(x, y), i
    assert int(opt.skipped) == 1 and int(clean.skipped) == 0 and int(opt.steps) == 2
    # a fresh optimizer whose FIRST step is the bad one: nothing moves, and the next step is a first step
    first_params, first = _make(values, max_norm=MAX_NORMS[0])
    _set_grads(first_params, bad)
    first.step()
    assert all(torch.equal(p.detach().cpu(), v) for p, v in zip(first_params, values)) and int(first.steps) == 0 and int(first.skipped) == 1
    assert all(not bool(t.any()) for mv in _moments(first, first_params) for t in mv)
    _set_grads(first_params, grads[0])
    first.step()
    ref_params, ref = _make(values, max_norm=MAX_NORMS[0])
    _set_grads(ref_params, grads[0])
    ref.step()
    assert all(torch.equal(x, y) for x, y in zip(first_params, ref_params))
    # skip_nonfinite=False takes the step, as a bare AdamW would
    loose_params, loose = _make(values, max_norm=None, skip_nonfinite=False)
    _set_grads(loose_params, bad)
    loose.step()
    assert int(loose.steps) == 1 and int(loose.skipped) == 0
    assert not bool(torch.isfinite(loose_params[-1 if where == 'nan-last-of-last' else 0]).all())


def test_a_parameter_without_a_gradient_is_left_alone(rpe):
    values, grads = _values(10)
    params, opt = _make(values, max_norm=MAX_NORMS[0])
    frozen = (1, 5)
    step_grads = [None if i in frozen else g for i, g in enumerate(grads[0])]
    _set_grads(params, step_grads)
    versions = [p._version for p in params]
    opt.step()
    for i, (p, v) in enumerate(zip(params, values)):
        if i in frozen:
            assert torch.equal(p.detach().cpu(), v) and p._version == versions[i] and 'exp_avg' not in opt.state[p]     # weight decay included
        else:
            assert not torch.equal(p.detach().cpu(), v) and p._version == versions[i] + 1
    p64, _, _, n64 = _cpu_run(values, [step_grads], MAX_NORMS[:1], torch.float64)
    p32, _, _, _ = _cpu_run(values, [step_grads], MAX_NORMS[:1], torch.float32)
    assert abs(float(opt.last_norm) - float(n64[0])) <= 1e-12 * float(n64[0])      # the norm is over the gradients that exist
    _check_bar('param (two frozen)', params, p64, p32)


@pytest.mark.parametrize('direction', ['hip-to-torch', 'torch-to-hip'])
def test_state_moves_between_the_two_optimizers(rpe, direction):
    values, grads = _values(11)
    mx = MAX_NORMS[0]
    if direction == 'hip-to-torch':
        params, opt, _ = _run_gpu(values, grads[:2], (mx, mx))
        state = opt.state_dict()
    else:
        params = [torch.nn.Parameter(v.to(DEV)) for v in values]
        opt = torch.optim.AdamW(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
        for k in range(2):
            for p, g in zip(params, grads[k]):
                p.grad = g.to(DEV).clone()
            torch.nn.utils.clip_grad_norm_(params, mx)
            opt.step()
        state = opt.state_dict()
    assert all(float(s['step']) == 2.0 for s in state['state'].values()) and len(state['state']) == len(values)
    now = [p.detach().cpu().clone() for p in params]
    # the third step: ClippedAdamW and torch.optim.AdamW on the GPU, each from the saved state over copies of the parameters
    hip_params, hip = _make(now, max_norm=mx)
    hip.load_state_dict(copy.deepcopy(state))               # (torch hands a loaded 'step' tensor on as it is, and steps it in place)
    _set_grads(hip_params, grads[2])
    hip.step()
    assert int(hip.steps) == 3
    tor_params = [torch.nn.Parameter(v.to(DEV)) for v in now]
    tor = torch.optim.AdamW(tor_params, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    tor.load_state_dict(copy.deepcopy(state))
    for p, g in zip(tor_params, grads[2]):
        p.grad = g.to(DEV).clone()
    torch.nn.utils.clip_grad_norm_(tor_params, mx)
    tor.step()
    cpu_state = lambda dtype: dict(state=copy.deepcopy(state['state']), param_groups=[dict(state['param_groups'][0], foreach=False, fused=None)])
    p64, m64, v64, _ = _cpu_run(now, grads[2:], (mx,), torch.float64, cpu_state(torch.float64))
    p32, m32, v32, _ = _cpu_run(now, grads[2:], (mx,), torch.float32, cpu_state(torch.float32))
    m, v = _moments(hip, hip_params)
    _check_bar(f'{direction} ClippedAdamW param', hip_params, p64, p32)
    _check_bar(f'{direction} ClippedAdamW exp_avg', m, m64, m32)
    _check_bar(f'{direction} ClippedAdamW exp_avg_sq', v, v64, v32)
    _check_bar(f'{direction} torch.optim.AdamW param', tor_params, p64, p32)


def test_same_bits_as_torch_on_the_gpu(rpe):
    """Without a clip, ClippedAdamW takes torch.optim.AdamW's roundings on the GPU: two models stepped by the two from the same gradients
    keep the same weights, so a comparison of two training runs compares the runs and not their first diverging ulp."""
    values, grads = _values(13)
    params, opt = _make(values, max_norm=None)
    twins = [torch.nn.Parameter(v.to(DEV)) for v in values]
    tor = torch.optim.AdamW(twins, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    for k in range(3):
        _set_grads(params, grads[k])
        opt.step()
        for p, g in zip(twins, grads[k]):
            p.grad = g.to(DEV).clone()
        tor.step()
        for i, (a, b) in enumerate(zip(params, twins)):
            assert torch.equal(a.detach(), b.detach()), (k, i)
            assert torch.equal(opt.state[a]['exp_avg'], tor.state[b]['exp_avg']) and torch.equal(opt.state[a]['exp_avg_sq'], tor.state[b]['exp_avg_sq']), (k, i)


def test_edges(rpe):
    from rpe_amd import _lib, optim
    values, _ = _values(12)
    params, opt = _make(values, max_norm=1.0)
    with _lib.CountingLib() as c:
        assert opt.step() is None                           # no parameter has a gradient: nothing is launched, nothing raised
    assert c.calls == 0 and int(opt.steps) == 0 and all(p._version == 0 or torch.equal(p.detach().cpu(), v) for p, v in zip(params, values))
    with pytest.raises(ValueError, match='float32 parameters on the GPU'):
        optim.ClippedAdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64, device=DEV))], lr=1e-3)
    with pytest.raises(ValueError, match='float32 parameters on the GPU'):
        optim.ClippedAdamW([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
    # the table is uploaded when a pointer changes, not otherwise
    g = [torch.ones_like(p) for p in params]
    for p, x in zip(params, g):
        p.grad = x
    opt.step()
    opt.step()
    assert opt._table.uploads == 1
    params[0].grad = torch.ones_like(params[0])
    opt.step()
    assert opt._table.uploads == 2 and int(opt.steps) == 3
