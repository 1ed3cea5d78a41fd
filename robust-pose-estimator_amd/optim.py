"""``ClippedAdamW``: the reference's parameter update -- ``GradScaler.unscale_`` / ``clip_grad_norm_`` / ``AdamW.step`` through ``scaler.step``
(scripts/train_posenet.py:115-133) -- as two launches of csrc/optim.hip and no host synchronisation.  The reference never enters an
autocast context, so its scaler's one observable effect is kept: a step whose gradients hold a NaN or an Inf is skipped.

``step()`` bumps the version counter of every parameter it wrote.  The kernels write through raw pointers, which autograd does not see,
and everything the package derives from weights -- packed Winograd and GEMM weights, folded batch norms, recorded launch lists -- is
cached under ``(tensor._version, data_ptr)`` (ops.wkey): without the bump the next forward would replay the old weights without a word.
A skipped step bumps the versions too (whether it was skipped is known on the device only): a repack of unchanged weights, never stale ones.

State follows torch.optim.AdamW's layout (per parameter ``step``, ``exp_avg``, ``exp_avg_sq``), so ``state_dict()`` loads into a
torch.optim.AdamW over the same parameters and the other way round.  One step counter on the device serves every parameter (they all
step together or not at all); ``state_dict()`` materialises it per parameter -- which reads it: saving synchronises, stepping does not."""
import torch

from . import ops

try:
    _bump = torch.autograd.graph.increment_version
except AttributeError:                                    # an older torch: its private spelling, else an in-place op that changes no bit
    _unsafe = getattr(torch._C._autograd, '_unsafe_set_version_counter', None)

    def _bump(t):
        if _unsafe is not None:
            _unsafe(t, t._version + 1)
        else:
            with torch.no_grad():
                t.detach().bitwise_or_(0) if not t.is_floating_point() else t.detach().view(torch.int32).bitwise_or_(0)


class ClippedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, skip_nonfinite=True):
        if not lr >= 0.0 or not eps >= 0.0 or not weight_decay >= 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f'ClippedAdamW: lr, eps, weight_decay must be >= 0 and the betas in [0, 1): got {lr}, {eps}, {weight_decay}, {betas}')
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, max_norm=max_norm, skip_nonfinite=skip_nonfinite))
        if len(self.param_groups) != 1:
            raise ValueError('ClippedAdamW: one parameter group (as the reference trains); several groups are not supported')
        params = self.param_groups[0]['params']
        devices = {p.device for p in params}
        for p in params:
            if not (p.is_cuda and p.dtype == torch.float32):
                raise ValueError(f'ClippedAdamW: float32 parameters on the GPU only (the update is a HIP kernel): got {p.dtype} on {p.device}')
            if not p.is_contiguous():
                raise ValueError('ClippedAdamW: parameters must be contiguous')
        if len(devices) > 1:
            raise ValueError(f'ClippedAdamW: the parameters live on {len(devices)} devices; one optimizer drives one GPU')
        device = next(iter(devices)) if devices else torch.device('cuda')
        self._record = ops.optim_record(device) if devices else None
        self._counters = torch.zeros(2, dtype=torch.int64, device=device) if devices else None      # [steps taken, steps skipped]
        self._table = ops.OptimTable()

    # -------------------------------------------------------------------------------------------------------------------- device state
    @property
    def last_norm(self):
        """(1,) float64 on the device: the global gradient norm of the last step, before clipping.  Reading it is the caller's sync."""
        return None if self._record is None else ops.optim_record_fields(self._record)['norm']

    @property
    def last_norm_f32(self):
        return None if self._record is None else ops.optim_record_fields(self._record)['norm_f32']

    @property
    def skipped(self):
        """(1,) int64 on the device: the steps skipped for a non-finite gradient."""
        return None if self._counters is None else self._counters[1:2]

    @property
    def steps(self):
        """(1,) int64 on the device: the steps taken (AdamW's ``step``, one for all parameters)."""
        return None if self._counters is None else self._counters[0:1]

    def _moments(self, p):
        """exp_avg / exp_avg_sq of ``p``, zero at first, placed at the parameter's own offset within 16 bytes so that the update's float4
        path serves parameters that are views."""
        st = self.state[p]
        if 'exp_avg' not in st:
            lead = (p.data_ptr() % 16) // 4
            for k in ('exp_avg', 'exp_avg_sq'):
                st[k] = torch.zeros(p.numel() + 3, dtype=torch.float32, device=p.device)[lead:lead + p.numel()].view(p.shape)
        return st['exp_avg'], st['exp_avg_sq']

    # ---------------------------------------------------------------------------------------------------------------------------- step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        rows = []
        for p in group['params']:
            g = p.grad
            if g is None:                                  # torch skips it, weight decay included
                continue
            if g.dtype != torch.float32 or g.device != p.device or g.is_sparse:
                raise ValueError(f'ClippedAdamW: a gradient of {g.dtype} on {g.device} (sparse: {g.is_sparse}) for a float32 GPU parameter')
            if not g.is_contiguous():
                g = g.contiguous()
            m, v = self._moments(p)
            rows.append((p, g, m, v))
        if not rows:
            return loss
        table = self._table.set(rows)
        ops.grad_norm(table, self._record)
        b1, b2 = group['betas']
        ops.adamw_step(table, self._record, self._counters, group['lr'], b1, b2, group['eps'], group['weight_decay'], group['max_norm'],
                       group['skip_nonfinite'])
        for p, _, _, _ in rows:
            _bump(p)
        return loss

    # ------------------------------------------------------------------------------------------------------------------- checkpoints
    def state_dict(self):
        """torch.optim.AdamW's layout.  The shared step counter is read here (a synchronisation) and written per parameter."""
        step = float(self._counters[0].item()) if self._counters is not None else 0.0
        for p in self.param_groups[0]['params']:
            if 'exp_avg' in self.state[p]:
                self.state[p]['step'] = torch.tensor(step, dtype=torch.float32)
        try:
            sd = super().state_dict()
            sd['state'] = {k: dict(v) for k, v in sd['state'].items()}      # (the packed entries ARE self.state's dicts: keep 'step' in the copy only)
        finally:
            for p in self.param_groups[0]['params']:
                self.state[p].pop('step', None)
        sd['skipped'] = int(self._counters[1].item()) if self._counters is not None else 0
        group = sd['param_groups'][0]
        for k, v in dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                         decoupled_weight_decay=True).items():
            group.setdefault(k, v)                         # (what torch.optim.AdamW.load_state_dict reads from a group)
        return sd

    def load_state_dict(self, state_dict):
        """From this class or from torch.optim.AdamW.  The parameters of one checkpoint share their step; one that does not is refused."""
        mine = {k: self.param_groups[0][k] for k in ('max_norm', 'skip_nonfinite')}
        sd = dict(state_dict)
        sd['param_groups'] = [dict(g) for g in state_dict['param_groups']]
        for g in sd['param_groups']:
            for k, v in mine.items():
                g.setdefault(k, v)
        skipped = int(sd.pop('skipped', 0))
        super().load_state_dict(sd)
        steps = set()
        for p in self.param_groups[0]['params']:
            st = self.state[p]
            if 'exp_avg' not in st:
                continue
            steps.add(float(st.pop('step', 0.0)))
            loaded = st.pop('exp_avg'), st.pop('exp_avg_sq')
            for dst, src in zip(self._moments(p), loaded):  # into buffers at the parameter's offset (see _moments)
                dst.copy_(src.to(dst.device, torch.float32).view(dst.shape))
        if len(steps) > 1:
            raise ValueError(f'ClippedAdamW.load_state_dict: the parameters carry different step counts {sorted(steps)}; one counter serves all')
        if self._counters is not None:
            self._counters.copy_(torch.tensor([int(steps.pop()) if steps else 0, skipped], dtype=torch.int64))
        self._table.key = None                             # (the moments moved)
