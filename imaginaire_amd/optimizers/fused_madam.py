"""Multi-tensor fused Madam (``mt_madam``, ``csrc/multi_tensor.hip``).

Same update as :class:`~imaginaire_amd.optimizers.madam.Madam` (which stays the reference
semantics and the ``fused_opt: False`` choice), one launch per param group, with the bf16
spectral-norm shadows written in the same pass.

State. On the native path each parameter owns a two-element fp32 device tensor
``state['_dev'] = [step, max]``: the kernels advance the step themselves (per parameter: one
that had no gradient keeps its own bias correction) and take ``max = scale * sqrt(mean(p²))``
from the parameter before its first update, so no step reads a device value back and a
captured step replays correctly. The device tensor is the truth during training; the host keys
``'step'`` / ``'max'`` are refreshed from it, with one gathered copy, by ``state_dict()``, which
returns the reference layout (``'max'`` a float, ``'step'`` an int, ``'exp_avg_sq'``).
``load_state_dict()`` accepts a ``Madam`` state dict and refreshes existing device tensors in
place, and a state dict written here loads into ``Madam``.

CPU tensors, ``_ext.force_eager()`` and non-fp32 / non-dense parameters take a
``torch._foreach_*`` path with the Python class's math (bitwise equal to it on the CPU).
"""
import torch
from torch.optim.optimizer import Optimizer, required

from imaginaire_amd.ops import _ext
from imaginaire_amd.optimizers.fused_fromage import (DeviceLR, is_native, native_grads,
                                                     native_shadows)


class FusedMadam(DeviceLR, Optimizer):
    def __init__(self, params, lr=required, scale=3.0, g_bound=None, momentum=0):
        self.scale = scale
        self.g_bound = g_bound
        defaults = dict(lr=lr, momentum=momentum)
        super().__init__(params, defaults)

    # -- host <-> device state -------------------------------------------------------------
    def _pull_host(self):
        """'step' / 'max' of every parameter with device state, read back in one copy."""
        sts = [st for st in self.state.values() if '_dev' in st]
        if not sts:
            return
        vals = torch.stack([st['_dev'] for st in sts]).cpu().tolist()
        for st, (step, mx) in zip(sts, vals):
            st['step'] = int(step)
            st['max'] = mx

    def state_dict(self):
        self._pull_host()
        sd = self._strip_hyper(super().state_dict())
        sd['state'] = {k: {n: v for n, v in st.items() if n != '_dev'}
                       for k, st in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict):
        hypers = [g.get('_hyper') for g in self.param_groups]
        old = {p: st for p, st in self.state.items()}
        super().load_state_dict(state_dict)
        self._reload_hyper(hypers)
        for p, st in self.state.items():
            st.pop('_dev', None)
            prev = old.get(p)
            if prev is None or 'step' not in st:
                continue
            # device tensors a captured step may name keep their addresses
            v = prev.get('exp_avg_sq')
            if v is not None and v.shape == st['exp_avg_sq'].shape and \
                    v.device == st['exp_avg_sq'].device and v.dtype == st['exp_avg_sq'].dtype:
                v.copy_(st['exp_avg_sq'])
                st['exp_avg_sq'] = v
            dev = prev.get('_dev')
            if dev is not None:
                dev.copy_(torch.tensor([float(st['step']), float(st['max'])]))
                st['_dev'] = dev

    # -- step ----------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            params = [p for p in group['params'] if p.grad is not None]
            if not params:
                continue
            grads = [p.grad for p in params]
            if any(g.is_sparse for g in grads):
                raise RuntimeError('FusedMadam does not support sparse gradients')
            if is_native(params):
                self._native_step(group, params, grads)
            else:
                self._foreach_step(group, params, grads)
        return loss

    def _native_step(self, group, params, grads):
        X = _ext.ext()
        fresh = []
        for p in params:
            st = self.state[p]
            if '_dev' in st:
                continue
            if 'exp_avg_sq' not in st:
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['_dev'] = torch.zeros(2, dtype=torch.float32, device=p.device)
                fresh.append(p)
            else:  # loaded, or stepped on the other path so far
                st['_dev'] = torch.tensor([float(st['step']), float(st['max'])],
                                          dtype=torch.float32, device=p.device)
        if fresh:
            X.mt_madam_init(fresh, [self.state[p]['_dev'] for p in fresh], float(self.scale))
        hyper = self._hyper(group, params[0].device)
        X.mt_madam(params, native_grads(params, grads),
                   [self.state[p]['exp_avg_sq'] for p in params], native_shadows(params),
                   [self.state[p]['_dev'] for p in params], float(group['lr']),
                   None if self.g_bound is None else float(self.g_bound), hyper)

    def _foreach_step(self, group, params, grads):
        """``Madam.step`` over a list: the same operations on the same values."""
        if any('_dev' in self.state[p] for p in params):
            self._pull_host()
        vs, bcs, maxs = [], [], []
        for p in params:
            st = self.state[p]
            if 'exp_avg_sq' not in st:
                st['max'] = self.scale * (p * p).mean().sqrt().item()
                st['step'] = 0
                st['exp_avg_sq'] = torch.zeros_like(p)
            st['step'] += 1
            bcs.append(1 - 0.999 ** st['step'])
            vs.append(st['exp_avg_sq'])
            maxs.append(st['max'])
        lr = group['lr']
        torch._foreach_mul_(vs, 0.999)
        g2 = torch._foreach_pow(grads, 2)
        torch._foreach_mul_(g2, 0.001)
        torch._foreach_add_(vs, g2)
        den = torch._foreach_div(vs, bcs)
        torch._foreach_sqrt_(den)
        gn = torch._foreach_div(grads, den)
        for t in gn:
            t.masked_fill_(torch.isnan(t), 0)
        if self.g_bound is not None:
            torch._foreach_clamp_min_(gn, -self.g_bound)
            torch._foreach_clamp_max_(gn, self.g_bound)
        torch._foreach_mul_(gn, -lr)
        torch._foreach_mul_(gn, torch._foreach_sign(params))
        torch._foreach_exp_(gn)
        torch._foreach_mul_(params, gn)
        torch._foreach_clamp_min_(params, [-m for m in maxs])
        torch._foreach_clamp_max_(params, maxs)
        for p in params:
            st = self.state[p]
            if '_dev' in st:
                st['_dev'].copy_(torch.tensor([float(st['step']), float(st['max'])]))
