"""Multi-tensor fused Fromage (``mt_fromage``, ``csrc/multi_tensor.hip``).

Same update as :class:`~imaginaire_amd.optimizers.fromage.Fromage` (which stays the reference
semantics and the ``fused_opt: False`` choice), as one launch sequence per param group: a
per-tensor norm pass with a fixed-order reduce, then one update pass that takes the zero-norm
branch on the device and writes the bf16 spectral-norm shadows (``fused_adam.register_shadow``)
along with the weights. No value is read back to the host, so the step records into a hipGraph;
the learning rate lives in a device tensor that ``sync_hyper`` refreshes between replays.

CPU tensors, ``_ext.force_eager()`` and non-fp32 / non-dense parameters take a
``torch._foreach_*`` path with the Python class's math (bitwise equal to it on the CPU).
"""
import math

import torch
from torch.optim.optimizer import Optimizer, required

from imaginaire_amd.ops import _ext
from imaginaire_amd.optimizers.fused_adam import shadow_of


class DeviceLR(object):
    """The device learning rate of a capturable native step, as ``FusedAdam`` keeps it: every
    group that has taken the native path owns a one-element device tensor ``group['_hyper']``
    which the kernels read instead of their host argument."""

    def _hyper(self, group, device):
        h = group.get('_hyper')
        if h is None or h.device != device:
            h = torch.tensor([float(group['lr'])], dtype=torch.float32, device=device)
            group['_hyper'] = h
            group['_hyper_lr'] = float(group['lr'])
        elif not torch.cuda.is_current_stream_capturing() and \
                group.get('_hyper_lr') != float(group['lr']):
            h.fill_(float(group['lr']))
            group['_hyper_lr'] = float(group['lr'])
        return h

    def sync_hyper(self):
        """Push a changed learning rate (LR scheduler) into the device hyper-parameters.
        Call outside any capture — e.g. before replaying a captured step."""
        for group in self.param_groups:
            h = group.get('_hyper')
            lr = float(group['lr'])
            if h is not None and group.get('_hyper_lr') != lr:
                h.fill_(lr)
                group['_hyper_lr'] = lr

    @staticmethod
    def _strip_hyper(sd):
        for g in sd['param_groups']:
            g.pop('_hyper', None)
            g.pop('_hyper_lr', None)
        return sd

    def _reload_hyper(self, hypers):
        """After ``load_state_dict``: the device tensors refreshed IN PLACE (a captured step
        keeps its pointer)."""
        for g, h in zip(self.param_groups, hypers):
            if h is not None:
                h.fill_(float(g['lr']))
                g['_hyper'] = h
                g['_hyper_lr'] = float(g['lr'])
            else:
                g.pop('_hyper', None)
                g.pop('_hyper_lr', None)


def is_native(params):
    return _ext.use_native(params[0]) and all(
        p.is_cuda and p.dtype == torch.float32 and _ext.is_dense(p) for p in params)


def native_grads(params, grads):
    """Gradients as the kernels take them: one dtype (fp32 or bf16, the first gradient's) and
    walking memory in the order of their parameters (channels-last conv weights); only
    mismatching ones are re-laid out."""
    gdt = grads[0].dtype
    if gdt not in (torch.float32, torch.bfloat16):
        gdt = torch.float32
    return [g if (g.dtype == gdt and g.stride() == p.stride())
            else torch.empty_like(p, dtype=gdt).copy_(g)
            for g, p in zip(grads, params)]


def native_shadows(params):
    sh = [shadow_of(p) for p in params]
    if not any(t is not None for t in sh):
        return []
    none = params[0].new_empty(0, dtype=torch.bfloat16)
    return [t if t is not None else none for t in sh]


class FusedFromage(DeviceLR, Optimizer):
    def __init__(self, params, lr=required, momentum=0):
        defaults = dict(lr=lr, momentum=momentum)
        super().__init__(params, defaults)

    def state_dict(self):
        return self._strip_hyper(super().state_dict())

    def load_state_dict(self, state_dict):
        hypers = [g.get('_hyper') for g in self.param_groups]
        super().load_state_dict(state_dict)
        self._reload_hyper(hypers)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            params = [p for p in group['params'] if p.grad is not None]
            if not params:
                continue
            grads = [p.grad for p in params]
            if any(g.is_sparse for g in grads):
                raise RuntimeError('FusedFromage does not support sparse gradients')
            lr = float(group['lr'])
            if is_native(params):
                hyper = self._hyper(group, params[0].device)
                _ext.ext().mt_fromage(params, native_grads(params, grads),
                                      native_shadows(params), lr, hyper)
            else:
                _foreach_fromage(params, grads, group['lr'])
        return loss


def _foreach_fromage(params, grads, lr):
    """``Fromage.step`` over a list: the same operations on the same values, with the host branch
    on the two norms replaced by a select (``d_p * 1`` is ``d_p``)."""
    ratios = []
    for p, g in zip(params, grads):
        d_p_norm = g.norm()
        p_norm = p.norm()
        ratio = p_norm / d_p_norm
        ratios.append(torch.where((p_norm > 0.0) & (d_p_norm > 0.0), ratio,
                                  torch.ones_like(ratio)))
    upd = torch._foreach_mul(grads, ratios)
    torch._foreach_add_(params, upd, alpha=-lr)
    torch._foreach_mul_(params, 1 / math.sqrt(1 + lr ** 2))
