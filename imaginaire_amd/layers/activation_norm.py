"""Activation normalisation layers (reference layers/activation_norm.py:22-432).

Every batch / sync-batch / instance norm here is a fused-norm module: its
``fused(x, gamma, beta, gb, act_slope)`` method runs statistics, affine,
(spatially) adaptive modulation and the following activation in the k1 HIP
kernels. Parameter / buffer names equal PyTorch's BatchNorm / InstanceNorm so
checkpoints match the reference's state dicts.

SPADE MI355X specifics (SpatiallyAdaptiveNorm):
  * with ``separate_projection`` the γ and β convolutions (two MIOpen calls on
    the same hidden map in the reference) are concatenated into ONE conv with
    2C output channels; its NHWC output is consumed directly by the fused
    kernel through strided views, and the backward writes dγ|dβ into one
    buffer (no slicing copies);
  * the nearest-neighbour resize of the label map is cached per resolution
    for the duration of one generator forward (``LabelMapCache``).
"""
import os
from types import SimpleNamespace

import torch

from imaginaire_amd.ops import conv as nhwc_conv
from torch import nn
from torch.nn import functional as F

from imaginaire_amd.ops import _ext
from imaginaire_amd.ops import label as label_ops
from imaginaire_amd.ops.norm import (BiasGradHolder, _NormCfg, defer_sync_bwd, fused_norm_act,
                                     fused_norm_act_pair, prefetch_sync_stats,
                                     spade_pair_enabled, sync_active)
from imaginaire_amd.ops.resize import interpolate
from .conv import LinearBlock, Conv2dBlock, HyperConv2d, PartialConv2dBlock
from .misc import PartialSequential


class _LabelGroup(object):
    """What one forward knows about the SPADE layers that read one resized label map."""
    __slots__ = ('label_map', 'asked', 'ran', 'out')

    def __init__(self, label_map):
        self.label_map = label_map  # (kept alive: the group is keyed by its id)
        self.asked = []             # (SpatiallyAdaptiveNorm, condition index) in call order
        self.ran = False            # the grouped launch of this map was decided (run or not)
        self.out = {}               # (id(module), index) -> hidden map not yet taken


def _label_conv(mod, i):
    """The first conv block of ``mod.mlps[i]`` when it is a plain conv + leaky / relu pair that
    ``ops.conv.conv2d_act`` runs (the label MLP's first layer), else None."""
    from .nonlinearity import act_slope
    from .conv import _fusible_conv
    mlp = mod.mlps[i]
    if mod.partial[i] or len(mlp) != (1 if mod.separate_projection else 2):
        return None
    blk = mlp[0]
    if type(blk) is not Conv2dBlock or list(blk.layers.keys()) != ['conv', 'nonlinearity']:
        return None
    conv = blk.layers['conv']
    if type(conv) is not nn.Conv2d or not _fusible_conv(conv) or conv.groups != 1 or \
            act_slope(blk.layers['nonlinearity']) is None:
        return None
    return blk


def _label_conv_sig(blk):
    """What two label convs must agree in to share a grouped launch."""
    from .nonlinearity import act_slope
    c = blk.layers['conv']
    return (c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, c.dilation,
            c.bias is None, act_slope(blk.layers['nonlinearity']), c.training,
            c.bias.device if c.bias is not None else None)


class LabelMapCache(object):
    """Per-forward cache of resized conditional maps keyed by (id, size), and of the hidden maps
    of the SPADE label MLPs that one grouped conv launch computed for several layers at once
    (``hidden``)."""

    _active = None

    def __init__(self):
        self.store = {}
        self.groups = {}

    def __enter__(self):
        self._prev = LabelMapCache._active
        LabelMapCache._active = self
        return self

    def __exit__(self, *args):
        LabelMapCache._active = self._prev
        self.store = {}
        groups, self.groups = self.groups, {}
        # learn, for the layer that asked first at each map, which layers followed it: the next
        # forward computes their hidden maps together with its own
        for g in groups.values():
            members = []
            for m in g.asked:
                if not any(m[0] is o[0] and m[1] == o[1] for o in members):
                    members.append(m)
            (mod, i), size = members[0], tuple(g.label_map.shape[2:])
            sig = _label_conv_sig(mod.mlps[i][0])
            members = [m for m in members if _label_conv_sig(m[0].mlps[m[1]][0]) == sig]
            mod.__dict__.setdefault('_label_groups', {})[(i, size)] = \
                members if len(members) >= 2 else None

    class suspended(object):
        """Context in which no cache is active (a checkpointed block: its recompute runs outside
        the generator's cache, so its first pass must not take part in a grouped launch)."""

        def __enter__(self):
            self._prev = LabelMapCache._active
            LabelMapCache._active = None

        def __exit__(self, *args):
            LabelMapCache._active = self._prev

    def hidden(self, mod, i, label_map):
        """``mod.mlps[i][0](label_map)``. The first layer to ask at a map whose followers are
        known from an earlier forward computes all their hidden maps in one grouped conv
        (ops/conv.py ``conv2d_act_group``); the followers take theirs from here."""
        from .conv import _plain_conv_weight
        blk = mod.mlps[i][0]
        g = self.groups.get(id(label_map))
        if g is None:
            g = self.groups[id(label_map)] = _LabelGroup(label_map)
        g.asked.append((mod, i))
        out = g.out.pop((id(mod), i), None)
        if out is not None:
            return out
        members = None
        if not g.ran:
            g.ran = True
            members = mod.__dict__.get('_label_groups', {}).get(
                (i, tuple(label_map.shape[2:])))
        if members and nhwc_conv.spade_group_enabled():
            # verify what was learned: the same first layer, every member still a label conv
            # that agrees with it
            blks = [_label_conv(m, j) for m, j in members]
            if members[0][0] is mod and members[0][1] == i and all(
                    b is not None and _label_conv_sig(b) == _label_conv_sig(blk) for b in blks):
                convs = [b.layers['conv'] for b in blks]
                c0 = convs[0]
                ys = nhwc_conv.conv2d_act_group(
                    label_map, [_plain_conv_weight(c) for c in convs], [c.bias for c in convs],
                    c0.stride, c0.padding, c0.dilation, _label_conv_sig(blk)[7])
                for (m, j), y in zip(members[1:], ys[1:]):
                    g.out[(id(m), j)] = y
                return ys[0]
        return blk(label_map)

    @staticmethod
    def resize(t, size, mode='nearest', conv_pad=False):
        """Resized conditional map, memoised per forward. ``conv_pad``: the consumer is a
        conv block — a CUDA NHWC map with an odd channel count (185-channel COCO-Stuff
        labels) is returned zero-padded to the conv kernels' channel granularity and marked
        (ops.conv.mark_zero_tail), so the padding happens once per resolution per forward
        instead of inside every SPADE layer's MLP conv."""
        cache = LabelMapCache._active
        same = tuple(t.shape[2:]) == tuple(size) and mode == 'nearest'
        pad = conv_pad and t.is_cuda and t.dim() == 4 and t.shape[1] > 64 and \
            t.shape[1] % 64 != 0
        if same and not pad:
            return t
        key = (id(t), t.data_ptr(), tuple(size), mode, pad)
        out = cache.store.get(key) if cache is not None else None
        packed = getattr(t, '_iamd_packed_label', None)
        if out is None and packed is not None and mode == 'nearest' and t.dim() == 4 and \
                _ext.use_native(t) and t.dtype in (torch.float32, torch.bfloat16) and \
                label_ops.packed_resize_enabled() and _ext.is_dense(t):
            # an expanded packed label: its resized (and padded) map is a function of the index
            # planes, written by one k19 launch instead of a padded full-resolution copy plus a
            # resize of that copy. Same values, dtype, layout and mark as the path below.
            c = t.shape[1]
            cl = t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()
            out = label_ops.expand_labels(
                packed.idx, packed.dense, packed.layout, size=tuple(size),
                pad_to=(c + 63) // 64 * 64 if pad else None, dtype=t.dtype,
                channels_last=pad or cl)
            if pad:
                out = nhwc_conv.mark_zero_tail(out, c)
            if cache is not None:
                cache.store[key] = out
        if out is None:
            src = t
            if pad:
                # pad ONCE at the source resolution (cached), then resize the padded map: the
                # zero tail stays zero and the NHWC resize kernels need channels % 8 == 0
                pkey = (id(t), t.data_ptr(), 'padded')
                src = cache.store.get(pkey) if cache is not None else None
                if src is None:
                    c = t.shape[1]
                    src = nhwc_conv.mark_zero_tail(
                        nhwc_conv._pad_channels(t, (c + 63) // 64 * 64), c)
                    if cache is not None:
                        cache.store[pkey] = src
            out = src if same else interpolate(src, size=size, mode=mode)
            if cache is not None:
                cache.store[key] = out
        return out


class _FusedNormBase(nn.Module):
    """Shared machinery of the fused batch / instance norms."""

    supports_fused_act = True
    mode = 'batch'

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True,
                 track_running_stats=True):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.affine = affine
        self.track_running_stats = track_running_stats
        if affine:
            self.weight = nn.Parameter(torch.ones(num_features))
            self.bias = nn.Parameter(torch.zeros(num_features))
        else:
            self.register_parameter('weight', None)
            self.register_parameter('bias', None)
        if track_running_stats:
            self.register_buffer('running_mean', torch.zeros(num_features))
            self.register_buffer('running_var', torch.ones(num_features))
            self.register_buffer('num_batches_tracked', torch.tensor(0, dtype=torch.long))
        else:
            self.register_buffer('running_mean', None)
            self.register_buffer('running_var', None)
            self.register_buffer('num_batches_tracked', None)
        self.process_group = None

    def reset_running_stats(self):
        if self.track_running_stats:
            self.running_mean.zero_()
            self.running_var.fill_(1)
            self.num_batches_tracked.zero_()

    def reset_parameters(self):
        self.reset_running_stats()
        if self.affine:
            nn.init.ones_(self.weight)
            nn.init.zeros_(self.bias)

    def _factor(self, defer_count=False):
        """Running-average factor of this call. With ``defer_count`` (and a fixed momentum)
        ``num_batches_tracked`` is NOT incremented here: the caller hands it to
        :func:`fused_norm_act`, whose statistics kernel increments it."""
        if not (self.training and self.track_running_stats):
            return 0.0
        if defer_count and self.momentum is not None:
            return self.momentum
        self.num_batches_tracked.add_(1)
        if self.momentum is None:
            return 1.0 / float(self.num_batches_tracked.item())
        return self.momentum

    def _deferred_count(self, use_batch):
        return self.num_batches_tracked if (
            use_batch and self.training and self.track_running_stats and
            self.momentum is not None) else None

    def _effective_mode(self):
        return self.mode

    def fused(self, x, gamma=None, beta=None, gb=None, act_slope=1.0, deferred=None,
              bias_grad=None):
        squeeze = None
        if x.dim() == 2:
            squeeze = x.shape
            x = x[:, :, None, None]
        elif x.dim() == 3:
            squeeze = x.shape
            x = x[:, :, :, None]
        elif x.dim() == 5:
            return self._fallback_nd(x, gamma, beta, act_slope)
        use_batch = self.training or not self.track_running_stats or \
            self._effective_mode() == 'instance'
        y = fused_norm_act(
            x, self._effective_mode(), self.weight, self.bias, gamma=gamma, beta=beta, gb=gb,
            running_mean=self.running_mean if self.track_running_stats else None,
            running_var=self.running_var if self.track_running_stats else None,
            training=use_batch, momentum=self._factor(True) if use_batch else 0.0, eps=self.eps,
            slope=act_slope, process_group=self.process_group, deferred=deferred,
            num_batches=self._deferred_count(use_batch), bias_grad=bias_grad)
        if squeeze is not None:
            y = y.reshape(squeeze)
        return y

    def _fallback_nd(self, x, gamma, beta, act_slope):
        if self._effective_mode() == 'instance':
            y = F.instance_norm(x, weight=self.weight, bias=self.bias, eps=self.eps)
        else:
            y = F.batch_norm(x, self.running_mean, self.running_var, self.weight, self.bias,
                             self.training or not self.track_running_stats,
                             self.momentum or 0.1, self.eps)
        if gamma is not None:
            y = y * (1 + gamma) + beta
        if act_slope != 1.0:
            y = F.leaky_relu(y, act_slope) if act_slope > 0 else F.relu(y)
        return y

    def forward(self, x, act_slope=1.0):
        return self.fused(x, act_slope=act_slope)

    def extra_repr(self):
        return '{num_features}, eps={eps}, momentum={momentum}, affine={affine}, ' \
               'track_running_stats={track_running_stats}'.format(**self.__dict__)


class BatchNorm2d(_FusedNormBase):
    """BatchNorm (1d/2d inputs) running on the fused HIP kernels."""
    mode = 'batch'


class SyncBatchNorm(_FusedNormBase):
    """Cross-replica BatchNorm: one all-gather (fwd) / all-reduce (bwd) per layer."""
    mode = 'sync_batch'

    def _effective_mode(self):
        from imaginaire_amd.ops.norm import sync_active
        if self.training and sync_active(self.process_group):
            return 'sync_batch'
        return 'batch'


class InstanceNorm2d(_FusedNormBase):
    """InstanceNorm (PyTorch defaults: no running stats)."""
    mode = 'instance'

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=False,
                 track_running_stats=False):
        super().__init__(num_features, eps, momentum, affine, track_running_stats)


def fused_norm_or_none(norm, x, gamma=None, beta=None, gb=None, act_slope=1.0, deferred=None,
                       bias_grad=None):
    """Apply ``norm`` (fused module, torch module or None) + modulation + activation.
    ``bias_grad``: the :class:`BiasGradHolder` shared with the conv that produced ``gb``."""
    if norm is None:
        return fused_norm_act(x, 'none', gamma=gamma, beta=beta, gb=gb, slope=act_slope,
                              bias_grad=bias_grad)
    if isinstance(norm, _FusedNormBase):
        return norm.fused(x, gamma=gamma, beta=beta, gb=gb, act_slope=act_slope,
                          deferred=deferred, bias_grad=bias_grad)
    y = norm(x)
    if gb is not None:
        gamma, beta = gb.chunk(2, dim=1)
    if gamma is not None:
        if gamma.dim() == 2:
            gamma, beta = gamma[:, :, None, None], beta[:, :, None, None]
        y = y * (1 + gamma) + beta
    if act_slope != 1.0:
        y = F.leaky_relu(y, act_slope) if act_slope > 0 else F.relu(y)
    return y


def _modulate_more(out, gbs, act_slope):
    """Further SPADE modulations ``out·(1+γ_i) + β_i`` (multi-condition SPADE: label map +
    warped image / flow mask in vid2vid / fs-vid2vid), the last one followed by the activation:
    each is one pass of the k1 kernel in 'none' (identity-normalisation) mode, forward and
    backward, with γ|β read straight from the fused γ|β conv output — instead of separate
    add / mul / add / leaky-relu passes and their backward, plus two slice-gradient scatters."""
    if _MULTIMOD_FUSED:
        for i, gb in enumerate(gbs):
            out = fused_norm_act(out, 'none', gb=gb,
                                 slope=act_slope if i == len(gbs) - 1 else 1.0)
        return out
    for gb in gbs:  # A/B reference path (IMAGINAIRE_AMD_SPADE_MULTIMOD=0)
        g, b = gb.chunk(2, dim=1)
        out = out * (1 + g) + b
    if act_slope != 1.0:
        out = F.leaky_relu(out, act_slope) if act_slope > 0 else F.relu(out)
    return out


_MULTIMOD_FUSED = os.environ.get('IMAGINAIRE_AMD_SPADE_MULTIMOD', '1') == '1'
# sync-BN data gradient finished by a join node after the γ|β backward (0: synchronous)
_ASYNC_SYNCBN_BWD = os.environ.get('IMAGINAIRE_AMD_ASYNC_SYNCBN_BWD', '1') == '1'


class AdaptiveNorm(nn.Module):
    """AdaIN / conditional BN: ``norm(x)·(1+γ(y)) + β(y)`` (activation_norm.py:22-106)."""

    supports_fused_act = True

    def __init__(self, num_features, cond_dims, weight_norm_type='', projection=True,
                 separate_projection=False, input_dim=2, activation_norm_type='instance',
                 activation_norm_params=None):
        super().__init__()
        self.projection = projection
        self.separate_projection = separate_projection
        if activation_norm_params is None:
            activation_norm_params = SimpleNamespace(affine=False)
        self.norm = get_activation_norm_layer(num_features, activation_norm_type, input_dim,
                                              **vars(activation_norm_params))
        if self.projection:
            if self.separate_projection:
                self.fc_gamma = LinearBlock(cond_dims, num_features,
                                            weight_norm_type=weight_norm_type)
                self.fc_beta = LinearBlock(cond_dims, num_features,
                                           weight_norm_type=weight_norm_type)
            else:
                self.fc = LinearBlock(cond_dims, num_features * 2,
                                      weight_norm_type=weight_norm_type)
        self.conditional = True

    def forward(self, x, y, act_slope=1.0, **kwargs):
        if self.projection:
            if self.separate_projection:
                gamma = self.fc_gamma(y)
                beta = self.fc_beta(y)
            else:
                gamma, beta = self.fc(y).chunk(2, 1)
        else:
            gamma, beta = y.chunk(2, 1)
        if x.dim() == 4 and gamma.dim() == 2:
            return fused_norm_or_none(self.norm, x, gamma=gamma.contiguous(),
                                      beta=beta.contiguous(), act_slope=act_slope)
        for _ in range(x.dim() - gamma.dim()):
            gamma = gamma.unsqueeze(-1)
            beta = beta.unsqueeze(-1)
        out = self.norm(x) if self.norm is not None else x
        out = out * (1 + gamma) + beta
        if act_slope != 1.0:
            out = F.leaky_relu(out, act_slope) if act_slope > 0 else F.relu(out)
        return out


class _Cat0View(torch.autograd.Function):
    """``cat([a, b], 0)`` of two channels-last tensors that already sit back to back in one
    storage (the γ and β conv weights of a SPADE layer written consecutively into the k5c
    spectral-norm buffer): a view, no copy; the backward splits the gradient."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.n = a.shape[0]
        shape = (a.shape[0] + b.shape[0],) + tuple(a.shape[1:])
        return a.as_strided(shape, a.stride(), a.storage_offset())

    @staticmethod
    def backward(ctx, g):
        return g[:ctx.n], g[ctx.n:]


def cat0(a, b):
    cl = torch.channels_last
    if a.is_cuda and a.dim() == 4 and b.dim() == 4 and a.dtype == b.dtype and \
            a.shape[1:] == b.shape[1:] and a.stride() == b.stride() and \
            a.is_contiguous(memory_format=cl) and b.is_contiguous(memory_format=cl) and \
            a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and \
            b.storage_offset() == a.storage_offset() + a.numel():
        return _Cat0View.apply(a, b)
    return torch.cat([a, b], 0)


class SpatiallyAdaptiveNorm(nn.Module):
    """SPADE (activation_norm.py:109-234), fused on MI355X (see module docstring)."""

    supports_fused_act = True

    def __init__(self, num_features, cond_dims, num_filters=128, kernel_size=3,
                 weight_norm_type='', separate_projection=False,
                 activation_norm_type='sync_batch', activation_norm_params=None, partial=False):
        super().__init__()
        if activation_norm_params is None:
            activation_norm_params = SimpleNamespace(affine=False)
        padding = kernel_size // 2
        self.separate_projection = separate_projection
        self.mlps = nn.ModuleList()
        self.gammas = nn.ModuleList()
        self.betas = nn.ModuleList()
        self.num_features = num_features
        if type(cond_dims) != list:
            cond_dims = [cond_dims]
        if not isinstance(num_filters, list):
            num_filters = [num_filters] * len(cond_dims)
        if not isinstance(partial, list):
            partial = [partial] * len(cond_dims)
        self.partial = partial
        for i, cond_dim in enumerate(cond_dims):
            mlp = []
            conv_block = PartialConv2dBlock if partial[i] else Conv2dBlock
            sequential = PartialSequential if partial[i] else nn.Sequential
            if num_filters[i] > 0:
                mlp += [conv_block(cond_dim, num_filters[i], kernel_size, padding=padding,
                                   weight_norm_type=weight_norm_type, nonlinearity='relu')]
            mlp_ch = cond_dim if num_filters[i] == 0 else num_filters[i]
            if self.separate_projection:
                if partial[i]:
                    raise NotImplementedError(
                        'Separate projection not yet implemented for partial conv')
                self.mlps.append(nn.Sequential(*mlp))
                self.gammas.append(conv_block(mlp_ch, num_features, kernel_size, padding=padding,
                                              weight_norm_type=weight_norm_type))
                self.betas.append(conv_block(mlp_ch, num_features, kernel_size, padding=padding,
                                             weight_norm_type=weight_norm_type))
                # γ and β run as ONE conv over their concatenated weights (_gb): their spectral
                # norm group materialises bf16(W / sigma) for them back to back (zero-copy cat)
                for blk in (self.gammas[-1], self.betas[-1]):
                    blk.layers.conv._iamd_sn_materialize = True
            else:
                mlp += [conv_block(mlp_ch, num_features * 2, kernel_size, padding=padding,
                                   weight_norm_type=weight_norm_type)]
                self.mlps.append(sequential(*mlp))
        self.norm = get_activation_norm_layer(num_features, activation_norm_type, 2,
                                              **vars(activation_norm_params))
        self.conditional = True
        # (condition index, map size) -> the [(norm, index)] whose label MLPs read the map this
        # layer is the first to ask for, learned by LabelMapCache from the previous forward
        self._label_groups = {}

    def _hidden(self, i, label_map):
        """The label MLP's hidden map ``mlps[i][0](label_map)``: inside an active
        :class:`LabelMapCache` the layers of one resolution compute theirs in one grouped conv
        launch (``IMAGINAIRE_AMD_SPADE_GROUP=0``: each its own)."""
        cache = LabelMapCache._active
        if cache is None or not nhwc_conv.spade_group_enabled() or \
                _label_conv(self, i) is None:
            return self.mlps[i][0](label_map)
        return cache.hidden(self, i, label_map)

    def _gb(self, i, label_map, bias_grad=None):
        """γ|β for condition i as one [N, 2C, H, W] tensor (first C = γ). ``bias_grad``: the
        holder in which the norm's backward leaves the γ|β conv's bias gradient."""
        if self.separate_projection:
            from .weight_norm import get_weight
            hidden = self._hidden(i, label_map) if len(self.mlps[i]) == 1 else \
                self.mlps[i](label_map)
            cg = self.gammas[i].layers.conv
            cb = self.betas[i].layers.conv
            w = cat0(get_weight(cg), get_weight(cb))
            b = torch.cat([cg.bias, cb.bias], 0) if cg.bias is not None else None
            return nhwc_conv.conv2d(hidden, w, b, cg.stride, cg.padding, cg.dilation, cg.groups,
                                    cg.padding_mode, bias_grad=bias_grad if b is not None else None)
        if len(self.mlps[i]) == 2 and not self.partial[i]:
            return self.mlps[i][1](self._hidden(i, label_map))
        return self.mlps[i](label_map)

    def forward(self, x, *cond_inputs, act_slope=1.0, **kwargs):
        active = [i for i in range(len(cond_inputs)) if cond_inputs[i] is not None]
        size = x.shape[2:]
        deferred = None
        if isinstance(self.norm, SyncBatchNorm) and self.training and \
                self.norm._effective_mode() == 'sync_batch':
            if not self.norm.affine:
                # start the cross-rank statistics exchange of x now: it rides xGMI while the
                # γ|β convolutions below (independent of it) run
                prefetch_sync_stats(x, self.norm.eps, self.norm.process_group)
            if _ASYNC_SYNCBN_BWD and active:
                # backward mirror: the norm's Σg, Σg·x̂ all-reduce runs while the γ|β / mlp
                # convolution backward runs; this join node (created before them) finishes dx
                x, deferred = defer_sync_bwd(x)
        # the first condition's γ|β goes to the norm alone: its backward sums dγ|dβ per channel
        # for the γ|β conv's bias gradient while it writes them (no second pass over the map)
        holder = BiasGradHolder() if active and self.separate_projection else None
        gbs = []
        for i in active:
            label_map = LabelMapCache.resize(cond_inputs[i], size,
                                             conv_pad=not self.partial[i])
            gbs.append(self._gb(i, label_map, holder if i == active[0] else None))
        if len(gbs) == 0:
            return fused_norm_or_none(self.norm, x, act_slope=act_slope)
        if len(gbs) == 1:
            return fused_norm_or_none(self.norm, x, gb=gbs[0], act_slope=act_slope,
                                      deferred=deferred, bias_grad=holder)
        return _modulate_more(fused_norm_or_none(self.norm, x, gb=gbs[0], act_slope=1.0,
                                                 deferred=deferred, bias_grad=holder),
                              gbs[1:], act_slope)


    def pair_applies(self, other, x_low, cond_inputs):
        """``self`` and ``other`` can normalise the nearest upsampling of ``x_low`` as a pair
        (:meth:`forward_pair`): two SPADE layers with one active, non-partial condition over
        the same kind of batch norm (param-free or with its per-channel affine; same eps and
        momentum, no cross-rank exchange active), on a packed channels-last GPU tensor with
        C % 8 == 0. This decides for the modules; what the kernels themselves need of the
        tensors (ops/norm.py ``pair_native_ok``, which sees the γ|β maps as well) is checked
        again there and falls back to upsample + two norms by itself."""
        if not (spade_pair_enabled() and type(other) is SpatiallyAdaptiveNorm and
                type(self) is SpatiallyAdaptiveNorm):
            return False
        active = [i for i in range(len(cond_inputs)) if cond_inputs[i] is not None]
        if len(active) != 1 or active[0] >= len(self.mlps) or active[0] >= len(other.mlps) or \
                self.partial[active[0]] or other.partial[active[0]] or \
                self.num_features != other.num_features:
            return False
        a, b = self.norm, other.norm
        if not (isinstance(a, _FusedNormBase) and type(a) is type(b) and
                type(a) in (BatchNorm2d, SyncBatchNorm) and a.affine == b.affine and
                a.eps == b.eps and a.momentum == b.momentum and a.momentum is not None and
                a.track_running_stats == b.track_running_stats and a.training == b.training and
                a.process_group is b.process_group and a._effective_mode() == 'batch' and
                not sync_active(a.process_group)):
            return False
        return torch.is_tensor(x_low) and x_low.dim() == 4 and _ext.use_native(x_low) and \
            x_low.dtype in (torch.bfloat16, torch.float32) and x_low.shape[1] % 8 == 0 and \
            x_low.shape[1] == self.num_features and x_low.numel() > 0 and \
            x_low.is_contiguous(memory_format=torch.channels_last)

    def forward_pair(self, other, x_low, up, *cond_inputs, act_slopes=(1.0, 1.0)):
        """``(self(x), other(x))`` for ``x`` the nearest upsampling of ``x_low`` by ``up``, which
        is never materialised (ops/norm.py ``fused_norm_act_pair``). The caller checked
        :meth:`pair_applies`. Both γ|β maps are computed at the upsampled size, in the order
        the two layers would ask for them. Neither layer's ``forward`` nor its norm module is
        called, so forward hooks registered on them do not fire on this path
        (``IMAGINAIRE_AMD_SPADE_PAIR=0`` when they must)."""
        i = [k for k in range(len(cond_inputs)) if cond_inputs[k] is not None][0]
        size = (x_low.shape[2] * up, x_low.shape[3] * up)
        gbs, holders, running, affines = [], [], [], []
        norm = self.norm
        use_batch = norm.training or not norm.track_running_stats
        for layer in (self, other):
            label_map = LabelMapCache.resize(cond_inputs[i], size, conv_pad=True)
            holders.append(BiasGradHolder() if layer.separate_projection else None)
            gbs.append(layer._gb(i, label_map, holders[-1]))
            n = layer.norm
            running.append((n.running_mean if n.track_running_stats else None,
                            n.running_var if n.track_running_stats else None,
                            n._deferred_count(use_batch)))
            affines.append((n.weight, n.bias))
        cfg = _NormCfg('batch', use_batch, norm._factor(True) if use_batch else 0.0, norm.eps,
                       1.0, norm.process_group)
        return fused_norm_act_pair(x_low, up, gbs[0], gbs[1], act_slopes, cfg, holders, running,
                                   affines)


class HyperSpatiallyAdaptiveNorm(nn.Module):
    """SPADE whose first MLP's weights are supplied at run time (activation_norm.py:237-326)."""

    supports_fused_act = True

    def __init__(self, num_features, cond_dims, num_filters=0, kernel_size=3,
                 weight_norm_type='', activation_norm_type='sync_batch', is_hyper=True):
        super().__init__()
        padding = kernel_size // 2
        self.mlps = nn.ModuleList()
        if type(cond_dims) != list:
            cond_dims = [cond_dims]
        for i, cond_dim in enumerate(cond_dims):
            mlp = []
            if not is_hyper or (i != 0):
                if num_filters > 0:
                    mlp += [Conv2dBlock(cond_dim, num_filters, kernel_size, padding=padding,
                                        weight_norm_type=weight_norm_type, nonlinearity='relu')]
                mlp_ch = cond_dim if num_filters == 0 else num_filters
                mlp += [Conv2dBlock(mlp_ch, num_features * 2, kernel_size, padding=padding,
                                    weight_norm_type=weight_norm_type)]
                mlp = nn.Sequential(*mlp)
            else:
                if num_filters > 0:
                    raise ValueError('Multi hyper layer not supported yet.')
                mlp = HyperConv2d(padding=padding)
            self.mlps.append(mlp)
        self.norm = get_activation_norm_layer(num_features, activation_norm_type, 2, affine=False)
        self.num_features = num_features
        self.conditional = True

    def forward(self, x, *cond_inputs, norm_weights=(None, None), act_slope=1.0, **kwargs):
        deferred = None
        if isinstance(self.norm, SyncBatchNorm) and self.training and _ASYNC_SYNCBN_BWD and \
                self.norm._effective_mode() == 'sync_batch' and \
                any(c is not None for c in cond_inputs):
            x, deferred = defer_sync_bwd(x)  # see SpatiallyAdaptiveNorm.forward
        gbs = []
        for i in range(len(cond_inputs)):
            if cond_inputs[i] is None:
                continue
            if type(cond_inputs[i]) == list:
                cond_input, mask = cond_inputs[i]
                mask = interpolate(mask, size=x.size()[2:], mode='bilinear',
                                     align_corners=False)
            else:
                cond_input = cond_inputs[i]
                mask = None
            label_map = LabelMapCache.resize(cond_input, x.size()[2:])
            if norm_weights is None or norm_weights[0] is None or i != 0:
                gb = self.mlps[i](label_map)
            else:
                gb = self.mlps[i](label_map, conv_weights=norm_weights)
            if mask is not None:
                # the mask (fp32 from the flow branch) must not promote the 2C-channel
                # modulation maps (and everything after them) to fp32
                gb = gb * (1 - mask.to(gb.dtype))
            gbs.append(gb)
        if len(gbs) == 0:
            return fused_norm_or_none(self.norm, x, act_slope=act_slope)
        if len(gbs) == 1:
            return fused_norm_or_none(self.norm, x, gb=gbs[0], act_slope=act_slope,
                                      deferred=deferred)
        return _modulate_more(fused_norm_or_none(self.norm, x, gb=gbs[0], act_slope=1.0,
                                                 deferred=deferred),
                              gbs[1:], act_slope)


class LayerNorm2d(nn.Module):
    """Per-sample mean/std normalisation over (C, H, W) (activation_norm.py:329-374)."""

    def __init__(self, num_features, eps=1e-5, affine=True):
        super().__init__()
        self.num_features = num_features
        self.affine = affine
        self.eps = eps
        if self.affine:
            self.gamma = nn.Parameter(torch.Tensor(num_features).uniform_())
            self.beta = nn.Parameter(torch.zeros(num_features))

    def forward(self, x):
        shape = [-1] + [1] * (x.dim() - 1)
        if x.size(0) == 1:
            mean = x.reshape(-1).mean().view(*shape)
            std = x.reshape(-1).std().view(*shape)
        else:
            mean = x.reshape(x.size(0), -1).mean(1).view(*shape)
            std = x.reshape(x.size(0), -1).std(1).view(*shape)
        x = (x - mean) / (std + self.eps)
        if self.affine:
            shape = [1, -1] + [1] * (x.dim() - 2)
            x = x * self.gamma.view(*shape) + self.beta.view(*shape)
        return x


def get_activation_norm_layer(num_features, norm_type, input_dim, **norm_params):
    """Activation-norm factory (activation_norm.py:377-432)."""
    input_dim = max(input_dim, 1)
    if norm_type == 'none' or norm_type == '':
        return None
    if norm_type == 'batch':
        if input_dim == 3:
            return nn.BatchNorm3d(num_features, **norm_params)
        return BatchNorm2d(num_features, **norm_params)
    if norm_type == 'instance':
        affine = norm_params.pop('affine', True)
        if input_dim == 3:
            return nn.InstanceNorm3d(num_features, affine=affine, **norm_params)
        return InstanceNorm2d(num_features, affine=affine, **norm_params)
    if norm_type == 'sync_batch':
        affine = norm_params.pop('affine', True)
        layer = SyncBatchNorm(num_features, affine=True, **norm_params)
        layer.weight.requires_grad = affine
        layer.bias.requires_grad = affine
        return layer
    if norm_type == 'layer':
        return nn.LayerNorm(num_features, **norm_params)
    if norm_type == 'layer_2d':
        return LayerNorm2d(num_features, **norm_params)
    if norm_type == 'group':
        return nn.GroupNorm(num_channels=num_features, **norm_params)
    if norm_type == 'adaptive':
        return AdaptiveNorm(num_features, **norm_params)
    if norm_type == 'spatially_adaptive':
        if input_dim != 2:
            raise ValueError('Spatially adaptive normalization layers only supports 2D input')
        return SpatiallyAdaptiveNorm(num_features, **norm_params)
    if norm_type == 'hyper_spatially_adaptive':
        if input_dim != 2:
            raise ValueError('Spatially adaptive normalization layers only supports 2D input')
        return HyperSpatiallyAdaptiveNorm(num_features, **norm_params)
    raise ValueError('Activation norm layer %s is not recognized' % norm_type)
