"""Packed label maps -> the label tensor the networks read (k19, ``csrc/label.hip``).

A dataset with ``data.packed_labels`` keeps every label type that ``make_one_hot`` would expand
as ONE index plane per pixel (``label_idx``: uint8, or int16 above 255 classes; value ``n`` =
don't care / out of range) and only the remaining types (edge maps, instance maps, ...) as fp32
channels (``label_dense``). One byte per pixel instead of ``n`` floats crosses the loader
workers' shared memory, the pinned copy and PCIe; :func:`expand_labels` turns the pair back into
exactly the tensor the unpacked path delivers, on the device, in one launch that also applies a
nearest resize and the conv kernels' zero channel padding when asked (what
``layers.activation_norm.LabelMapCache.resize`` needs per SPADE resolution).

The *layout* is the ordered list of segments
``(name, kind, out_channels, num_labels, use_dont_care)`` a dataset's ``get_label_layout()``
returns, ``kind`` being ``'index'`` (one index plane -> ``out_channels`` one-hot channels, the
last of them the don't-care channel when ``use_dont_care``) or ``'dense'`` (``out_channels``
channels copied).

GPU tensors run the HIP kernel; CPU tensors and ``_ext.force_eager()`` run the PyTorch reference
below (scatter, cat, nearest interpolate, zero pad), which is also the oracle of the kernel: the
outputs are zeros, ones and copied values, so the two agree bit for bit.
"""
import os

import torch
import torch.nn.functional as F

from imaginaire_amd.ops import _ext
from imaginaire_amd.ops.resize import _pair, _src_scale

INDEX, DENSE = 'index', 'dense'
MAX_SEGMENTS = 16


def index_dtype(layout):
    """dtype of a layout's index planes: uint8 while every index (0 .. num_labels) fits."""
    ns = [seg[3] for seg in layout if seg[1] == INDEX]
    return torch.int16 if ns and max(ns) > 255 else torch.uint8


def layout_channels(layout):
    return sum(seg[2] for seg in layout)


def packed_resize_enabled():
    """``IMAGINAIRE_AMD_LABEL_PACKED_RESIZE`` (read per call; 0: ``LabelMapCache.resize`` pads
    and resizes the expanded label as it does for any tensor, the A/B switch)."""
    return os.environ.get('IMAGINAIRE_AMD_LABEL_PACKED_RESIZE', '1') != '0'


class PackedSource(object):
    """What an expanded label remembers of where it came from (``t._iamd_packed_label``)."""
    __slots__ = ('idx', 'dense', 'layout')

    def __init__(self, idx, dense, layout):
        self.idx, self.dense, self.layout = idx, dense, layout


def _check(idx, dense, layout):
    layout = [tuple(seg) for seg in layout]
    if not 1 <= len(layout) <= MAX_SEGMENTS:
        raise ValueError('expand_labels: 1 .. %d layout segments expected, got %d' %
                         (MAX_SEGMENTS, len(layout)))
    k = d = 0
    for name, kind, out_ch, n, udc in layout:
        if kind == INDEX:
            if out_ch != n + (1 if udc else 0) or n < 1:
                raise ValueError('expand_labels: segment %r: %d channels for %d labels' %
                                 (name, out_ch, n))
            k += 1
        elif kind == DENSE:
            if out_ch < 1:
                raise ValueError('expand_labels: segment %r has no channels' % (name,))
            d += out_ch
        else:
            raise ValueError('expand_labels: unknown segment kind %r' % (kind,))
    for t, want, what in ((idx, k, 'idx'), (dense, d, 'dense')):
        if want == 0:
            continue
        if t is None or t.dim() not in (4, 5) or t.shape[-3] != want:
            raise ValueError('expand_labels: %s must be [B, (T,) %d, H, W], got %s' % (
                what, want, None if t is None else tuple(t.shape)))
        if t.requires_grad:
            raise RuntimeError('expand_labels is not differentiable: labels carry no gradient '
                               '(%s requires grad)' % what)
    if k and idx.dtype not in (torch.uint8, torch.int16):
        raise TypeError('expand_labels: idx must be uint8 or int16, got %s' % idx.dtype)
    if d and dense.dtype != torch.float32:
        raise TypeError('expand_labels: dense must be float32, got %s' % dense.dtype)
    if k and d and (idx.shape[:-3] != dense.shape[:-3] or idx.shape[-2:] != dense.shape[-2:] or
                    idx.device != dense.device):
        raise ValueError('expand_labels: idx %s and dense %s do not match' % (
            tuple(idx.shape), tuple(dense.shape)))
    return layout, (idx if k else None), (dense if d else None)


def expand_labels_reference(idx, dense, layout, *, size=None, pad_to=None, dtype=torch.float32,
                            channels_last=False):
    """PyTorch form of :func:`expand_labels` on 4-D inputs (the oracle)."""
    parts, k, d = [], 0, 0
    for _, kind, out_ch, n, udc in layout:
        if kind == INDEX:
            plane = idx[:, k:k + 1].long()
            hot = torch.zeros((plane.shape[0], n + 1) + tuple(plane.shape[2:]),
                              device=plane.device)
            hot.scatter_(1, plane, 1.0)
            parts.append(hot if udc else hot[:, :n])
            k += 1
        else:
            parts.append(dense[:, d:d + out_ch])
            d += out_ch
    x = torch.cat(parts, 1)
    if size is not None:
        x = F.interpolate(x, size=tuple(size), mode='nearest')
    if pad_to is not None and pad_to > x.shape[1]:
        x = torch.cat([x, x.new_zeros((x.shape[0], pad_to - x.shape[1]) + tuple(x.shape[2:]))], 1)
    x = x.to(dtype)
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()


def expand_labels(idx, dense, layout, *, size=None, pad_to=None, dtype=torch.float32,
                  channels_last=False):
    """``[B, C (+ pad), Ho, Wo]`` (or ``[B, T, C (+ pad), Ho, Wo]`` for 5-D inputs) label tensor
    of ``dtype`` (fp32 / bf16) from the index planes ``idx [B, (T,) K, H, W]`` and the dense
    channels ``dense [B, (T,) Cd, H, W]`` (either ``None`` when the layout has no such segment).

    ``size``: nearest resize to ``(Ho, Wo)``, equal to ``F.interpolate(expanded, size)``;
    ``pad_to``: zero channels up to that count; ``channels_last``: packed NHWC output (4-D
    only). Not differentiable."""
    layout, idx, dense = _check(idx, dense, layout)
    ref = idx if idx is not None else dense
    c = layout_channels(layout)
    if pad_to is not None and pad_to < c:
        raise ValueError('expand_labels: pad_to %d below the %d label channels' % (pad_to, c))
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('expand_labels: fp32 or bf16 output, got %s' % (dtype,))
    if ref.dim() == 5:
        if channels_last:
            raise ValueError('expand_labels: channels_last needs a 4-D label')
        b, t = ref.shape[:2]
        out = expand_labels(None if idx is None else idx.flatten(0, 1),
                            None if dense is None else dense.flatten(0, 1), layout,
                            size=size, pad_to=pad_to, dtype=dtype)
        return out.view((b, t) + tuple(out.shape[1:]))
    if size is not None:
        size = tuple(int(s) for s in _pair(size))
    if not _ext.use_native(ref):
        return expand_labels_reference(idx, dense, layout, size=size, pad_to=pad_to, dtype=dtype,
                                       channels_last=channels_last)
    h, w = ref.shape[-2:]
    ho, wo = size if size is not None else (h, w)
    kinds, cns, srcs, k, d = [], [], [], 0, 0
    for _, kind, out_ch, _n, _udc in layout:
        kinds.append(0 if kind == INDEX else 1)
        cns.append(out_ch)
        if kind == INDEX:
            srcs.append(k)
            k += 1
        else:
            srcs.append(d)
            d += out_ch
    return _ext.ext().label_expand(
        None if idx is None else idx.contiguous(), None if dense is None else dense.contiguous(),
        kinds, cns, srcs, c if pad_to is None else int(pad_to), ho, wo,
        _src_scale(h, ho, False, None), _src_scale(w, wo, False, None), dtype,
        bool(channels_last))


def cast_label(label, dtype):
    """``label.to(dtype)`` that keeps the packed source of an expanded fp32 label through the
    cast to bf16: it changes no value (zeros, ones) of the one-hot channels and rounds the dense
    ones exactly as the kernel's own bf16 output does. Every other cast drops the source (a
    bf16 label cast back to fp32 holds rounded dense values the source would not reproduce)."""
    out = label.to(dtype)
    src = getattr(label, '_iamd_packed_label', None)
    if src is not None and out is not label and label.dtype == torch.float32 and \
            dtype == torch.bfloat16:
        out._iamd_packed_label = src
    return out


def expand_packed_labels(data, layout, channels_last=False):
    """Replace ``label_idx`` / ``label_dense`` (and the ``few_shot_`` pair) of a batch by the
    ``label`` / ``few_shot_label`` the unpacked loader delivers: fp32, 4-D (channels-last when
    asked, as ``utils.misc.to_device`` makes 4-D float tensors) or 5-D ``[B, T, C, H, W]``. The
    result remembers its packed source (``_iamd_packed_label``) for
    ``LabelMapCache.resize``; any op that makes a new tensor drops the attribute."""
    for prefix in ('', 'few_shot_'):
        ki, kd = prefix + 'label_idx', prefix + 'label_dense'
        if ki not in data and kd not in data:
            continue
        if layout is None:
            raise RuntimeError('a packed label batch (%s) reached a trainer whose data loader '
                               'has no get_label_layout()' % ki)
        idx, dense = data.pop(ki, None), data.pop(kd, None)
        ref = idx if idx is not None else dense
        label = expand_labels(idx, dense, layout,
                              channels_last=channels_last and ref.dim() == 4)
        if label.dim() == 4:
            label._iamd_packed_label = PackedSource(idx, dense, [tuple(s) for s in layout])
        data[prefix + 'label'] = label
    return data
