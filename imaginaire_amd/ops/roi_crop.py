"""Part boxes and box crops that stay on the device (k17, ``csrc/roi_crop.hip``).

Reference model_utils/fs_vid2vid.py:631-777 finds the face / hand box of every sample with
``.nonzero()`` and four ``.item()`` reads, slices with the resulting Python integers and calls
``F.interpolate`` per sample: five host reads per sample per crop, none of which a hipGraph
can record, and a box that is host state (a capture would replay the capture-time box for
ever). Here

* :func:`part_bbox` reduces each (sample, part channel) plane to its box on the device and
  applies the reference's box rule in integer arithmetic: ``int32 [B, n, 5]`` holding
  ``ys, ye, xs, xe, valid``, equal to ``get_face_bbox_for_output`` /
  ``get_hand_bbox_for_output`` as integers;
* :func:`roi_crop_resize` crops the last 3 image channels to those boxes (clipped to the image
  as a Python slice is) and resizes bilinearly with ``align_corners=True``; its backward is a
  gather over the whole image gradient (no atomics, nothing to zero, deterministic).

GPU tensors run the HIP kernels; CPU tensors and ``_ext.force_eager()`` run the PyTorch
reference below, written without host reads as well (masked ``amin`` / ``amax`` over index
grids, integer tensor arithmetic, gathers by computed indices), which is also the numerics
oracle of the kernels.
"""
import torch

from imaginaire_amd.ops import _ext

RULES = {'face_openpose': 0, 'face_densepose': 1, 'hand': 2}


def _channels(label, channel):
    chans = [channel] if isinstance(channel, int) else list(channel)
    c = label.shape[1]
    chans = [ch + c if ch < 0 else ch for ch in chans]
    if not chans or any(ch < 0 or ch >= c for ch in chans):
        raise ValueError('part_bbox: channel %r out of range for %d channels' % (channel, c))
    return chans


def _clamp_centre(c, length, dim):
    # max(len // 2, min(dim - 1 - len // 2, c)), the reference's order
    return torch.maximum(length // 2, torch.minimum(dim - 1 - length // 2, c))


def part_bbox_reference(label, channel, *, rule, threshold=None, equals=None, crop_smaller=0):
    """PyTorch form of :func:`part_bbox` with no host read."""
    chans = _channels(label, channel)
    h, w = label.shape[-2:]
    plane = label[:, chans]
    mask = plane == equals if equals is not None else plane > threshold
    dev = label.device
    yy = torch.arange(h, device=dev).view(1, 1, h, 1)
    xx = torch.arange(w, device=dev).view(1, 1, 1, w)
    big = max(h, w)
    y0 = torch.where(mask, yy, big).amin((2, 3))
    y1 = torch.where(mask, yy, -1).amax((2, 3))
    x0 = torch.where(mask, xx, big).amin((2, 3))
    x1 = torch.where(mask, xx, -1).amax((2, 3))
    empty = y1 < 0
    zero = torch.zeros_like(y0)
    if rule == 'hand':
        length = zero + h // 64 * 8
        yc = _clamp_centre(torch.where(empty, zero, (y0 + y1) // 2), length, h)
        xc = _clamp_centre(torch.where(empty, zero, (x0 + x1) // 2), length, w)
        valid = (~empty).long()
    else:
        xc = (x0 + x1) // 2
        if rule == 'face_openpose':
            yc = (3 * y0 + 2 * y1) // 5
            length = (5 * (x1 - x0)) // 2
        elif rule == 'face_densepose':
            yc = (y0 + y1) // 2
            length = (5 * (y1 - y0)) // 4
        else:
            raise ValueError('part_bbox: unknown rule %r' % (rule,))
        length = length.clamp(min=32).clamp(max=w)
        yc = _clamp_centre(yc, length, h)
        xc = _clamp_centre(xc, length, w)
        length = torch.where(empty, zero + h // 32 * 8, length)
        yc = torch.where(empty, zero + h // 4, yc)
        xc = torch.where(empty, zero + w // 2, xc)
        valid = torch.ones_like(y0)
    half = length // 2
    box = [yc - half + crop_smaller, yc + half - crop_smaller,
           xc - half + crop_smaller, xc + half - crop_smaller, valid]
    return torch.stack(box, -1).to(torch.int32)


def part_bbox(label, channel, *, rule, threshold=None, equals=None, crop_smaller=0):
    """Box of the pixels of ``label[:, channel]`` (an int or a sequence of ints, negative from
    the end) that are ``> threshold`` or ``== equals``: ``int32 [B, n, 5]`` =
    ``ys, ye, xs, xe, valid`` under ``rule`` ('face_openpose', 'face_densepose': square face
    box, ``valid`` always 1, a default box on an empty mask; 'hand': fixed-size box,
    ``valid`` 0 on an empty mask)."""
    if rule not in RULES:
        raise ValueError('part_bbox: unknown rule %r' % (rule,))
    if (threshold is None) == (equals is None):
        raise ValueError('part_bbox: give exactly one of threshold / equals')
    if label.dim() != 4:
        raise ValueError('part_bbox: [B, C, H, W] label expected')
    if not _ext.use_native(label):
        return part_bbox_reference(label, channel, rule=rule, threshold=threshold,
                                   equals=equals, crop_smaller=crop_smaller)
    ref = equals if equals is not None else threshold
    # torch compares a tensor with a Python scalar in the tensor's dtype
    ref = float(torch.tensor(ref, dtype=label.dtype))
    return _ext.ext().part_bbox(label, _channels(label, channel), RULES[rule],
                                equals is not None, ref, int(crop_smaller))


def _axis_taps(start, end, dim, out, dtype):
    """Per box: source indices (absolute, clamped into the image) and weight of the second tap
    for every output index of one axis; PyTorch's align_corners=True rule on the box clipped
    to [0, dim). Returns (i0 [N, out], i1 [N, out], lambda [N, out], non-empty [N])."""
    start = start.clamp(min=0)
    n_in = end.clamp(max=dim) - start
    if out > 1:
        scale = (n_in - 1).to(dtype) / (out - 1)
    else:
        scale = torch.zeros_like(n_in, dtype=dtype)
    o = torch.arange(out, device=start.device, dtype=dtype)
    src = scale.unsqueeze(1) * o
    i0 = src.long()
    i1 = i0 + (i0 < (n_in - 1).unsqueeze(1)).long()
    lam = src - i0.to(dtype)
    base = start.unsqueeze(1)
    return (base + i0).clamp(0, dim - 1), (base + i1).clamp(0, dim - 1), lam, n_in > 0


def roi_crop_resize_reference(image, boxes, out_hw):
    """PyTorch form of :func:`roi_crop_resize` (differentiable in ``image``), no host read."""
    oh, ow = out_hw
    b, c, h, w = image.shape
    n = boxes.shape[1]
    acc = torch.float64 if image.dtype == torch.float64 else torch.float32
    bx = boxes.reshape(b * n, 5).long()
    y0, y1, ly, oky = _axis_taps(bx[:, 0], bx[:, 1], h, oh, acc)
    x0, x1, lx, okx = _axis_taps(bx[:, 2], bx[:, 3], w, ow, acc)
    img = image[:, c - 3:].to(acc)
    bi = torch.arange(b, device=image.device).repeat_interleave(n).view(-1, 1, 1, 1)
    ci = torch.arange(3, device=image.device).view(1, 3, 1, 1)

    def tap(yi, xi):
        return img[bi, ci, yi.view(-1, 1, oh, 1), xi.view(-1, 1, 1, ow)]
    ly = ly.view(-1, 1, oh, 1)
    lx = lx.view(-1, 1, 1, ow)
    out = (1 - ly) * ((1 - lx) * tap(y0, x0) + lx * tap(y0, x1)) + \
        ly * ((1 - lx) * tap(y1, x0) + lx * tap(y1, x1))
    out = out * (oky & okx).view(-1, 1, 1, 1).to(acc)
    return out.to(image.dtype)


class _RoiCropResize(torch.autograd.Function):
    """k17 crop + resize; gather-form backward that writes the whole image gradient."""

    @staticmethod
    def forward(ctx, image, boxes, oh, ow):
        ctx.save_for_backward(boxes)
        # the backward writes dimage in the image's own layout
        ctx.like = image if _ext.is_dense(image) else image.contiguous()
        ctx.like = torch.empty_strided(ctx.like.shape, ctx.like.stride(), device='meta',
                                       dtype=image.dtype)
        return _ext.ext().roi_crop_fwd(image, boxes, oh, ow)

    @staticmethod
    def backward(ctx, dy):
        boxes, = ctx.saved_tensors
        dy = dy.to(ctx.like.dtype).contiguous()
        return _ext.ext().roi_crop_bwd(dy, boxes, ctx.like), None, None, None


def roi_crop_resize(image, boxes, out_hw):
    """``[B * n, 3, oh, ow]``: the last 3 channels of ``image [B, C, H, W]`` cropped to
    ``boxes [B, n, 5]`` (from :func:`part_bbox`; read on the device) and resized bilinearly
    with ``align_corners=True``, sample-major. Differentiable in ``image`` only."""
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if image.dim() != 4 or image.shape[1] < 3:
        raise ValueError('roi_crop_resize: [B, C >= 3, H, W] image expected')
    if boxes.dim() != 3 or boxes.shape[0] != image.shape[0] or boxes.shape[2] != 5:
        raise ValueError('roi_crop_resize: boxes must be [B, n, 5]')
    if not _ext.use_native(image):
        return roi_crop_resize_reference(image, boxes, (oh, ow))
    if image.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('roi_crop_resize: the kernel takes fp32 or bf16 images, got %s' %
                        image.dtype)
    boxes = boxes.to(device=image.device, dtype=torch.int32).contiguous()
    return _RoiCropResize.apply(image, boxes, oh, ow)
