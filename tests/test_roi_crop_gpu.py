"""k17 part boxes and box crops (csrc/roi_crop.hip) on the GPU.

Boxes: exactly the integers of the reference helpers run on a CPU copy of the label, for fp32 /
bf16 labels, NCHW / channels_last / non-dense strides, and W = 70 (16-byte body with scalar
head and tail). Crops: against slice + ``F.interpolate(align_corners=True)`` in float64.

Tolerances (inputs uniform in [-1, 1], source coordinates < 256): an fp32 source coordinate
carries an ulp <= 1.5e-5, which moves lambda by a few ulp against a neighbour difference <= 2,
over two axes: forward max abs <= 1e-4 in fp32; bf16 adds half an ulp at magnitude 1 (2^-9):
<= 4e-3. Backward: every contribution carries the same weight error: <= 1e-4 x max|reference|
in fp32; the bf16 gradient adds its own output rounding: bf16 keeps 8 significant bits, so half
an ulp is at most 2^-8 of the value, hence of max|reference| (unlike the forward's outputs the
gradients are not confined below 1, where half an ulp is 2^-9); dy is drawn in bf16, so it
carries no input error.
"""
import pytest
import torch
import torch.nn.functional as F

from imaginaire_amd.model_utils import fs_vid2vid as M
from imaginaire_amd.ops import _ext
from imaginaire_amd.ops.roi_crop import part_bbox, roi_crop_resize
from test_roi_crop_cpu import (B, DENSE_CFG, face_case, face_label, hand_label, mask_batches,
                               part_masks)

gpu = pytest.mark.gpu
DEV = 'cuda'
FWD_TOL = {torch.float32: 1e-4, torch.bfloat16: 4e-3}
BWD_TOL = {torch.float32: 1e-4, torch.bfloat16: 1e-4 + 2.0 ** -8}


def _layout(t, layout):
    if layout == 'nhwc':
        return t.contiguous(memory_format=torch.channels_last)
    if layout == 'strided':  # rows of a wider buffer: neither dense nor 16-byte aligned
        wide = torch.zeros(t.shape[:-1] + (t.shape[-1] + 3,), dtype=t.dtype, device=t.device)
        wide[..., 1:-2] = t
        return wide[..., 1:-2]
    return t.contiguous()


# (65, 70): planes of 4550 elements, so the OpenPose channel starts off a 16-byte boundary
@gpu
@pytest.mark.parametrize('layout', ['nchw', 'nhwc', 'strided'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('rule', ['face_densepose', 'face_openpose'])
@pytest.mark.parametrize('h,w', [(64, 96), (256, 256), (65, 70)])
def test_face_bbox_kernel_equals_cpu_helper(h, w, rule, dtype, layout):
    cfg, kw = face_case(rule)
    for crop_smaller in (0, 2):
        for names, mask in mask_batches(h, w):
            label = face_label(mask, rule, dtype)
            boxes = part_bbox(_layout(label.to(DEV), layout), rule=rule,
                              crop_smaller=crop_smaller, **kw)
            assert boxes.dtype == torch.int32 and boxes.shape == (B, 1, 5) and boxes.is_cuda
            want = [M.get_face_bbox_for_output(cfg, label[i:i + 1], crop_smaller=crop_smaller)
                    + [1] for i in range(B)]
            assert boxes[:, 0].tolist() == want, (names, crop_smaller)


@gpu
@pytest.mark.parametrize('layout', ['nchw', 'nhwc', 'strided'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('h,w', [(64, 96), (256, 256), (64, 70)])
def test_hand_bbox_kernel_equals_cpu_helper(h, w, dtype, layout):
    label = hand_label(h, w, dtype)
    boxes = part_bbox(_layout(label.to(DEV), layout), (-3, -2), rule='hand', equals=1)
    assert boxes[..., 4].tolist() == [[1, 1], [0, 1], [0, 0]]
    for i in range(B):
        got = [bx[:4] for bx in boxes[i].tolist() if bx[4]]
        assert got == M.get_hand_bbox_for_output(DENSE_CFG, label[i:i + 1])


# ---- crops -----------------------------------------------------------------------------------
def _face_boxes_256(kind):
    """[B, 1, 5] boxes on 256x256: 32-pixel boxes ('small') or the full image ('full')."""
    masks = part_masks(256, 256)
    if kind == 'full':
        mask = masks['full'].expand(B, 256, 256)
    else:
        mask = torch.zeros(B, 256, 256, dtype=torch.bool)
        mask[0, 40:50, 60:70] = True
        mask[1, 250:, 3:9] = True
        mask[2, 128, 128] = True
    boxes = part_bbox(face_label(mask, 'face_densepose').to(DEV), 2, rule='face_densepose',
                      threshold=0.9)
    side = 256 if kind == 'full' else 32
    assert all(bx[1] - bx[0] == side and bx[3] - bx[2] == side for bx in boxes[:, 0].tolist())
    return boxes


def _image(c, dtype, layout, h=256, w=256, seed=7):
    g = torch.Generator().manual_seed(seed)
    img = (torch.rand(B, c, h, w, generator=g) * 2 - 1).to(dtype)
    return _layout(img.to(DEV), 'nhwc' if layout == 'nhwc' else 'nchw')


def _oracle(image, boxes, out_hw, dy=None):
    """float64 slice + interpolate on the CPU (and its autograd gradient for ``dy``)."""
    img = image.detach().cpu().double().requires_grad_(dy is not None)
    crops = []
    for i in range(boxes.shape[0]):
        for ys, ye, xs, xe, _ in boxes[i].tolist():
            crops.append(F.interpolate(img[i:i + 1, -3:, ys:ye, xs:xe], size=out_hw,
                                       mode='bilinear', align_corners=True))
    out = torch.cat(crops)
    if dy is None:
        return out
    grad, = torch.autograd.grad(out, img, dy.detach().cpu().double())
    return out, grad


@gpu
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('c', [3, 6])
@pytest.mark.parametrize('kind', ['small', 'full'])
def test_crop_forward_against_float64(kind, c, dtype, layout):
    """32-pixel boxes up to 64 and the full 256 image down to 64; only the last 3 channels."""
    boxes = _face_boxes_256(kind)
    image = _image(c, dtype, layout)
    out = roi_crop_resize(image, boxes, (64, 64))
    assert out.shape == (B, 3, 64, 64) and out.dtype == dtype and out.is_contiguous()
    err = (out.cpu().double() - _oracle(image, boxes, (64, 64))).abs().max().item()
    print('roi_crop fwd %s c%d %s %s: max abs err %.3g' % (kind, c, dtype, layout, err))
    assert err <= FWD_TOL[dtype]


@gpu
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('c', [3, 6])
def test_hand_crop_is_bitwise_the_slice(c, dtype, layout):
    label = hand_label(256, 256).to(DEV)
    boxes = part_bbox(label, (-3, -2), rule='hand', equals=1)
    image = _image(c, dtype, layout)
    out = roi_crop_resize(image, boxes, (32, 32))
    want = torch.cat([image[i:i + 1, -3:, ys:ye, xs:xe] for i in range(B)
                      for ys, ye, xs, xe, _ in boxes[i].tolist()])
    assert out.shape == (2 * B, 3, 32, 32) and torch.equal(out, want)


@gpu
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('c', [3, 6])
@pytest.mark.parametrize('kind', ['small', 'full', 'hand', 'clipped'])
def test_crop_backward_against_float64(kind, c, dtype, layout):
    """dimage against float64 autograd; exactly 0 outside the boxes and in the channels before
    the last three; two runs bitwise equal; all under deterministic algorithms."""
    h, w, out_hw = 256, 256, (64, 64)
    if kind == 'hand':
        boxes = part_bbox(hand_label(256, 256).to(DEV), (-3, -2), rule='hand', equals=1)
        out_hw = (32, 32)
    elif kind == 'clipped':  # 64x96 full mask: a 96-pixel box on 64 rows, odd extents
        h, w, out_hw = 64, 96, (16, 16)
        label = face_label(part_masks(h, w)['full'].expand(B, h, w), 'face_densepose')
        boxes = part_bbox(label.to(DEV), 2, rule='face_densepose', threshold=0.9,
                          crop_smaller=1)
    else:
        boxes = _face_boxes_256(kind)
    torch.use_deterministic_algorithms(True)
    try:
        image = _image(c, dtype, layout, h, w).requires_grad_(True)
        out = roi_crop_resize(image, boxes, out_hw)
        g = torch.Generator().manual_seed(9)
        dy = torch.randn(out.shape, generator=g).to(dtype).to(DEV)
        got, = torch.autograd.grad(out, image, dy, retain_graph=True)
        again, = torch.autograd.grad(out, image, dy)
    finally:
        torch.use_deterministic_algorithms(False)
    assert got.shape == image.shape and got.dtype == dtype and got.stride() == image.stride()
    assert torch.equal(got, again)
    _, ref = _oracle(image, boxes, out_hw, dy)
    err = (got.cpu().double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print('roi_crop bwd %s c%d %s %s: max abs err %.3g, max |ref| %.3g' % (
        kind, c, dtype, layout, err, scale))
    assert scale > 0 and err <= BWD_TOL[dtype] * scale
    inside = torch.zeros(B, 1, h, w, dtype=torch.bool)
    for i in range(B):
        for ys, ye, xs, xe, _ in boxes[i].tolist():
            inside[i, :, max(ys, 0):ye, max(xs, 0):xe] = True
    got = got.cpu()
    assert (got[:, -3:][~inside.expand(B, 3, h, w)] == 0).all()
    assert (got[:, :-3] == 0).all()


# ---- public functions ------------------------------------------------------------------------
def _pose_batch(dtype=torch.float32):
    label = hand_label(256, 256)
    label[:, 2] = -1
    label[0, 2, 30:90, 100:140] = 1
    label[1, 2, 200:256, 0:30] = 1  # sample 2: no face, the default box
    image = _image(3, dtype, 'nchw', seed=11)
    return label.to(DEV), image


@gpu
def test_crop_face_from_output_matches_per_sample_path():
    label, image = _pose_batch()
    for crop_smaller in (0, 2):
        got = M.crop_face_from_output(DENSE_CFG, image, label, crop_smaller=crop_smaller)
        want = M._crop_face_per_sample(DENSE_CFG, image, label, crop_smaller=crop_smaller)
        assert got.shape == want.shape == (B, 3, 64, 64)
        assert (got - want).abs().max().item() <= FWD_TOL[torch.float32]
    both = M.crop_face_from_output(DENSE_CFG, [image, -image], label)
    assert isinstance(both, list) and len(both) == 2
    assert torch.equal(both[0], M.crop_face_from_output(DENSE_CFG, image, label))
    assert torch.equal(both[1], -both[0])


@gpu
def test_crop_hand_from_output_matches_per_sample_path():
    label, image = _pose_batch()
    got = M.crop_hand_from_output(DENSE_CFG, image, label)
    want = M._crop_hand_per_sample(DENSE_CFG, image, label)
    assert got.shape == want.shape == (3, 3, 32, 32) and torch.equal(got, want)
    both = M.crop_hand_from_output(DENSE_CFG, [image, -image], label)
    assert torch.equal(both[0], want) and torch.equal(both[1], -want)
    label[:, -3:-1] = 0
    assert M.crop_hand_from_output(DENSE_CFG, image, label) is None
    assert M.crop_hand_from_output(DENSE_CFG, [image, image], label) == [None, None]


@gpu
def test_face_path_runs_without_host_reads():
    label, image = _pose_batch()
    image.requires_grad_(True)
    M.crop_face_from_output(DENSE_CFG, image, label).sum().backward()  # code objects loaded
    image.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        M.crop_face_from_output(DENSE_CFG, image, label, crop_smaller=1).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert image.grad is not None and bool((image.grad != 0).any())


@gpu
def test_captured_crop_follows_the_label():
    """part_bbox -> roi_crop_resize -> backward captured over static buffers: a replay on a
    different label (the face elsewhere) equals a fresh eager call bitwise."""
    assert _ext.available()
    masks = torch.zeros(2, B, 256, 256, dtype=torch.bool)
    masks[0, :, 20:80, 30:70] = True
    masks[1, 0, 150:250, 120:200] = True
    masks[1, 1, 0:5, 250:256] = True  # sample 2 of the second label: no face
    labels = [face_label(m, 'face_densepose').to(DEV) for m in masks]
    image = _image(6, torch.float32, 'nchw', seed=13).requires_grad_(True)
    dy = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(14)).to(DEV)
    static_label = labels[0].clone()

    def step(label):
        boxes = part_bbox(label, 2, rule='face_densepose', threshold=0.9)
        out = roi_crop_resize(image, boxes, (64, 64))
        grad, = torch.autograd.grad(out, image, dy)
        return boxes, out, grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(static_label)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        boxes_g, out_g, grad_g = step(static_label)
    for label in (labels[1], labels[0]):
        static_label.copy_(label)
        graph.replay()
        torch.cuda.synchronize()
        boxes_e, out_e, grad_e = step(label)
        assert torch.equal(boxes_g, boxes_e)
        assert torch.equal(out_g, out_e) and torch.equal(grad_g, grad_e)
    first = part_bbox(labels[0], 2, rule='face_densepose', threshold=0.9)
    second = part_bbox(labels[1], 2, rule='face_densepose', threshold=0.9)
    assert not torch.equal(first, second)
