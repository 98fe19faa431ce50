"""Point-cloud splat renderer that stays on the device (k18, ``csrc/splat.hip``).

Reference model_utils/wc_vid2vid/render.py:63-147 keeps the colour / seen / first-seen-time
arrays of the 3-D point cloud in host numpy, grows them to the largest point id of every frame
and updates / renders them with fancy-index assignments: host state that a hipGraph cannot
record and that would freeze the capture-time cloud into every replay. Here the cloud has a
FIXED capacity of ``P`` points per sample, lives in :class:`SplatState` and is only ever
modified in place:

* :func:`splat_update` gives every listed point that is not yet seen the colour of its pixel
  (quantised exactly as ``tensor2im`` does; NaN maps to 0) and the call index as its time;
* :func:`splat_render` writes the stored colours and the seen flags of the listed points into
  a ``[B, 4, h, w]`` guidance image (``-1, -1, -1, 0`` where nothing is listed).

The list is ``rows`` int32 ``[B, R, 3]`` = ``(i, j, point id)`` with ``counts`` int32 ``[B]``
valid leading rows per sample; ``counts`` is read on the device and rows past it are ignored.
Duplicate targets resolve as numpy's fancy assignment does (the last row wins). Rows that
cannot be applied (point id outside ``[0, P)``, pixel outside the image) are dropped and
counted: the one difference from the reference, which grows its arrays instead.

GPU tensors run the HIP kernels; CPU tensors and ``_ext.force_eager()`` run the PyTorch
reference below, written without host reads as well (``scatter_reduce_(amax)`` of row numbers,
gathers and scatters of fixed shape), which is also the oracle of the kernels. The guidance is
rendered from uint8 state, so there is no backward.
"""
import torch

from imaginaire_amd.ops import _ext

SEEN = 1 << 24  # colour word: R | G << 8 | B << 16 | seen << 24


class SplatState(object):
    """The cloud of ``batch`` samples x ``max_points`` point slots on ``device``: allocated
    once, modified in place only (a captured graph keeps valid pointers)."""

    def __init__(self, batch, max_points, device):
        self.batch, self.max_points, self.device = int(batch), int(max_points), device
        if self.max_points < 1:
            raise ValueError('SplatState: max_points must be positive')
        shape = (self.batch, self.max_points)
        self.color = torch.zeros(shape, dtype=torch.int32, device=device)
        self.seen_time = torch.zeros(shape, dtype=torch.int32, device=device)
        # call_idx, dropped rows, 2 spare
        self.counters = torch.zeros((self.batch, 4), dtype=torch.int32, device=device)
        # winner tables of the kernels' last-row-wins passes: -1 between calls
        self.win_pt = torch.full(shape, -1, dtype=torch.int32, device=device)
        self.win_px = {}

    def pixel_winners(self, hw):
        """The per-pixel winner table of an ``hw``-pixel guidance image (made on first use)."""
        if hw not in self.win_px:
            self.win_px[hw] = torch.full((self.batch, hw), -1, dtype=torch.int32,
                                         device=self.device)
        return self.win_px[hw]

    def reset(self):
        """Forget every point, in place (the winner tables already hold -1)."""
        self.color.zero_()
        self.seen_time.zero_()
        self.counters.zero_()


def quantise(x):
    """``tensor2im``'s uint8 of a [-1, 1] tensor, as int32: ``(x + 1) / 2 * 255`` in fp32,
    clamped to [0, 255], truncated; NaN gives 0."""
    t = (x.float() + 1) / 2 * 255
    return torch.where(t != t, torch.zeros_like(t), t).clamp(0, 255).to(torch.int32)


def _check(state, rows, counts):
    if rows.dim() != 3 or rows.shape[2] != 3 or rows.shape[0] != state.batch:
        raise ValueError('splat: rows must be [B, R, 3] with the batch of the state')
    if counts.shape != (state.batch,):
        raise ValueError('splat: counts must be [B]')


def _listed(state, rows, counts, h, w):
    """(i, j, pid as int64 [B, R]; ok [B, R]: the row is listed and can be applied); counts
    the listed rows that cannot into the drop counter."""
    r = rows.shape[1]
    n = counts.clamp(0, r).long()
    i, j, pid = rows.long().unbind(-1)
    listed = torch.arange(r, device=rows.device).unsqueeze(0) < n.unsqueeze(1)
    ok = listed & (pid >= 0) & (pid < state.max_points) & (i >= 0) & (i < h) & (j >= 0) & (j < w)
    state.counters[:, 1] += (listed & ~ok).sum(1).to(torch.int32)
    return i, j, pid, ok, n


def _winners(target, ok, size):
    """last [B, size + 1]: the largest row number among the ``ok`` rows of each target, -1
    where there is none (slot ``size`` collects the other rows); and the routed targets."""
    b, r = target.shape
    tgt = torch.where(ok, target, torch.full_like(target, size))
    rown = torch.arange(r, device=target.device).expand(b, r)
    last = torch.full((b, size + 1), -1, dtype=torch.long, device=target.device)
    last.scatter_reduce_(1, tgt, rown, reduce='amax')
    return last, tgt, rown


def splat_update_reference(state, image, rows, counts):
    """PyTorch form of :func:`splat_update` with no host read."""
    b, _, h, w = image.shape
    p = state.max_points
    i, j, pid, ok, n = _listed(state, rows, counts, h, w)
    state.counters[:, 0] += (n > 0).to(torch.int32)
    if rows.shape[1] == 0:
        return
    last, tgt, rown = _winners(pid, ok, p)
    wins = ok & (last.gather(1, tgt) == rown)
    bi = torch.arange(b, device=image.device).unsqueeze(1)
    q = quantise(image[bi, :, i.clamp(0, h - 1), j.clamp(0, w - 1)])  # [B, R, 3]
    word = q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | SEEN
    pad = torch.zeros(b, 1, dtype=torch.int32, device=image.device)
    color = torch.cat([state.color, pad], 1)
    seen_time = torch.cat([state.seen_time, pad], 1)
    write = wins & ((color.gather(1, tgt) & SEEN) == 0)
    # at most one writing row per point; all the others go to the spare slot p
    tgt = torch.where(write, pid, torch.full_like(pid, p))
    color.scatter_(1, tgt, word)
    seen_time.scatter_(1, tgt, state.counters[:, :1].expand_as(word))
    state.color.copy_(color[:, :p])
    state.seen_time.copy_(seen_time[:, :p])


_TABLES = {}


def _unquantise_table(device):
    """``(c / 255 - 0.5) * 2`` for c = 0 .. 255, computed on the CPU as the reference generator
    does (PyTorch's GPU division by a scalar multiplies by the reciprocal, which rounds
    differently) and kept on ``device``."""
    if device not in _TABLES:
        _TABLES[device] = torch.arange(256).float().div(255).sub(0.5).mul(2).to(device)
    return _TABLES[device]


def splat_render_reference(state, rows, counts, h, w):
    """PyTorch form of :func:`splat_render` with no host read."""
    b, p, hw = state.batch, state.max_points, h * w
    if rows.shape[1] == 0:
        word = torch.zeros(b, hw, dtype=torch.int32, device=rows.device)
    else:
        i, j, pid, ok, _ = _listed(state, rows, counts, h, w)
        last = _winners(i * w + j, ok, hw)[0][:, :hw]
        shown = pid.gather(1, last.clamp(min=0)).clamp(0, p - 1)
        # an unlisted pixel shows the reference's zero image: word 0
        word = state.color.gather(1, shown) * (last >= 0).to(torch.int32)
    rgb = torch.stack([word & 255, (word >> 8) & 255, (word >> 16) & 255], 1)
    rgb = _unquantise_table(rows.device)[rgb.long()]
    mask = ((word >> 24) & 1).float().unsqueeze(1)
    return torch.cat([rgb, mask], 1).view(b, 4, h, w)


def _native_rows(rows, counts):
    rows = rows.to(torch.int32)
    if rows.stride(2) != 1 or rows.stride(1) != 3:
        rows = rows.contiguous()
    return rows, counts.to(torch.int32)


def splat_update(state, image, rows, counts):
    """Colour the points of ``state`` that ``rows[b, :counts[b]]`` list and that are not yet
    seen with the pixels of ``image [B, 3, H, W]`` (fp32 or bf16, any strides), in place. A
    sample with ``counts[b] == 0`` is left alone; otherwise its ``call_idx`` advances by one
    and is the ``seen_time`` of the points it colours."""
    if image.dim() != 4 or image.shape[1] != 3 or image.shape[0] != state.batch:
        raise ValueError('splat_update: [B, 3, H, W] image with the batch of the state expected')
    _check(state, rows, counts)
    if not _ext.use_native(image):
        return splat_update_reference(state, image, rows, counts)
    if image.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('splat_update: the kernel takes fp32 or bf16 images, got %s' % image.dtype)
    rows, counts = _native_rows(rows, counts)
    _ext.ext().splat_update(image, rows, counts, state.color, state.seen_time, state.counters,
                            state.win_pt)


def splat_render(state, rows, counts, h, w):
    """fp32 ``[B, 4, h, w]``: channels 0-2 ``(c / 255 - 0.5) * 2`` of the stored colour of the
    point each listed pixel shows, channel 3 its seen flag; ``-1, -1, -1, 0`` elsewhere."""
    h, w = int(h), int(w)
    _check(state, rows, counts)
    if not _ext.use_native(state.color):
        return splat_render_reference(state, rows, counts, h, w)
    rows, counts = _native_rows(rows, counts)
    return _ext.ext().splat_render(rows, counts, state.color, state.counters,
                                   state.pixel_winners(h * w), h, w)
