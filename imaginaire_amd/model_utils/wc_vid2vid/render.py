"""World-consistent vid2vid point-cloud splat renderer
(reference model_utils/wc_vid2vid/render.py:11-199).

The reference keeps the colour / seen-mask / first-seen-time arrays of the
3-D point cloud in host numpy and re-renders per frame on the CPU. Two
renderers live here:

* ``DeviceSplatRenderer`` is what the generator and the trainer use. Its
  cloud has a fixed capacity and stays on the device (ops/splat.py, k18):
  the frame's point list, its length, the generated frame and the guidance
  image never visit the host, nothing is reallocated, and batch entries are
  rendered per sample, so the training iteration is captured as a hipGraph
  whose replays follow each batch's own points. What stays on the host: the
  ``N > Rcap`` shape check of ``unprojections_to_rows`` (tensor shapes, no
  device read) and ``num_points()`` / ``dropped()``, which read counters back
  for logging outside the step.
* ``SplatRenderer`` is the growing-array form of the reference with the
  arrays held in device tensors. It takes host point lists, reads the
  largest point id back to grow its arrays and returns numpy images, i.e. it
  synchronises with the host on every call; it is kept as the behavioural
  twin of the reference (tests/test_wc_render_cpu.py).

Semantics are the reference's: a point's colour is fixed the first time it is
seen; rendering writes the stored colour of every visible point and a mask
where the point has been seen. Duplicate targets (one point id listed
twice in a frame, two points projecting to one pixel) resolve as numpy's
fancy-index assignment does — the LAST row wins (reference render.py:87-97,
138). ``SplatRenderer`` gets there by a scatter-max of row numbers that keeps
only each target's winning row before a duplicate-free index_put (a plain
device index_put with duplicate indices has an undefined write order); the
kernels by an integer atomic max of row numbers. The one difference of the
device renderer: a row whose point id does not fit the capacity, or whose
pixel lies outside the image, is dropped and counted instead of growing the
arrays.
"""
import json
import os

import numpy as np
import torch


def _last_rows(target, size):
    """Boolean mask of the rows of ``target`` (1-D long) that are the last occurrence of their
    value: numpy's last-write-wins order for ``a[target] = values``, made deterministic."""
    rows = torch.arange(target.numel(), device=target.device)
    last = torch.full((size,), -1, dtype=torch.long, device=target.device)
    last.scatter_reduce_(0, target, rows, reduce='amax')
    return last[target] == rows


class SplatRenderer(object):
    def __init__(self, device=None):
        self.device = device
        self.reset()

    def reset(self):
        self.seen_mask = None
        self.seen_time = None
        self.colors = None
        self.call_idx = 0

    def num_points(self):
        return 0 if self.seen_mask is None else int(self.seen_mask.sum())

    def _as_index(self, point_info, device):
        p = torch.as_tensor(np.asarray(point_info), device=device).long()
        return p[:, 0], p[:, 1], p[:, 2]

    def _resize_arrays(self, max_point_idx, device):
        old = 0 if self.colors is None else self.colors.shape[0]
        if max_point_idx > old:
            colors = torch.zeros(max_point_idx, 3, dtype=torch.uint8, device=device)
            seen = torch.zeros(max_point_idx, 1, dtype=torch.uint8, device=device)
            seen_t = torch.zeros(max_point_idx, 1, dtype=torch.int32, device=device)
            if old:
                colors[:old] = self.colors
                seen[:old] = self.seen_mask
                seen_t[:old] = self.seen_time
            self.colors, self.seen_mask, self.seen_time = colors, seen, seen_t

    def update_point_cloud(self, image, point_info):
        """image: HxWx3 uint8 (numpy or tensor); point_info: Nx3 (i, j, point id)."""
        if point_info is None or len(point_info) == 0:
            return
        image = torch.as_tensor(np.ascontiguousarray(image) if isinstance(image, np.ndarray)
                                else image)
        device = self.device or image.device
        image = image.to(device)
        self.call_idx += 1
        i, j, pid = self._as_index(point_info, device)
        self._resize_arrays(int(pid.max()) + 1, device)
        keep = _last_rows(pid, self.colors.shape[0])
        i, j, pid = i[keep], j[keep], pid[keep]
        seen = self.seen_mask[pid]
        self.colors[pid] = seen * self.colors[pid] + (1 - seen) * image[i, j].to(torch.uint8)
        self.seen_time[pid] = seen.int() * self.seen_time[pid] + \
            (1 - seen.int()) * self.call_idx
        self.seen_mask[pid] = 1

    def render_image(self, point_info, w, h, return_mask=False):
        device = self.device or (self.colors.device if self.colors is not None else 'cpu')
        output = torch.zeros(h, w, 3, dtype=torch.uint8, device=device)
        mask = torch.zeros(h, w, 1, dtype=torch.uint8, device=device)
        if point_info is not None and len(point_info) != 0:
            i, j, pid = self._as_index(point_info, device)
            self._resize_arrays(int(pid.max()) + 1, device)
            keep = _last_rows(i * w + j, h * w)
            i, j, pid = i[keep], j[keep], pid[keep]
            output[i, j] = self.colors[pid]
            mask[i, j] = 255 * self.seen_mask[pid]
        output, mask = output.cpu().numpy(), mask.cpu().numpy()
        return (output, mask) if return_mask else output


# Point slots per sample of the device renderer (gen.guidance.max_points). A slot costs three
# int32 words (colour + seen flag, first-seen time, the update's winner word): 48 MiB per
# sample at the default, plus 4 bytes per guidance pixel (2 MiB at 512 x 1024).
DEFAULT_MAX_POINTS = 1 << 22


class DeviceSplatRenderer(object):
    """Fixed-capacity point cloud on the device (ops/splat.py). The state for
    ``(batch, max_points, device)`` is allocated on first use and afterwards only modified in
    place; ``update`` / ``render`` read nothing back."""

    def __init__(self, max_points=DEFAULT_MAX_POINTS):
        self.max_points = int(max_points)
        self.state = None

    def _state(self, batch, device):
        s = self.state
        if s is None or s.batch != batch or s.device != device:
            from imaginaire_amd.ops.splat import SplatState
            self.state = s = SplatState(batch, self.max_points, device)
        return s

    def reset(self):
        """Forget every point: zeroes the state in place and keeps the storage."""
        if self.state is not None:
            self.state.reset()

    def update(self, image, rows, counts):
        """image ``[B, 3, H, W]`` in [-1, 1]; rows int32 ``[B, R, 3]`` = (i, j, point id);
        counts int32 ``[B]`` valid leading rows."""
        from imaginaire_amd.ops.splat import splat_update
        splat_update(self._state(image.shape[0], image.device), image, rows, counts)

    def render(self, rows, counts, h, w):
        """fp32 ``[B, 4, h, w]`` guidance: colour in [-1, 1] and seen mask of the listed
        points, ``-1, -1, -1, 0`` elsewhere."""
        from imaginaire_amd.ops.splat import splat_render
        return splat_render(self._state(rows.shape[0], rows.device), rows, counts, h, w)

    # the only host reads: for logging, outside the training step
    def num_points(self):
        """Seen points per sample (list of int)."""
        if self.state is None:
            return []
        return ((self.state.color >> 24) & 1).sum(1).tolist()

    def dropped(self):
        """Rows dropped so far per sample (point id beyond the capacity or pixel outside the
        image), over updates and renders."""
        return [] if self.state is None else self.state.counters[:, 1].tolist()


def unprojections_to_rows(value, max_rows, width, is_flipped=None):
    """The padded point lists of a batch, ``[B, T, N + 1, 3]`` (padded with -1, the last row of
    each frame the length sentinel of ``decode_unprojections``), as what the device renderer
    takes: rows int32 ``[B, T, max_rows, 3]`` and counts int32 ``[B, T]``, on ``value``'s
    device, with nothing read back. ``is_flipped`` (bool, scalar or ``[B]``): the sample was
    flipped horizontally, so its valid rows get ``j -> width - 1 - j`` (the reference flips
    the frame before the update and the rendering after it: the same map, and a bijection, so
    the last row still wins). ``N > max_rows`` raises ValueError (a shape check)."""
    if value.dim() != 4 or value.shape[2] < 1 or value.shape[3] != 3:
        raise ValueError('unprojections: [B, T, N + 1, 3] expected, got %s' % (tuple(value.shape),))
    b, t, n = value.shape[0], value.shape[1], value.shape[2] - 1
    if n > max_rows:
        raise ValueError('unprojections hold up to %d rows per frame but gen.guidance.max_rows '
                         'is %d' % (n, max_rows))
    counts = value[:, :, -1, 0].clamp(0, n).to(torch.int32)
    rows = torch.zeros(b, t, max_rows, 3, dtype=torch.int32, device=value.device)
    body = value[:, :, :n].to(torch.int32)
    if is_flipped is not None:
        flip = torch.as_tensor(is_flipped, device=value.device).bool().reshape(-1, 1, 1)
        valid = torch.arange(n, device=value.device).view(1, 1, n) < counts.unsqueeze(-1)
        body[..., 1] = torch.where(valid & flip, width - 1 - body[..., 1], body[..., 1])
    rows[:, :, :n] = body
    return rows, counts


def _load_item(item):
    """Decode one serialized unprojection record: JSON (preferred) or, only
    when IMAGINAIRE_AMD_ALLOW_PICKLE=1, the reference's pickle format."""
    if isinstance(item, dict):
        return item
    if isinstance(item, (bytes, bytearray)):
        try:
            return json.loads(item.decode('utf-8'))
        except (UnicodeDecodeError, ValueError):
            if os.environ.get('IMAGINAIRE_AMD_ALLOW_PICKLE', '0') != '1':
                raise ValueError('unprojection record is not JSON; set '
                                 'IMAGINAIRE_AMD_ALLOW_PICKLE=1 to decode trusted pickles')
            import pickle
            return pickle.loads(item)  # noqa: S301 (explicit opt-in, trusted data)
    return json.loads(item)


def decode_unprojections(data):
    """List of per-frame {resolution: flat [i, j, id, ...]} records ->
    {resolution: [T, max_len + 1, 3] int array}; each row list is padded with
    -1 and ends with a sentinel row holding its length (render.py:150-199)."""
    per_res = {}
    for item in data:
        for resolution, value in _load_item(item).items():
            per_res.setdefault(resolution, []).append(list(value) if value else [])
    outputs = {}
    for resolution, values in per_res.items():
        max_len = max(len(v) for v in values)
        rows = []
        for v in values:
            assert len(v) % 3 == 0
            padded = v + [-1] * (max_len - len(v)) + [len(v) // 3] * 3
            rows.append(np.array(padded).reshape(-1, 3))
        outputs[resolution] = np.stack(rows, axis=0)
    return outputs
