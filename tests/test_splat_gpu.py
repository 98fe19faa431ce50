"""The k18 HIP kernels (csrc/splat.hip) vs the numpy oracle of tests/test_splat_cpu.py, bit for
bit (GPU): colours, seen flags, times and counters are integers, the guidance a float derived
from one uint8. Every operation runs twice from the same state and must repeat itself exactly
(determinism: the last-row-wins resolution may not depend on the order blocks run in)."""
import numpy as np
import pytest
import torch

import test_splat_cpu as sc

H, W, RCAP = sc.H, sc.W, sc.RCAP


def _dev():
    return torch.device('cuda', 0)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,channels_last', [(torch.float32, False), (torch.bfloat16, True)])
def test_kernels_match_numpy(dtype, channels_last):
    sc.check_sequence(_dev(), 128, sc.small_frames(), H, W, dtype=dtype,
                      channels_last=channels_last, twice=True)


@pytest.mark.gpu
def test_empty_and_full_lists():
    # counts = 0 (nothing changes, background only) and counts = Rcap (no row is padding)
    rows = [150, RCAP, 0, RCAP]
    frames = sc.small_frames(rows=lambda frame, b: rows[frame])
    ren, clouds = sc.check_sequence(_dev(), 128, frames, H, W, twice=True)
    assert clouds[0].call_idx == 3


@pytest.mark.gpu
def test_rows_beyond_the_capacity_are_dropped_and_counted():
    frames = sc.small_frames()
    frames[1][1][0, 5, 0] = H
    frames[1][1][0, 9, 1] = -1
    frames[3][1][0, 0, 2] = -7
    frames[3][1][0, 1, 2] = 2 ** 31 - 1
    ren, clouds = sc.check_sequence(_dev(), 64, frames, H, W, dtype=torch.bfloat16,
                                    channels_last=True, twice=True)
    assert clouds[0].dropped > 6


@pytest.mark.gpu
def test_batch_of_two_and_strided_rows():
    frames = sc.small_frames(batch=2, rows=lambda frame, b: (150, 97 - 30 * frame)[b])

    def frame_view(rows, counts):
        # what the trainer hands over: frame t of [B, T, Rcap, 3], a strided batch
        seq = torch.full((2, 3, RCAP, 3), 5, dtype=torch.int32)
        seq[:, 1] = rows
        return seq
    ren = sc.check_sequence(_dev(), 128, frames, H, W, twice=True)[0]
    view = sc.check_sequence(
        _dev(), 128, frames, H, W,
        rows_for_device=lambda rows, counts: frame_view(rows, counts).to(_dev())[:, 1])[0]
    assert all(torch.equal(a, b) for a, b in zip(sc.state_tensors(ren), sc.state_tensors(view)))


@pytest.mark.gpu
def test_flipped_input_equals_the_reference_flip():
    def flipped(rows, counts):
        value = torch.cat([rows.long(), counts.long().view(-1, 1, 1).expand(-1, 1, 3)], 1)
        return sc.unprojections_to_rows(value.unsqueeze(1).to(_dev()), RCAP, W,
                                        is_flipped=torch.tensor([True]))[0][:, 0]
    sc.check_sequence(_dev(), 128, sc.small_frames(), H, W, oracle_flip=True,
                      rows_for_device=flipped)


@pytest.mark.gpu
def test_many_workgroups():
    """64 x 128, Rcap = 20000, counts = 17001 (no multiple of the wave or block size), ids in
    [0, 6000) so most ids repeat, ~58 % of the rows on an already listed pixel: the smallest
    shape at which a cross-block race in the last-row-wins resolution can show."""
    frames = sc.make_frames(3, 1, 64, 128, 20000, lambda frame, b: 17001, lambda frame: 6000,
                            frames=3)
    sc.check_sequence(_dev(), 8192, frames, 64, 128, twice=True)
    sc.check_sequence(_dev(), 8192, frames, 64, 128, dtype=torch.bfloat16, channels_last=True)


@pytest.mark.gpu
def test_render_writes_every_element():
    """The output buffer holds NaN before the kernels run (torch's fill of uninitialised
    memory, and a freed NaN block of the output's size for the allocator to hand back): every
    element must be defined afterwards, for a vectorised size and an odd one, with a list
    and without."""
    from imaginaire_amd.model_utils.wc_vid2vid.render import DeviceSplatRenderer
    dev = _dev()
    det, fill = torch.are_deterministic_algorithms_enabled(), \
        torch.utils.deterministic.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    try:
        for h, w in ((12, 16), (5, 7)):
            ren = DeviceSplatRenderer(128)
            rng = np.random.RandomState(h)
            rows = np.stack([rng.randint(0, h, (2, 40)), rng.randint(0, w, (2, 40)),
                             rng.randint(0, 128, (2, 40))], -1)
            rows = torch.from_numpy(rows).int().to(dev)
            image = torch.rand(2, 3, h, w, device=dev) * 2 - 1
            for counts in ([40, 0], [0, 0], [17, 40]):
                counts = torch.tensor(counts, dtype=torch.int32, device=dev)
                ren.update(image, rows, counts)
                poison = torch.full((2, 4, h, w), float('nan'), device=dev)
                del poison
                out = ren.render(rows, counts, h, w)
                assert torch.isfinite(out).all()
                assert ((out[:, :3] >= -1) & (out[:, :3] <= 1)).all()
                assert ((out[:, 3] == 0) | (out[:, 3] == 1)).all()
    finally:
        torch.utils.deterministic.fill_uninitialized_memory = fill
        torch.use_deterministic_algorithms(det)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_quantisation_is_tensor2im(dtype):
    sc.test_quantisation_is_tensor2im(dtype, device=_dev())


@pytest.mark.gpu
def test_eager_reference_on_the_gpu_matches_too():
    """``_ext.force_eager()`` routes GPU tensors to the PyTorch reference, the kernels' oracle."""
    from imaginaire_amd.ops import _ext
    with _ext.eager_scope():
        sc.check_sequence(_dev(), 128, sc.small_frames(), H, W)
