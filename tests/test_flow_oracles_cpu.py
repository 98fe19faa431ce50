"""The float64 oracles of ``test_flow_paths_gpu.py`` checked on the CPU: the cost-volume oracle
against a loop-per-element brute force (taps outside the frame read zero, whatever the
``pad_size``), the package's fp32 references (the CPU paths of the ops) against the oracles, and
the k6 case table against the kernels it has to reach. No GPU needed.
"""
import pytest
import torch

from test_flow_paths_gpu import (FP32, _K6_EXTRA, _K6_ROWS, _check, _corr_out_size, _corr_ref64,
                                 _flows, _randn, _resample_ref64, _warp_ref64)

# (C, H, W), (pad, ks, md, s1, s2): pad < md, pad > md, md % s2 != 0, a window with both
# strides 2, taps that leave the padded frame (pad 0 and md % s2 == 0), one pixel
_CORR_CASES = [
    ((3, 5, 7), (2, 1, 4, 1, 1)),
    ((3, 5, 7), (6, 1, 4, 1, 2)),
    ((3, 5, 7), (3, 1, 3, 1, 2)),
    ((3, 9, 11), (4, 3, 3, 2, 2)),
    ((3, 6, 8), (0, 3, 1, 1, 1)),
    ((3, 6, 8), (3, 3, 2, 2, 1)),
    ((2, 1, 1), (4, 1, 4, 1, 2)),
]
_CORR_IDS = ['%dx%dx%d-%s' % (s + ('_'.join(map(str, p)),)) for s, p in _CORR_CASES]


def _corr_brute(a, b, pad, ks, md, s1, s2):
    """One output element at a time from the unpadded inputs; a tap outside the image is 0."""
    n, c, h, w = a.shape
    kr, R = (ks - 1) // 2, md // s2
    D = 2 * R + 1
    oh, ow = _corr_out_size(h, pad, ks, md, s1), _corr_out_size(w, pad, ks, md, s1)
    out = torch.zeros(n, D * D, oh, ow, dtype=torch.float64)

    def px(t, y, x):
        if 0 <= y < h and 0 <= x < w:
            return t[:, :, y, x]
        return torch.zeros(n, c, dtype=torch.float64)
    for tj in range(-R, R + 1):
        for ti in range(-R, R + 1):
            for oy in range(oh):
                for ox in range(ow):
                    y1, x1 = oy * s1 + md - pad, ox * s1 + md - pad  # image coordinates
                    acc = 0.
                    for j in range(-kr, kr + 1):
                        for i in range(-kr, kr + 1):
                            acc = acc + (px(a, y1 + j, x1 + i) *
                                         px(b, y1 + j + tj * s2, x1 + i + ti * s2)).sum(1)
                    out[:, (tj + R) * D + ti + R, oy, ox] = acc
    return out / (ks * ks * c)


def _corr_inputs(shape):
    a = _randn((2,) + shape, 5, device='cpu')
    b = _randn((2,) + shape, 6, device='cpu')
    return a, b


@pytest.mark.parametrize('shape,params', _CORR_CASES, ids=_CORR_IDS)
def test_corr_oracle_matches_brute_force(shape, params):
    a, b = _corr_inputs(shape)
    ref = _corr_ref64(a.double(), b.double(), *params)
    brute = _corr_brute(a.double(), b.double(), *params)
    assert ref.shape == brute.shape
    assert float((ref - brute).abs().max()) <= 1e-13


@pytest.mark.parametrize('shape,params', _CORR_CASES, ids=_CORR_IDS)
def test_correlation_reference_matches_oracle(shape, params):
    """The CPU path of the op, fp32, by the tolerance rule of the GPU module. At (0, 3, 1, 1, 1)
    the window reaches row -1 of the frame: zero, not the last row."""
    from imaginaire_amd.ops.flownet_ops import correlation_reference
    a, b = _corr_inputs(shape)
    ks = params[1]
    ref = _corr_ref64(a.double(), b.double(), *params)
    s_out = _corr_ref64(a.double().abs(), b.double().abs(), *params)
    _check(correlation_reference(a, b, *params), ref, ks * ks * shape[0] + 4, s_out,
           'correlation_reference', 'out')


def _in_frame_flow(B, H, W, seed):
    """Fractional flows whose samples stay strictly inside the image."""
    g = torch.Generator().manual_seed(seed)
    tx = 0.05 + (W - 1.1) * torch.rand(B, H, W, generator=g)
    ty = 0.05 + (H - 1.1) * torch.rand(B, H, W, generator=g)
    xs = torch.arange(W, dtype=FP32).view(1, 1, W)
    ys = torch.arange(H, dtype=FP32).view(1, H, 1)
    return torch.stack([tx - xs, ty - ys], 1)


def test_warp_oracle_matches_grid_sample_reference():
    """``flow_warp_reference`` samples through grid_sample's normalised fp32 coordinates: the
    position is off by a few roundings at magnitude W (3 * 2^-24 * 23 < 5e-6 px), times a slope
    of at most max - min of the randn image (< 10): 1e-4 absolute."""
    from imaginaire_amd.ops.flow_warp import flow_warp_reference
    B, C, H, W = 2, 3, 17, 23
    img = _randn((B, C, H, W), 7, device='cpu')
    flow = _in_frame_flow(B, H, W, 8)
    ref = _warp_ref64(img.double(), flow)
    got = flow_warp_reference(img, flow)
    assert float((got.double() - ref).abs().max()) <= 1e-4


@pytest.mark.parametrize('ks', [1, 2, 3])
@pytest.mark.parametrize('kind', ['frac', 'int'])
def test_resample_oracle_matches_reference(kind, ks):
    from imaginaire_amd.ops.flownet_ops import resample2d_reference
    B, C, H, W = 2, 3, 17, 23
    img = _randn((B, C, H, W), 9, device='cpu')
    flow = _flows(kind, B, H, W, 10, device='cpu')
    ref = _resample_ref64(img.double(), flow, ks)
    s_out = _resample_ref64(img.double().abs(), flow, ks)
    _check(resample2d_reference(img, flow, ks), ref, 4 * ks * ks + 4, s_out,
           'resample2d_reference', 'out')


def test_k6_table_reaches_every_kernel():
    """All four forward kernels with both S2 instantiations of the MFMA ones, and all three
    backward kernels, stand in the case table (each case is compared with the oracle)."""
    by_id = {r[0]: r for r in _K6_ROWS}
    fwd = {(r[7], r[8]) for r in _K6_ROWS} | {(e[2], by_id[e[0]][8] if e[2].startswith('mfma')
                                                else 0) for e in _K6_EXTRA}
    bwd = {r[9] for r in _K6_ROWS} | {e[3] for e in _K6_EXTRA}
    assert fwd == {('mfma_diag', 1), ('mfma_diag', 2), ('mfma', 1), ('mfma', 2), ('k1', 0),
                   ('generic', 0)}
    assert bwd == {'k1r', 'k1', 'elem'}
    # the bf16 instance of the generic forward and both large-LDS backward gates
    assert any(r[1] == torch.bfloat16 and r[7] == 'generic' for r in _K6_ROWS)
    assert any(r[10] is not None and 64 * 1024 < r[10] <= 96 * 1024 for r in _K6_ROWS)
