"""k1 (fused norm + modulation + activation) and k2 (bias + activation) on every host dispatch
path: vector widths 8 / 4 / 2 / 1, thread rows that do not divide the block, several channel
blocks with a tail, empty pixel rows, the two-stage statistics merge, the atomic and the
deterministic sum of the backward partials, HW == 1, N == 1, no affine, slopes 1 / 0.2 / 0.

Every case asserts, through the extension's read-only ``norm_plan`` / ``bias_act_plan``, that
its shape still reaches the path it is named for, then compares the kernels with the formula
written out in float64 (gradients by float64 autograd) at the tolerances of
``test_fused_norm_act`` / ``test_bias_act``.

GPU tests carry ``@gpu``; the two table / input sanity tests at the end run without a GPU.
"""
import pytest
import torch

gpu = pytest.mark.gpu
BF16, FP32 = torch.bfloat16, torch.float32
EPS = 1e-5


# ---- float64 reference --------------------------------------------------------------------
def _act(y, slope, mask=None):
    if slope == 1.0:
        return y
    if mask is None:
        mask = y > 0
    return torch.where(mask, y, y * slope)


def _ref_norm64(x, mode, w, b, gamma, beta, slope, rm=None, rv=None, mask=None):
    """act((x̂·w + b)·(1 + γ) + β) in float64; returns (out, pre-activation)."""
    C = x.shape[1]
    if mode == 'none':
        xh = x
    else:
        if mode == 'eval':
            mean, var = rm.reshape(1, C, 1, 1), rv.reshape(1, C, 1, 1)
        else:
            dims = (2, 3) if mode == 'instance' else (0, 2, 3)
            mean = x.mean(dims, keepdim=True)
            var = ((x - mean) ** 2).mean(dims, keepdim=True)
        xh = (x - mean) / torch.sqrt(var + EPS)
    y = xh
    if w is not None:
        y = y * w.reshape(1, C, 1, 1) + b.reshape(1, C, 1, 1)
    if gamma is not None:
        if gamma.dim() == 2:
            gamma, beta = gamma[:, :, None, None], beta[:, :, None, None]
        y = y * (1 + gamma) + beta
    return _act(y, slope, mask), y


def _leaf64(t, dtype=None):
    """float64 leaf of ``t`` as the kernel sees it (rounded to ``dtype`` first)."""
    if t is None:
        return None
    t = t.detach()
    if dtype is not None:
        t = t.to(dtype)
    return t.double().requires_grad_(True)


def _scale(t):
    return max(1.0, float(t.abs().max()))


def _close(got, ref, atol, rtol, name):
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), '%s: %d of %d off, max err %.3e (atol %.3e)' % (
        name, int(bad.sum()), bad.numel(), float(err.max()), atol)


# ---- case table ---------------------------------------------------------------------------
def _p_tpr3_zero_rows(p, N, C, HW):
    assert p['vec'] == 8 and p['tpr'] == 3 and p['rpb'] == 85
    assert HW < p['rpb']  # pixel rows with a zero count enter chan_merge


def _p_vec4_tpr3(p, N, C, HW):
    assert p['vec'] == 4 and p['tpr'] == 3


def _p_vec4(p, N, C, HW):
    assert p['vec'] == 4


def _p_vec2(p, N, C, HW):
    assert p['vec'] == 2


def _p_vec1_tpr3(p, N, C, HW):
    assert p['vec'] == 1 and p['tpr'] == 3


def _p_185(p, N, C, HW):
    assert p['vec'] == 1 and p['tpr'] == 185 and p['rpb'] == 1 and N == 1


def _p_1026(p, N, C, HW):
    assert p['vec'] == 2 and p['tpr'] == 256 and p['nzc'] == 3
    # channels the last channel block still covers: one thread's worth
    assert C - (p['nzc'] - 1) * p['tpr'] * p['vec'] == p['vec']


def _p_two_stage(p, N, C, HW):
    # (rs_stats is asserted for batch and for instance statistics by the caller)
    assert p['P'] >= 32 and p['rs_bwd'] > 1
    assert HW - (p['P'] - 1) * p['chunk'] < p['chunk']  # short last chunk


def _p_512(p, N, C, HW):
    _p_two_stage(p, N, C, HW)
    assert HW - (p['P'] - 1) * p['chunk'] == 1  # last chunk of one pixel


def _p_nchw_vec1_small(p, N, C, HW):
    assert p['vec'] == 1 and HW < 256


def _p_nchw_91(p, N, C, HW):
    assert p['vec'] == 1
    _p_two_stage(p, N, C, HW)


def _p_nchw_vec4_big(p, N, C, HW):
    assert p['vec'] == 4 and p['P'] >= 32


def _p_hw1(p, N, C, HW):
    assert HW == 1


# (layout, (N, C, H, W), dtype, property); both statistics kinds must take the two-stage merge
# on the rows flagged in _TWO_STAGE
_ROWS = [
    ('cl', (2, 24, 7, 5), BF16, _p_tpr3_zero_rows),
    ('cl', (2, 12, 7, 5), BF16, _p_vec4_tpr3),
    ('cl', (2, 12, 7, 5), FP32, _p_vec4_tpr3),
    ('cl', (2, 6, 5, 9), BF16, _p_vec2),
    ('cl', (2, 6, 5, 9), FP32, _p_vec2),
    ('cl', (2, 3, 9, 11), BF16, _p_vec1_tpr3),
    ('cl', (2, 3, 9, 11), FP32, _p_vec1_tpr3),
    ('cl', (1, 185, 6, 7), BF16, _p_185),
    ('cl', (1, 185, 6, 7), FP32, _p_185),
    ('cl', (1, 1026, 3, 5), BF16, _p_1026),
    ('cl', (1, 1026, 3, 5), FP32, _p_1026),
    ('cl', (2, 512, 23, 23), BF16, _p_512),
    ('cl', (2, 512, 23, 23), FP32, _p_512),
    ('nchw', (2, 5, 7, 9), BF16, _p_nchw_vec1_small),
    ('nchw', (2, 5, 7, 9), FP32, _p_nchw_vec1_small),
    ('nchw', (2, 3, 6, 7), BF16, _p_vec2),
    ('nchw', (2, 3, 6, 7), FP32, _p_vec2),
    ('nchw', (1, 4, 6, 6), BF16, _p_vec4),
    ('nchw', (1, 2, 91, 91), FP32, _p_nchw_91),
    ('nchw', (1, 2, 128, 256), FP32, _p_nchw_vec4_big),
    ('nchw', (4, 32, 1, 1), BF16, _p_hw1),
    ('nchw', (4, 32, 1, 1), FP32, _p_hw1),
]
_TWO_STAGE = (_p_512, _p_nchw_91)
_MODES = ['batch', 'instance', 'none', 'eval']
_MODS = [None, 'spatial', 'gb', 'bcast']
_SLOPES = [1.0, 0.2, 0.0]


def _cases():
    """Every row with every mode; modulation, slope and affine rotate with the row so that each
    value of each axis meets both layouts without the full product."""
    out = []
    for i, (layout, shape, dtype, prop) in enumerate(_ROWS):
        for k, mode in enumerate(_MODES):
            if mode == 'instance' and shape[2] * shape[3] == 1:
                continue  # the variance of one pixel is 0: batch and 'none' modes only
            mod = _MODS[(i + k) % 4]
            slope = _SLOPES[(i + 2 * k) % 3]
            affine = (i + k // 2 + k) % 2 == 0
            out.append(pytest.param(
                i, mode, mod, slope, affine,
                id='%s-%s-%s-%s-%s-s%g-%s' % (
                    layout, 'x'.join(map(str, shape)), 'bf16' if dtype == BF16 else 'fp32', mode,
                    mod, slope, 'affine' if affine else 'plain')))
    return out


def _make_x(layout, shape, dtype, gen_seed):
    torch.manual_seed(gen_seed)
    x = (torch.randn(*shape, device='cuda') * 2 + 0.5).to(dtype)
    if layout == 'cl':
        x = x.contiguous(memory_format=torch.channels_last)
    return x


def _make_mod(mod, layout, shape, dtype):
    N, C, H, W = shape
    gamma = beta = gb = None
    cl = layout == 'cl'
    if mod == 'spatial':
        gamma = (torch.randn(N, C, H, W, device='cuda') * 0.3).to(dtype)
        beta = (torch.randn(N, C, H, W, device='cuda') * 0.3).to(dtype)
        if cl:
            gamma = gamma.contiguous(memory_format=torch.channels_last)
            beta = beta.contiguous(memory_format=torch.channels_last)
    elif mod == 'gb':
        gb = (torch.randn(N, 2 * C, H, W, device='cuda') * 0.3).to(dtype)
        if cl:
            gb = gb.contiguous(memory_format=torch.channels_last)
    elif mod == 'bcast':
        gamma = torch.randn(N, C, device='cuda') * 0.3
        beta = torch.randn(N, C, device='cuda') * 0.3
    return gamma, beta, gb


def _run_and_check(x, mode, mod, slope, affine, layout):
    """Forward + backward of fused_norm_act against the float64 formula; returns the gradients
    (dx, dw) of the kernel run."""
    from imaginaire_amd.ops.norm import fused_norm_act
    dtype = x.dtype
    shape = tuple(x.shape)
    N, C, H, W = shape
    w = b = rm = rv = None
    if affine:
        w = torch.randn(C, device='cuda') * 0.5 + 1
        b = torch.randn(C, device='cuda') * 0.1
    if mode == 'eval':
        rm = torch.randn(C, device='cuda') * 0.5 + 0.3
        rv = torch.rand(C, device='cuda') * 3 + 1
    gamma, beta, gb = _make_mod(mod, layout, shape, dtype)
    x = x.detach().clone(memory_format=torch.preserve_format)
    leaves = [t for t in (x, w, b, gamma, beta, gb) if t is not None]
    for t in leaves:
        t.requires_grad_(True)
    rm0, rv0 = (rm.clone(), rv.clone()) if rm is not None else (None, None)
    y = fused_norm_act(x, 'batch' if mode == 'eval' else mode, w, b, gamma=gamma, beta=beta,
                       gb=gb, running_mean=rm, running_var=rv, training=mode != 'eval',
                       momentum=0.0, eps=EPS, slope=slope)
    assert y.shape == x.shape and y.dtype == dtype
    if rm is not None:  # eval mode leaves the running statistics alone
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)

    g_gamma, g_beta = (gb[:, :C], gb[:, C:]) if gb is not None else (gamma, beta)
    xr, wr, br = _leaf64(x), _leaf64(w), _leaf64(b)
    # the op applies the modulation in the activation dtype: round like it does
    gr, ber = _leaf64(g_gamma, dtype), _leaf64(g_beta, dtype)
    rm64 = rm.double() if rm is not None else None
    rv64 = rv.double() if rv is not None else None
    yr, pre = _ref_norm64(xr, mode, wr, br, gr, ber, slope, rm64, rv64)
    if dtype == BF16 and slope != 1.0:
        # bf16 sign ties of a pre-activation within a rounding of 0: activation mask from the
        # kernel's own output, and the masks may differ on isolated elements only
        mask = y.detach() > 0
        differ = float((mask != (pre.detach() > 0)).double().mean())
        assert differ <= 0.01, differ
        yr, pre = _ref_norm64(xr, mode, wr, br, gr, ber, slope, rm64, rv64, mask=mask)
    tol = 2e-2 if dtype == BF16 else 1e-4
    _close(y, yr.detach(), tol * 5, tol, 'y')

    go = torch.randn_like(yr).to(dtype)
    y.backward(go)
    yr.backward(go.double())
    _close(x.grad, xr.grad, tol * 5 * _scale(xr.grad), tol * 5, 'dx')
    if affine:
        assert w.grad.dtype == w.dtype and b.grad.dtype == b.dtype
        _close(w.grad, wr.grad, tol * 20 * _scale(wr.grad), tol * 5, 'dw')
        _close(b.grad, br.grad, tol * 20 * _scale(br.grad), tol * 5, 'db')
    if gb is not None:
        dgb = torch.cat([gr.grad, ber.grad], 1)
        _close(gb.grad, dgb, tol * 5 * _scale(dgb), tol * 5, 'dgb')
    elif gamma is not None:
        _close(gamma.grad, gr.grad.reshape(gamma.shape), tol * 20 * _scale(gr.grad), tol * 5,
               'dgamma')
        _close(beta.grad, ber.grad.reshape(beta.shape), tol * 20 * _scale(ber.grad), tol * 5,
               'dbeta')
    return x.grad, (w.grad if affine else None)


def _plan(x, per_instance=False):
    from imaginaire_amd.ops import _ext
    return dict(_ext.ext().norm_plan(x, per_instance))


@gpu
@pytest.mark.parametrize('row,mode,mod,slope,affine', _cases())
def test_norm_dispatch_paths(row, mode, mod, slope, affine):
    layout, shape, dtype, prop = _ROWS[row]
    x = _make_x(layout, shape, dtype, 100 + row)
    N, C, H, W = shape
    p = _plan(x, mode == 'instance')
    assert p['cl'] == (layout == 'cl')
    prop(p, N, C, H * W)
    if prop in _TWO_STAGE:
        assert _plan(x, False)['rs_stats'] > 1 and _plan(x, True)['rs_stats'] > 1
    _run_and_check(x, mode, mod, slope, affine, layout)


# ---- running statistics through the second merge stage -----------------------------------
@gpu
@pytest.mark.parametrize('dtype', [FP32, BF16])
def test_running_stats_two_stage_merge(dtype):
    from imaginaire_amd.ops.norm import fused_norm_act
    x = _make_x('cl', (2, 512, 23, 23), dtype, 7)
    C = x.shape[1]
    assert _plan(x)['rs_stats'] > 1
    rm = torch.randn(C, device='cuda')
    rv = torch.rand(C, device='cuda') * 2 + 0.5
    nb = torch.tensor([5], device='cuda', dtype=torch.int64)
    rm0, rv0 = rm.double(), rv.double()
    y = fused_norm_act(x, 'batch', running_mean=rm, running_var=rv, training=True, momentum=0.1,
                       eps=EPS, slope=1.0, num_batches=nb)
    x64 = x.double()
    n = x64.numel() // C
    mean = x64.mean((0, 2, 3))
    var = ((x64 - mean.reshape(1, C, 1, 1)) ** 2).mean((0, 2, 3))
    _close(rm, 0.9 * rm0 + 0.1 * mean, 1e-3, 1e-3, 'running_mean')
    _close(rv, 0.9 * rv0 + 0.1 * var * n / (n - 1), 1e-3, 1e-3, 'running_var')
    assert int(nb) == 6
    yr, _ = _ref_norm64(x64, 'batch', None, None, None, None, 1.0)
    tol = 2e-2 if dtype == BF16 else 1e-4
    _close(y, yr, tol * 5, tol, 'y')


# ---- ill-conditioned statistics -----------------------------------------------------------
_ILL_SHAPE = (2, 5, 91, 91)


def _ill_input(mean, std, device):
    g = torch.Generator(device='cpu').manual_seed(11)
    return (mean + std * torch.randn(*_ILL_SHAPE, generator=g)).to(device)


@gpu
@pytest.mark.parametrize('per_instance', [False, True])
@pytest.mark.parametrize('layout', ['cl', 'nchw'])
def test_stats_ill_conditioned(layout, per_instance):
    """mean 100, std 0.01 in fp32: the shifted sums + Chan merge must keep the mean to 4 ulp of
    100 and the variance to 1e-4 relative, where a one-pass E[x²] - E[x]² is off by ~10x (see
    test_ill_conditioned_input_separates_formulas)."""
    from imaginaire_amd.ops import _ext
    x = _ill_input(100.0, 0.01, 'cuda')
    if layout == 'cl':
        x = x.contiguous(memory_format=torch.channels_last)
    assert _plan(x, per_instance)['rs_stats'] > 1
    cnt, mean, var = _ext.ext().norm_stats(x, per_instance, EPS, None, None, False)[:3]
    dims = (2, 3) if per_instance else (0, 2, 3)
    x64 = x.double()
    mean64 = x64.mean(dims, keepdim=True)
    var64 = ((x64 - mean64) ** 2).mean(dims).reshape(-1, 5)
    mean64 = mean64.reshape(-1, 5)
    assert cnt.shape == mean.shape == var.shape == mean64.shape
    assert torch.equal(cnt.double(), torch.full_like(mean64, x64.numel() / mean64.numel()))
    emean = float((mean.double() - mean64).abs().max())
    evar = float(((var.double() - var64).abs() / var64).max())
    print('ill-conditioned %s inst=%d: |dmean| %.3e, rel dvar %.3e' % (
        layout, per_instance, emean, evar))
    assert emean <= 3e-5, emean
    assert evar <= 1e-4, evar


@gpu
@pytest.mark.parametrize('mode', ['batch', 'instance'])
@pytest.mark.parametrize('layout', ['cl', 'nchw'])
def test_forward_large_mean(layout, mode):
    """End to end at mean 30, std 0.1 (fp32, the ordinary tolerance)."""
    from imaginaire_amd.ops.norm import fused_norm_act
    x = _ill_input(30.0, 0.1, 'cuda')
    if layout == 'cl':
        x = x.contiguous(memory_format=torch.channels_last)
    y = fused_norm_act(x, mode, training=True, momentum=0.0, eps=EPS, slope=1.0)
    yr, _ = _ref_norm64(x.double(), mode, None, None, None, None, 1.0)
    _close(y, yr, 5e-4, 1e-4, 'y')


# ---- deterministic mode -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('dtype', [FP32, BF16])
def test_deterministic_backward_single_split(dtype):
    x = _make_x('cl', (2, 512, 23, 23), dtype, 21)
    assert _plan(x)['rs_bwd'] > 1
    was = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        assert _plan(x)['rs_bwd'] == 1
        torch.manual_seed(22)
        dx1, dw1 = _run_and_check(x, 'batch', 'bcast', 0.2, True, 'cl')
        torch.manual_seed(22)
        dx2, dw2 = _run_and_check(x, 'batch', 'bcast', 0.2, True, 'cl')
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert torch.equal(dx1, dx2) and torch.equal(dw1, dw2)


# ---- sync_stats_merge, one process --------------------------------------------------------
@gpu
@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('counts', [(35, 0, 1), (0, 1, 0)])
def test_sync_stats_merge_unequal_counts(counts, affine):
    """Fabricated per-rank (count, mean, var) rows with unequal counts, an empty rank and a
    one-sample rank; C = 300 spans two 256-thread blocks with a tail."""
    from imaginaire_amd.ops import _ext
    torch.manual_seed(5)
    Wn, C = len(counts), 300
    allst = torch.empty(Wn, 3, C, device='cuda')
    for r, n in enumerate(counts):
        allst[r, 0] = float(n)
        allst[r, 1] = torch.randn(C, device='cuda') * 0.5
        # biased variance of n samples: 0 for one sample; an empty rank's rows must be ignored
        allst[r, 2] = 0.0 if n == 1 else torch.rand(C, device='cuda') + 0.5
    w = (torch.randn(C, device='cuda') * 0.1 + 1) if affine else None
    b = (torch.randn(C, device='cuda') * 0.1) if affine else None
    rm = torch.randn(C, device='cuda')
    rv = torch.rand(C, device='cuda') + 0.5
    nb = torch.tensor([41], device='cuda', dtype=torch.int64)
    rm0, rv0 = rm.double(), rv.double()
    a64 = allst.double()
    outs = _ext.ext().sync_stats_merge(allst, EPS, w, b, rm, rv, nb, 0.1)
    n_i, m_i, v_i = a64[:, 0], a64[:, 1], a64[:, 2]
    n = n_i.sum(0)
    mean = (n_i * m_i).sum(0) / n
    var = (n_i * (v_i + (m_i - mean) ** 2)).sum(0) / n
    rstd = 1 / torch.sqrt(var + EPS)
    a = w.double() if affine else torch.ones_like(mean)
    sh = b.double() if affine else torch.zeros_like(mean)
    ref = (n, mean, var, rstd, rstd * a, sh - mean * rstd * a)
    for got, want, name in zip(outs, ref, ('count', 'mean', 'var', 'rstd', 'scale', 'shift')):
        assert got.shape == (1, C) and got.dtype == FP32
        _close(got.reshape(-1), want, 1e-6, 1e-5, name)
    unb = var * n / (n - 1).clamp_min(1)
    _close(rm, 0.9 * rm0 + 0.1 * mean, 1e-6, 1e-5, 'running_mean')
    _close(rv, 0.9 * rv0 + 0.1 * unb, 1e-6, 1e-5, 'running_var')
    assert int(nb) == 42
    # without running statistics nothing but the outputs is written
    outs2 = _ext.ext().sync_stats_merge(allst, EPS, w, b)
    for g1, g2 in zip(outs, outs2):
        assert torch.equal(g1, g2)
    assert int(nb) == 42


# ---- k2: bias + activation ----------------------------------------------------------------
def _b_tpr3(p):
    assert p['tpr'] == 3


def _b_vec1(p):
    assert p['vec'] == 1


def _b_vec2(p):
    assert p['vec'] == 2


def _b_nzc3(p):
    assert p['nzc'] == 3


_BA_ROWS = [
    ('cl', (2, 24, 5, 7), (BF16,), _b_tpr3),
    ('cl', (2, 3, 9, 11), (BF16, FP32), _b_vec1),
    ('cl', (1, 185, 6, 7), (BF16, FP32), _b_vec1),
    ('cl', (1, 1026, 3, 5), (BF16, FP32), _b_nzc3),
    ('cl', (2, 6, 5, 9), (BF16, FP32), _b_vec2),
    ('linear', (5, 10), (BF16, FP32), _b_vec2),
    ('linear', (3, 7), (BF16, FP32), _b_vec1),
    ('nchw', (2, 5, 7, 9), (BF16, FP32), _b_vec1),
    ('nchw', (2, 3, 6, 7), (BF16, FP32), _b_vec2),
    # 2x64x48x48 fills its last block exactly (4608 rows = 36 x 128 = 72 x 64): one image row
    # less leaves a short one; 2x64x9x11 is the smallest such shape (two blocks)
    ('cl', (2, 64, 47, 48), (BF16, FP32), None),
    ('cl', (2, 64, 9, 11), (BF16, FP32), None),
]


def _ba_cases():
    out = []
    for i, (layout, shape, dtypes, _) in enumerate(_BA_ROWS):
        for dtype in dtypes:
            for slope in (0.2, 0.0, 1.0):
                out.append(pytest.param(i, dtype, slope, id='%s-%s-%s-s%g' % (
                    layout, 'x'.join(map(str, shape)), 'bf16' if dtype == BF16 else 'fp32',
                    slope)))
    return out


def _ba_input(layout, shape, dtype, seed=1):
    torch.manual_seed(seed)
    x = torch.randn(*shape, device='cuda').to(dtype)
    if layout == 'cl':
        x = x.contiguous(memory_format=torch.channels_last)
    b = torch.randn(shape[1], device='cuda')
    go = torch.randn(*shape, device='cuda').to(dtype)
    return x, b, go


def _ba_plan(x, slope):
    from imaginaire_amd.ops import _ext
    return dict(_ext.ext().bias_act_plan(x, slope))


def _ba_run(x, b, go, slope, check=True):
    from imaginaire_amd.ops.bias_act import bias_act
    dtype = x.dtype
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    b = b.detach().clone().requires_grad_(True) if b is not None else None
    y = bias_act(x, b, slope)
    y.backward(go)
    if check:
        xr, br = _leaf64(x), _leaf64(b)
        pre = xr
        if br is not None:
            pre = xr + br.reshape([1, -1] + [1] * (x.dim() - 2))
        yr = _act(pre, slope)
        yr.backward(go.double())
        tol = 2e-2 if dtype == BF16 else 1e-5
        _close(y.detach(), yr.detach(), tol, tol, 'y')
        _close(x.grad, xr.grad, tol * 2, tol * 2, 'dx')
        if b is not None:
            assert b.grad.dtype == b.dtype
            _close(b.grad, br.grad, tol * 50, tol * 5, 'db')
    return x.grad, (b.grad if b is not None else None)


@gpu
@pytest.mark.parametrize('row,dtype,slope', _ba_cases())
def test_bias_act_dispatch_paths(row, dtype, slope, monkeypatch):
    monkeypatch.delenv('IMAGINAIRE_AMD_BIASACT_UNROLL', raising=False)
    layout, shape, _, prop = _BA_ROWS[row]
    x, b, go = _ba_input(layout, shape, dtype)
    p = _ba_plan(x, slope)
    if prop is not None:
        prop(p)
    else:
        rows = x.numel() // shape[1]
        assert p['P'] > 1 and rows > p['rows_per_block']
        assert 0 < rows - (p['P'] - 1) * p['rows_per_block'] < p['rows_per_block']
    dx, _ = _ba_run(x, b, go, slope)
    if slope == 1.0:
        if layout != 'nchw':  # identity on a channels-fast input: the bias-only kernel
            assert p['act'] is False and p['unroll'] is True
        assert torch.equal(dx, go)
    elif layout != 'nchw':
        assert p['act'] is True and p['unroll'] is False


@gpu
@pytest.mark.parametrize('layout,shape', [('cl', (2, 6, 5, 9)), ('nchw', (2, 5, 7, 9)),
                                          ('linear', (5, 10))])
@pytest.mark.parametrize('dtype', [BF16, FP32])
def test_bias_act_without_bias(layout, shape, dtype):
    x, _, go = _ba_input(layout, shape, dtype, seed=2)
    _ba_run(x, None, go, 0.2)


@gpu
@pytest.mark.parametrize('layout,shape,dtype', [('cl', (2, 64, 47, 48), BF16),
                                                ('cl', (2, 24, 5, 7), BF16),
                                                ('cl', (2, 64, 47, 48), FP32),
                                                ('linear', (5, 10), FP32)])
@pytest.mark.parametrize('slope', [0.2, 1.0])
def test_bias_act_unroll_variants_agree(layout, shape, dtype, slope, monkeypatch):
    """IMAGINAIRE_AMD_BIASACT_UNROLL = 1 / 4 with and without an activation: the four
    (ACT, U) kernels. Same dx; db equal within the fp32 tolerance (another summation order)."""
    x, b, go = _ba_input(layout, shape, dtype, seed=3)
    res = {}
    for u in ('1', '4'):
        monkeypatch.setenv('IMAGINAIRE_AMD_BIASACT_UNROLL', u)
        p = _ba_plan(x, slope)  # the variable is read on every call
        assert p['act'] is (slope != 1.0) and p['unroll'] is (u == '4')
        res[u] = _ba_run(x, b, go, slope)
    assert torch.equal(res['1'][0], res['4'][0])
    _close(res['4'][1], res['1'][1], 1e-5 * 50, 1e-5 * 5, 'db')


# ---- no GPU needed ------------------------------------------------------------------------
def test_case_table_covers_every_axis():
    """Each value of each axis of the k1 cross meets a channels-last and an NCHW row, and the
    two-stage rows run batch and instance statistics."""
    seen = {}
    for c in _cases():
        row, mode, mod, slope, affine = c.values
        layout, shape, dtype, prop = _ROWS[row]
        for axis, v in (('mode', mode), ('mod', mod), ('slope', slope), ('affine', affine),
                        ('dtype', dtype)):
            seen.setdefault((axis, v), set()).add(layout)
        if prop in _TWO_STAGE:
            seen.setdefault(('two_stage', row), set()).add(mode)
    for key, layouts in seen.items():
        if key[0] == 'two_stage':
            assert {'batch', 'instance'} <= layouts, key
        else:
            assert layouts == {'cl', 'nchw'}, (key, layouts)
    axes = {k for k in seen if k[0] != 'two_stage'}
    assert len(axes) == len(_MODES) + len(_MODS) + len(_SLOPES) + 2 + 2
    assert sum(1 for k in seen if k[0] == 'two_stage') == 3


def test_ill_conditioned_input_separates_formulas():
    """The input of test_stats_ill_conditioned keeps its teeth: against float64 of the same fp32
    values, a robust fp32 variance (torch.var_mean) is orders of magnitude inside the 1e-4 bound
    and the one-pass E[x²] - E[x]² in fp32 is orders of magnitude outside it."""
    x = _ill_input(100.0, 0.01, 'cpu')
    x64 = x.double()
    mean64 = x64.mean((0, 2, 3), keepdim=True)
    var64 = ((x64 - mean64) ** 2).mean((0, 2, 3))
    var32, mean32 = torch.var_mean(x, (0, 2, 3), unbiased=False)
    robust = float(((var32.double() - var64).abs() / var64).max())
    naive_var = (x * x).mean((0, 2, 3)) - x.mean((0, 2, 3)) ** 2
    naive = float(((naive_var.double() - var64).abs() / var64).min())
    assert robust <= 1e-6, robust
    assert naive >= 1e-2, naive
    assert float((mean32.double() - mean64.reshape(-1)).abs().max()) <= 3e-5
