"""``mt_fromage`` / ``mt_madam`` (``csrc/multi_tensor.hip``) and ``FusedFromage`` / ``FusedMadam``
on the GPU.

Raw kernels: every step is compared with the update written out in float64 FROM THE KERNEL'S OWN
fp32 STATE before that step (parameters, ``exp_avg_sq``, device ``[step, max]``, the gradient as
rounded to its dtype, the learning rate as rounded to fp32), over tensors of 1, 3, 37, kChunk - 1,
kChunk, kChunk + 1, 2 kChunk + 3 and 70001 elements with an empty tensor in the middle of every
list: fp32 and bf16 gradients, the host and the device learning rate (changed between steps),
exactly one operand misaligned (scalar path), a channels-last 4-D parameter, a bf16 shadow on some
parameters only (bitwise ``p.to(bfloat16)`` after every step), and the gaps between the carved
operands untouched. Fromage: neighbouring tensors three decades apart in magnitude (a partial
credited to the wrong tensor moves the ratio by orders of magnitude), an all-zero gradient and an
all-zero parameter. Madam: g = 0 at step 1 (0 / 0 -> 0), p = 0 stays 0, ``g_bound`` None and 0.5,
and a case whose ±max clamp bites on part of a multi-chunk tensor.

Tolerance: ``ADAM_ATOL, ADAM_RTOL = 1e-6, 1e-5`` against float64, as for ``mt_adam``. Where the
Python class itself (fp32, same device, same inputs, one step from the same state) is further than
that from the same oracle, twice ITS deviation is allowed instead: that is the rounding of the
reference's own fp32 arithmetic, not of the kernel (``_bound_factor``; the figures are printed by
every case and recorded in the docstrings of the tests they concern).

Then: two runs from one state are bitwise equal; a captured step (2 eager warm-ups on a side
stream, 3 replays, a learning-rate change through ``sync_hyper`` in between) is bitwise the eager
fused step and within the tolerance of the Python class; the SPADE trainer with ``fromage`` /
``madam`` optimizers is captured and keeps every bf16 shadow in step with its weight. The
control "capturing the Python ``Fromage`` raises" is not run here: it would leave a failed capture
behind in a process the rest of the suite shares; ``GraphedStep``'s message on such a step
("capture ... failed ...; running eagerly") is what the Python class gives.
"""
import functools
import os

import pytest
import torch

gpu = pytest.mark.gpu
BF16, FP32 = torch.bfloat16, torch.float32
K_CHUNK = 16384  # kChunk of multi_tensor.hip
SIZES = (1, 3, 37, K_CHUNK - 1, K_CHUNK, K_CHUNK + 1, 2 * K_CHUNK + 3, 70001)
EMPTY_AT = 4  # every list also holds one numel == 0 tensor here
ALL_SIZES = list(SIZES[:EMPTY_AT]) + [0] + list(SIZES[EMPTY_AT:])
MULTI_CHUNK = ALL_SIZES.index(2 * K_CHUNK + 3)
SENTINEL = 768.0  # (exact in bf16)
ADAM_ATOL, ADAM_RTOL = 1e-6, 1e-5  # those of test_multi_tensor_paths_gpu
STEPS = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _X():
    from imaginaire_amd.ops import _ext
    return _ext.ext()


def _f32(x):
    """A Python float as the kernels receive it."""
    return float(torch.tensor(x, dtype=FP32))


def _ratio(got, ref):
    """max |got - ref| / (atol + rtol |ref|) at the Adam tolerance (inf for a NaN)."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    r = (got - ref).abs() / (ADAM_ATOL + ADAM_RTOL * ref.abs())
    return float('inf') if bool(torch.isnan(r).any()) else float(r.max())


def _bound_factor(py_ratio):
    """1 (the Adam tolerance as it is) unless the Python class is itself further than that from
    the float64 oracle; then twice its deviation."""
    return max(1.0, 2.0 * py_ratio)


# ---- operands carved from one flat buffer (as in test_multi_tensor_paths_gpu) --------------
def _carve(sizes, dtype, offsets=0, device='cuda', modulo=16):
    """1-D views of one sentinel-filled flat buffer, view ``i`` starting ``offsets[i]`` bytes
    past a multiple of ``modulo`` bytes (asserted on ``data_ptr``). Returns (buffer, views)."""
    item = torch.empty(0, dtype=dtype).element_size()
    if isinstance(offsets, int):
        offsets = [offsets] * len(sizes)
    per = modulo // item
    total = sum((n + per - 1) // per * per + 2 * per for n in sizes) + per
    buf = torch.full((total,), SENTINEL, dtype=dtype, device=device)
    assert buf.data_ptr() % modulo == 0
    views, cur = [], per
    for n, off in zip(sizes, offsets):
        assert off % item == 0 and 0 <= off < modulo
        start = cur + off // item
        v = buf.narrow(0, start, n)
        if n:
            assert v.data_ptr() % modulo == off, (n, off, v.data_ptr() % modulo)
        views.append(v)
        cur = (start + n + per - 1) // per * per + per
    assert cur <= total
    return buf, views


def _gaps_untouched(buf, views, name):
    used = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    item = buf.element_size()
    for v in views:
        if v.numel():
            s = (v.data_ptr() - buf.data_ptr()) // item
            used[s:s + v.numel()] = True
    rest = buf[~used].float()
    assert bool((rest == SENTINEL).all()), '%s: wrote outside its operands' % name


HAS_SHADOW = [i % 3 != 1 and n > 0 for i, n in enumerate(ALL_SIZES)]


def _operands(p0, gdt, offs, with_v):
    """Carved p / g / (v) / shadow; offs: {'p' | 'g' | 'v' | 's': byte offset}."""
    bufs = {}
    kinds = [('p', FP32), ('g', gdt)] + ([('v', FP32)] if with_v else [])
    for key, dt in kinds:
        bufs[key] = _carve(ALL_SIZES, dt, offs.get(key, 0), modulo=16 if dt is FP32 else 8)
    bufs['s'] = _carve([n if h else 0 for n, h in zip(ALL_SIZES, HAS_SHADOW)], BF16,
                       offs.get('s', 0), modulo=8)
    for t, src in zip(bufs['p'][1], p0):
        t.copy_(src)
    if with_v:
        for t in bufs['v'][1]:
            t.zero_()
    for key, (_, views) in bufs.items():
        mod = 16 if views[0].dtype is FP32 else 8
        for t in views:
            if t.numel():
                assert t.data_ptr() % mod == offs.get(key, 0)
    return bufs


def _check_gaps_and_shadows(bufs, step, name):
    ps, ss = bufs['p'][1], bufs['s'][1]
    for i, (s, p) in enumerate(zip(ss, ps)):
        if HAS_SHADOW[i]:
            assert torch.equal(s, p.to(BF16)), '%s step %d shadow %d' % (name, step, i)
    for key, (buf, views) in bufs.items():
        _gaps_untouched(buf, views, '%s %s' % (name, key))


# ---- Fromage ---------------------------------------------------------------------------------
F_ZERO_GRAD, F_ZERO_PARAM = 2, 1  # indices into ALL_SIZES (37 and 3 elements)
F_LRS = (1e-2, 1e-2, 5e-3)  # rewritten before step 3


def _f_mag(i):
    return 1e3 if i % 2 == 0 else 1e-3  # neighbours three decades apart


@functools.lru_cache(maxsize=2)
def _fromage_case(gdt):
    """CPU inputs, never modified: p0 [tensor] fp32, grads [step][tensor] in the gradient dtype.
    Parameter and gradient of tensor i both carry the magnitude ``_f_mag(i)``."""
    gen = torch.Generator().manual_seed(4321)
    p0 = [torch.randn(n, generator=gen) * _f_mag(i) for i, n in enumerate(ALL_SIZES)]
    p0[F_ZERO_PARAM].zero_()
    grads = []
    for _ in range(STEPS):
        gs = [(torch.randn(n, generator=gen) * _f_mag(i)).to(gdt) for i, n in enumerate(ALL_SIZES)]
        gs[F_ZERO_GRAD].zero_()
        grads.append(gs)
    return p0, grads


def _fromage64(p, g, lr):
    """One Fromage step in float64 on the fp32 values the kernel was given."""
    p, g = p.double(), g.double()
    pn, gn = float(p.pow(2).sum().sqrt()), float(g.pow(2).sum().sqrt())
    ratio = pn / gn if (pn > 0 and gn > 0) else 1.0
    return (p - lr * ratio * g) / (1 + lr * lr) ** 0.5


def _fromage_python(p, g, lr):
    """The Python class, fp32, on the device, one step from the same state."""
    from imaginaire_amd.optimizers import Fromage
    q = torch.nn.Parameter(p.detach().clone().contiguous())
    q.grad = g.detach().float().reshape(q.shape).contiguous()
    Fromage([q], lr=lr).step()
    return q.detach()


def _run_fromage(gdt, path, offs, name):
    p0, grads = _fromage_case(gdt)
    bufs = _operands(p0, gdt, offs, with_v=False)
    ps, gs_, ss = bufs['p'][1], bufs['g'][1], bufs['s'][1]
    X = _X()
    hyper = torch.tensor([F_LRS[0]], dtype=FP32, device='cuda') if path == 'hyper' else None
    worst, worst_py = 0.0, 0.0
    for k in range(STEPS):
        lr = _f32(F_LRS[k])
        before = [p.detach().clone() for p in ps]
        for g_dev, g in zip(gs_, grads[k]):
            g_dev.copy_(g)
        if hyper is not None:
            hyper.fill_(F_LRS[k])
            X.mt_fromage(ps, gs_, ss, 123.0, hyper)  # (the host lr is ignored on this path)
        else:
            X.mt_fromage(ps, gs_, ss, F_LRS[k], None)
        torch.cuda.synchronize()
        if k == 0:
            assert float(before[F_ZERO_PARAM].abs().sum()) == 0  # the zero-|p| branch ran
        assert float(gs_[F_ZERO_GRAD].float().abs().sum()) == 0  # the zero-|g| branch ran
        for i, p in enumerate(ps):
            ref = _fromage64(before[i].cpu(), grads[k][i], lr)
            py = _ratio(_fromage_python(before[i], gs_[i], F_LRS[k]), ref)
            got = _ratio(p, ref)
            worst, worst_py = max(worst, got), max(worst_py, py)
            assert got <= _bound_factor(py), \
                '%s step %d p[%d, n=%d]: err / bound %.3f, Python class %.3f' % (
                    name, k + 1, i, p.numel(), got, py)
        _check_gaps_and_shadows(bufs, k + 1, name)
    print('%s: max err / Adam bound: kernel %.3f, Python Fromage %.3f' % (name, worst, worst_py))
    return bufs


_F_ALIGNED = [(gdt, path) for gdt in ('fp32', 'bf16') for path in ('hyper', 'host')]
_F_MISALIGNED = [('fp32', {'p': 4}), ('fp32', {'g': 12}), ('bf16', {'g': 2}), ('fp32', {'s': 6}),
                 ('bf16', {'p': 8})]
_DT = {'fp32': FP32, 'bf16': BF16}


@gpu
@pytest.mark.parametrize('gdt,path', _F_ALIGNED)
def test_fromage_vector_body(gdt, path):
    """All operands aligned: the 16-byte body and its 1..3 element tail, tensors of several
    chunks, the per-tensor reduce with neighbours x1e3 / x1e-3, both zero-norm branches.

    Measured (MI355X), max err / Adam bound over all tensors and steps: kernel 0.546 (fp32
    gradients) and 0.707 (bf16); the Python ``Fromage`` 0.946 and 1.174 on the same inputs, i.e.
    the reference's own fp32 rounding is past the Adam bound in the bf16 case (on the x1e3
    tensors, where an element that lands near 0 carries the rounding of a step of size ~10)."""
    _run_fromage(_DT[gdt], path, {}, 'fromage-%s-%s' % (gdt, path))


@gpu
@pytest.mark.parametrize('gdt,offs', _F_MISALIGNED,
                         ids=['%s-%s+%d' % (g, *list(o.items())[0]) for g, o in _F_MISALIGNED])
def test_fromage_one_operand_misaligned(gdt, offs):
    """Exactly one of p / g / shadow off the vector alignment: the scalar path.

    Measured (MI355X), max err / Adam bound: kernel 0.586 with fp32 gradients (Python ``Fromage``
    0.946) and 1.079 with bf16 gradients (cases bf16-g+2 and bf16-p+8; Python ``Fromage`` 1.174,
    so 2.35 is allowed there): the one place where the Adam tolerance as it stands is missed, by
    the kernel and by the reference alike."""
    path = 'hyper' if 'g' in offs else 'host'
    _run_fromage(_DT[gdt], path, offs, 'fromage-%s-%s' % (gdt, offs))


def _cl_strides(shape):
    n, c, h, w = shape
    return (c * h * w, 1, w * c, c)


_CL_SHAPES = [(5, 6, 3, 3), (3, 5, 7, 11), (0,), (16, 2, 1, 1), (37,)]


def _cl_dev(t, dtype):
    if t.dim() == 4:
        return torch.empty_strided(t.shape, _cl_strides(t.shape), dtype=dtype, device='cuda')
    return torch.empty(t.shape, dtype=dtype, device='cuda')


@gpu
@pytest.mark.parametrize('gdt', ['fp32', 'bf16'])
def test_fromage_channels_last(gdt):
    """Channels-last 4-D parameters with gradient and shadow in the parameter's strides (the
    norms are order-independent up to rounding, the update elementwise in memory order)."""
    dt = _DT[gdt]
    gen = torch.Generator().manual_seed(77)
    p0 = [torch.randn(s, generator=gen) for s in _CL_SHAPES]
    ps = [_cl_dev(t, FP32).copy_(t) for t in p0]
    gs_ = [_cl_dev(t, dt) for t in p0]
    ss = [_cl_dev(t, BF16) for t in p0]
    assert not ps[0].is_contiguous() and ps[0].is_contiguous(memory_format=torch.channels_last)
    lr = 1e-2
    for k in range(STEPS):
        before = [p.detach().clone() for p in ps]
        for g in gs_:
            g.copy_(torch.randn(g.shape, generator=gen))
        _X().mt_fromage(ps, gs_, ss, lr, None)
        for i, p in enumerate(ps):
            ref = _fromage64(before[i].cpu(), gs_[i].cpu(), _f32(lr))
            py = _ratio(_fromage_python(before[i], gs_[i], lr), ref)
            got = _ratio(p, ref)
            assert got <= _bound_factor(py), (k, i, got, py)
            if p.numel():
                assert torch.equal(ss[i], p.to(BF16)), (k, i)


# ---- Madam -----------------------------------------------------------------------------------
M_LRS = (1e-2, 1e-2, 2e-2)  # rewritten before step 3
M_SCALE = 3.0
CLAMP_LR, CLAMP_SCALE = 0.1, 1.5  # the ±max clamp bites on part of every larger tensor


@functools.lru_cache(maxsize=2)
def _madam_case(gdt):
    """CPU inputs, never modified. Element 0 of every gradient of step 1 is 0 (0 / 0 -> 0) and
    element 1 of every parameter of 3 or more elements is 0 (stays 0)."""
    gen = torch.Generator().manual_seed(1234)
    p0 = [torch.randn(n, generator=gen) for n in ALL_SIZES]
    for p in p0:
        if p.numel() >= 3:
            p[1] = 0
    grads = [[torch.randn(n, generator=gen).to(gdt) for n in ALL_SIZES] for _ in range(STEPS)]
    for g in grads[0]:
        if g.numel():
            g[0] = 0
    return p0, grads


def _madam64(p, g, v, step, mx, lr, g_bound):
    """One Madam step in float64 on the fp32 values the kernel was given; ``step`` is the count
    after the prologue has advanced it."""
    p, g, v = p.double(), g.double(), v.double()
    bc = 1 - 0.999 ** step
    v = 0.999 * v + 0.001 * g * g
    gn = g / (v / bc).sqrt()
    gn = torch.where(torch.isnan(gn), torch.zeros_like(gn), gn)
    if g_bound is not None:
        gn = gn.clamp(-g_bound, g_bound)
    p = p * torch.exp(-lr * gn * torch.sign(p))
    return p.clamp(-mx, mx), v


def _madam_python(p, g, v, step_before, mx, lr, scale, g_bound):
    """The Python class, fp32, on the device, one step from the same state."""
    from imaginaire_amd.optimizers import Madam
    q = torch.nn.Parameter(p.detach().clone().contiguous())
    q.grad = g.detach().float().reshape(q.shape).contiguous()
    opt = Madam([q], lr=lr, scale=scale, g_bound=g_bound)
    opt.state[q] = {'max': mx, 'step': step_before,
                    'exp_avg_sq': v.detach().clone().reshape(q.shape).contiguous()}
    opt.step()
    return q.detach(), opt.state[q]['exp_avg_sq']


def _run_madam(gdt, path, offs, g_bound, name, lrs=M_LRS, scale=M_SCALE, clamp_share=None):
    p0, grads = _madam_case(gdt)
    bufs = _operands(p0, gdt, offs, with_v=True)
    ps, gs_, vs, ss = bufs['p'][1], bufs['g'][1], bufs['v'][1], bufs['s'][1]
    X = _X()
    state = torch.zeros(len(ps), 2, dtype=FP32, device='cuda')
    sts = list(state.unbind(0))
    X.mt_madam_init(ps, sts, scale)
    torch.cuda.synchronize()
    for i, p in enumerate(p0):
        ref = scale * float(p.double().pow(2).mean().sqrt()) if p.numel() else 0.0
        assert abs(float(state[i, 1]) - ref) <= ADAM_ATOL + ADAM_RTOL * ref, (name, i)
        assert float(state[i, 0]) == 0
        assert torch.equal(ps[i].cpu(), p)  # (the bound was taken without touching p)
    hyper = torch.tensor([lrs[0]], dtype=FP32, device='cuda') if path == 'hyper' else None
    worst, worst_py, shares = 0.0, 0.0, []
    for k in range(STEPS):
        lr = _f32(lrs[k])
        before_p = [p.detach().clone() for p in ps]
        before_v = [v.detach().clone() for v in vs]
        mxs = state[:, 1].tolist()
        for g_dev, g in zip(gs_, grads[k]):
            g_dev.copy_(g)
        if hyper is not None:
            hyper.fill_(lrs[k])
            X.mt_madam(ps, gs_, vs, ss, sts, 123.0, g_bound, hyper)
        else:
            X.mt_madam(ps, gs_, vs, ss, sts, lrs[k], g_bound, None)
        torch.cuda.synchronize()
        assert state[:, 0].tolist() == [float(k + 1)] * len(ps)  # every listed step moved on
        assert state[:, 1].tolist() == mxs
        for i, p in enumerate(ps):
            rp, rv = _madam64(before_p[i].cpu(), grads[k][i], before_v[i].cpu(), k + 1, mxs[i],
                              lr, g_bound)
            qp, qv = _madam_python(before_p[i], gs_[i], before_v[i], k, mxs[i], lrs[k], scale,
                                   g_bound)
            py = max(_ratio(qp, rp), _ratio(qv, rv))
            got = max(_ratio(p, rp), _ratio(vs[i], rv))
            worst, worst_py = max(worst, got), max(worst_py, py)
            assert got <= _bound_factor(py), \
                '%s step %d [%d, n=%d]: err / bound %.3f, Python class %.3f' % (
                    name, k + 1, i, p.numel(), got, py)
            if p.numel() >= 3:
                assert float(p[1]) == 0.0  # p = 0 stays 0
            if k == 0 and p.numel():
                assert float(gs_[i][0]) == 0 and float(vs[i][0]) == 0  # the 0 / 0 element ...
                assert float(p[0]) == float(before_p[i][0].clamp(-mxs[i], mxs[i]))  # ... stood
            if i == MULTI_CHUNK:
                shares.append(float((rp.abs() == mxs[i]).double().mean()))
        _check_gaps_and_shadows(bufs, k + 1, name)
    print('%s: max err / Adam bound: kernel %.3f, Python Madam %.3f; share of the %d-element '
          'tensor at ±max after each step: %s' % (name, worst, worst_py, ALL_SIZES[MULTI_CHUNK],
                                                  ['%.3f' % s for s in shares]))
    if clamp_share is not None:
        lo, hi = clamp_share
        assert any(lo <= s <= hi for s in shares), shares
    return bufs, state


_M_ALIGNED = [(gdt, path, gb) for gdt in ('fp32', 'bf16') for path in ('hyper', 'host')
              for gb in (None, 0.5)]
_M_MISALIGNED = [('fp32', {'p': 4}), ('fp32', {'g': 8}), ('fp32', {'v': 12}), ('bf16', {'g': 6}),
                 ('fp32', {'s': 2}), ('bf16', {'v': 4})]


@gpu
@pytest.mark.parametrize('gdt,path,g_bound', _M_ALIGNED)
def test_madam_vector_body(gdt, path, g_bound):
    """All operands aligned: the 16-byte body and its tail, several chunks per tensor, the
    per-parameter device step and bound, g = 0 at step 1, p = 0, ``g_bound`` None / 0.5.

    Measured (MI355X), max err / Adam bound in every Madam case of this file: kernel 0.011-0.012,
    Python ``Madam`` 0.011-0.012: the Adam tolerance holds as it is."""
    _run_madam(_DT[gdt], path, {}, g_bound, 'madam-%s-%s-gb%s' % (gdt, path, g_bound))


@gpu
@pytest.mark.parametrize('gdt,offs', _M_MISALIGNED,
                         ids=['%s-%s+%d' % (g, *list(o.items())[0]) for g, o in _M_MISALIGNED])
def test_madam_one_operand_misaligned(gdt, offs):
    """Exactly one of p / g / v / shadow off the vector alignment: the scalar path."""
    path = 'hyper' if 'v' in offs else 'host'
    gb = 0.5 if 'p' in offs or 's' in offs else None
    _run_madam(_DT[gdt], path, offs, gb, 'madam-%s-%s' % (gdt, offs))


@gpu
@pytest.mark.parametrize('g_bound', [None, 0.5])
def test_madam_clamp_bites(g_bound):
    """lr 0.1, scale 1.5: between 1% and 50% of the 2 kChunk + 3 element tensor end a step at
    ±max (asserted on the oracle's output; the values were chosen with the Python ``Madam`` on
    the CPU, ``test_madam_clamp_case_holds_on_cpu``), the rest inside."""
    _run_madam(FP32, 'host', {}, g_bound, 'madam-clamp-gb%s' % g_bound, lrs=(CLAMP_LR,) * STEPS,
               scale=CLAMP_SCALE, clamp_share=(0.01, 0.5))


def test_madam_clamp_case_holds_on_cpu():
    """The clamp case is a condition on the inputs: with the Python ``Madam`` (CPU, no GPU
    needed) between 1% and 50% of the multi-chunk tensor sit at ±max after every step."""
    from imaginaire_amd.optimizers import Madam
    p0, grads = _madam_case(FP32)
    p = torch.nn.Parameter(p0[MULTI_CHUNK].clone())
    opt = Madam([p], lr=CLAMP_LR, scale=CLAMP_SCALE)
    for k in range(STEPS):
        p.grad = grads[k][MULTI_CHUNK].clone()
        opt.step()
        mx = torch.tensor(opt.state[p]['max'], dtype=FP32)
        share = float((p.detach().abs() == mx).float().mean())
        assert 0.01 <= share <= 0.5, (k, share)


@gpu
def test_madam_channels_last():
    gen = torch.Generator().manual_seed(78)
    p0 = [torch.randn(s, generator=gen) for s in _CL_SHAPES]
    ps = [_cl_dev(t, FP32).copy_(t) for t in p0]
    gs_ = [_cl_dev(t, BF16) for t in p0]
    vs = [_cl_dev(t, FP32).zero_() for t in p0]
    ss = [_cl_dev(t, BF16) for t in p0]
    state = torch.zeros(len(ps), 2, dtype=FP32, device='cuda')
    sts = list(state.unbind(0))
    X = _X()
    X.mt_madam_init(ps, sts, M_SCALE)
    lr = 1e-2
    for k in range(STEPS):
        bp = [p.detach().clone() for p in ps]
        bv = [v.detach().clone() for v in vs]
        for g in gs_:
            g.copy_(torch.randn(g.shape, generator=gen))
        X.mt_madam(ps, gs_, vs, ss, sts, lr, 0.5, None)
        mxs = state[:, 1].tolist()
        for i, p in enumerate(ps):
            rp, rv = _madam64(bp[i].cpu(), gs_[i].cpu(), bv[i].cpu(), k + 1, mxs[i], _f32(lr), 0.5)
            qp, qv = _madam_python(bp[i], gs_[i], bv[i], k, mxs[i], lr, M_SCALE, 0.5)
            py = max(_ratio(qp, rp), _ratio(qv, rv))
            got = max(_ratio(p, rp), _ratio(vs[i], rv))
            assert got <= _bound_factor(py), (k, i, got, py)
            if p.numel():
                assert torch.equal(ss[i], p.to(BF16)), (k, i)


# ---- repeatability -------------------------------------------------------------------------------
@gpu
def test_two_runs_are_bitwise_equal():
    """Fixed-order reduces, no atomics: the same steps from the same state give the same bits."""
    a = _run_fromage(FP32, 'host', {}, 'fromage-repeat-a')
    b = _run_fromage(FP32, 'host', {}, 'fromage-repeat-b')
    for x, y in zip(a['p'][1], b['p'][1]):
        assert torch.equal(x, y)
    (a, sa), (b, sb) = (_run_madam(BF16, 'hyper', {}, 0.5, 'madam-repeat-%s' % t) for t in 'ab')
    assert torch.equal(sa, sb)
    for key in 'pv':
        for x, y in zip(a[key][1], b[key][1]):
            assert torch.equal(x, y)


# ---- the optimizer classes on the GPU --------------------------------------------------------
_OPT_SHAPES = [(64, 32, 3, 3), (257,), (1000, 7)]


def _make(kind, fused, ps, lr):
    from imaginaire_amd import optimizers as O
    if kind == 'fromage':
        return (O.FusedFromage if fused else O.Fromage)(ps, lr=lr)
    return (O.FusedMadam if fused else O.Madam)(ps, lr=lr, scale=3.0, g_bound=2.0)


@gpu
@pytest.mark.parametrize('kind', ['fromage', 'madam'])
def test_captured_fused_step_matches_eager(kind):
    """2 eager warm-up steps on a side stream, then ``zero_grad -> backward of Σ(p·x)² -> step``
    captured and replayed 3 times, the learning rate halved through ``sync_hyper`` before the
    last replay: parameters (and Madam's ``exp_avg_sq`` and device steps, = 5) bitwise those of
    a second fused instance stepped 5 times eagerly, and within the Adam tolerance of the Python
    class stepped 5 times."""
    from imaginaire_amd.ops import _ext
    from imaginaire_amd.optimizers.fused_adam import register_shadow, shadow_of
    torch.manual_seed(0)
    init = [torch.randn(*s, device='cuda') for s in _OPT_SHAPES]
    init[0] = init[0].contiguous(memory_format=torch.channels_last)
    xs = [torch.randn(*s, device='cuda') for s in _OPT_SHAPES]
    lr0, lr1 = 1e-2, 5e-3

    def fresh():
        return [torch.nn.Parameter(t.detach().clone()) for t in init]
    ps, es, rs = fresh(), fresh(), fresh()
    for plist in (ps, es):
        register_shadow(plist[0], torch.empty_like(plist[0], dtype=BF16))
    opt, eopt, ropt = _make(kind, True, ps, lr0), _make(kind, True, es, lr0), \
        _make(kind, False, rs, lr0)

    def step(params, o):
        o.zero_grad(set_to_none=True)
        loss = sum((p * x).pow(2).sum() for p, x in zip(params, xs))
        loss.backward()
        o.step()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(ps, opt)
    torch.cuda.current_stream().wait_stream(side)
    versions = [p._version for p in ps]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step(ps, opt)
    _ext.ext().flush_deferred_uploads()
    for k in range(3):
        if k == 2:
            opt.param_groups[0]['lr'] = lr1
            opt.sync_hyper()
        g.replay()
    for o, params in ((eopt, es), (ropt, rs)):
        for k in range(5):
            if k == 4:
                o.param_groups[0]['lr'] = lr1
            step(params, o)
    torch.cuda.synchronize()
    assert [p._version for p in ps] == versions  # a native step bumps no version counter
    for i, (p, e, r) in enumerate(zip(ps, es, rs)):
        assert torch.equal(p, e), (kind, i)
        assert _ratio(p, r.detach()) <= 1.0, (kind, i, _ratio(p, r.detach()))
        if kind == 'madam':
            sp, se, sr = opt.state[p], eopt.state[e], ropt.state[r]
            assert torch.equal(sp['exp_avg_sq'], se['exp_avg_sq'])
            assert sp['_dev'].tolist() == se['_dev'].tolist() and float(sp['_dev'][0]) == 5
            assert _ratio(sp['exp_avg_sq'], sr['exp_avg_sq']) <= 1.0
            assert abs(float(sp['_dev'][1]) - sr['max']) <= ADAM_RTOL * sr['max']
    assert torch.equal(shadow_of(ps[0]), ps[0].detach().to(BF16))
    if kind == 'madam':
        sd = opt.state_dict()['state']
        assert [st['step'] for st in sd.values()] == [5, 5, 5]
        assert all(type(st['max']) is float and '_dev' not in st for st in sd.values())


@gpu
def test_fused_madam_resume_on_the_gpu():
    """2 native steps, ``state_dict`` into the Python ``Madam`` and into an already-stepped
    ``FusedMadam`` (its device tensors refreshed in place), 2 more steps: the fused resume is
    bitwise the 4 uninterrupted fused steps; a parameter without a gradient keeps its step."""
    import copy
    from imaginaire_amd.optimizers import FusedMadam, Madam
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=gen).cuda() for s in _OPT_SHAPES]
    grads = [[torch.randn(s, generator=gen).cuda() for s in _OPT_SHAPES] for _ in range(4)]
    grads[1][1] = None
    kw = dict(lr=1e-2, scale=2.0, g_bound=1.0)

    def run(o, params, ks):
        for k in ks:
            for p, gr in zip(params, grads[k]):
                p.grad = None if gr is None else gr.clone()
            o.step()

    def fresh():
        return [torch.nn.Parameter(t.clone()) for t in init]
    base = fresh()
    obase = FusedMadam(base, **kw)
    run(obase, base, range(4))
    assert [int(obase.state[p]['_dev'][0]) for p in base] == [4, 3, 4]

    a = fresh()
    oa = FusedMadam(a, **kw)
    run(oa, a, range(2))
    sd = copy.deepcopy(oa.state_dict())
    assert [st['step'] for st in sd['state'].values()] == [2, 1, 2]

    b = fresh()
    ob = FusedMadam(b, **kw)
    run(ob, b, [3, 3, 3])
    ptrs = [ob.state[p]['_dev'].data_ptr() for p in b]
    with torch.no_grad():
        for p, q in zip(b, a):
            p.copy_(q)
    ob.load_state_dict(sd)
    assert [ob.state[p]['_dev'].data_ptr() for p in b] == ptrs
    run(ob, b, [2, 3])
    for i, (p, q) in enumerate(zip(b, base)):
        assert torch.equal(p, q), i
        assert torch.equal(ob.state[p]['exp_avg_sq'], obase.state[q]['exp_avg_sq'])
        assert ob.state[p]['_dev'].tolist() == obase.state[q]['_dev'].tolist()

    c = fresh()
    oc = Madam(c, **kw)
    with torch.no_grad():
        for p, q in zip(c, a):
            p.copy_(q)
    oc.load_state_dict(copy.deepcopy(sd))
    run(oc, c, [2, 3])
    for i, (p, q) in enumerate(zip(c, base)):
        assert _ratio(p, q.detach()) <= 1.0, i
        assert oc.state[p]['step'] == int(obase.state[q]['_dev'][0])


# ---- trainer level ---------------------------------------------------------------------------
def _build(tmp, opt_type):
    from imaginaire_amd.config import Config
    from imaginaire_amd.utils.trainer import get_model_optimizer_and_scheduler, get_trainer
    torch.manual_seed(0)
    cfg = Config(os.path.join(ROOT, 'configs', 'unit_test', 'spade.yaml'))
    cfg.speed_benchmark = False
    cfg.logdir = str(tmp)
    cfg.trainer.model_average_start_iteration = 3
    cfg.gen_opt.type = opt_type
    cfg.dis_opt.type = opt_type
    nets = get_model_optimizer_and_scheduler(cfg, seed=0)
    tr = get_trainer(cfg, *nets, train_data_loader=[], val_data_loader=None)
    tr.net_G_module.style_encoder.freeze_random = True
    return cfg, tr


@gpu
@pytest.mark.parametrize('opt_type', ['fromage', 'madam'])
def test_spade_trainer_step_is_captured(tmp_path, opt_type):
    """The SPADE unit-test trainer with both optimizers set to ``opt_type``: the factory hands out
    the fused classes, the step is captured, 5 iterations give finite losses, after the last
    replay every bf16 shadow is bitwise its weight, and Madam's per-parameter device steps have
    moved on with every replay. (The Python ``Fromage`` reads its norms on the host, which a
    capture refuses: that step falls back to eager. The Python ``Madam`` keeps its step count on
    the host and rebinds ``exp_avg_sq`` to a new tensor every step, neither of which a replay
    can advance.)"""
    import math
    from imaginaire_amd import optimizers as O
    from imaginaire_amd.datasets.synthetic import DeviceBatchSource
    from imaginaire_amd.optimizers.fused_adam import shadow_of
    from imaginaire_amd.utils.cuda_graph import make_trainer_step
    torch.cuda.set_device(0)
    cfg, tr = _build(tmp_path, opt_type)
    fused = O.FusedFromage if opt_type == 'fromage' else O.FusedMadam
    assert type(tr.opt_G) is fused and type(tr.opt_D) is fused
    src = DeviceBatchSource(cfg, 2, torch.device('cuda', 0), pool=4, seed=0)
    step, graphed = make_trainer_step(tr, warmup=2)
    assert graphed is not None
    for i in range(5):
        torch.manual_seed(1)
        b = src.next()
        d = tr.start_of_iteration({k: v.clone() if torch.is_tensor(v) else v
                                   for k, v in b.items()}, i)
        step(d)
        torch.cuda.synchronize()
        assert math.isfinite(float(tr.dis_losses['total'])), i
        assert math.isfinite(float(tr.gen_losses['total'])), i
    assert graphed.graph is not None and not graphed.failed, 'step was not captured'
    shadowed = 0
    for o in (tr.opt_G, tr.opt_D):
        for p in (p for g in o.param_groups for p in g['params']):
            s = shadow_of(p)
            if s is not None:
                shadowed += 1
                assert torch.equal(s, p.detach().to(BF16))
    assert shadowed > 0
    if opt_type == 'madam':  # every replay advanced the per-parameter device steps
        for o in (tr.opt_G, tr.opt_D):
            assert max(int(st['_dev'][0]) for st in o.state.values()) == 5
