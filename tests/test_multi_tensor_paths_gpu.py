"""k4 / k5 (``csrc/multi_tensor.hip``) on every branch, against the update written out in float64.

``mt_adam``: plain / L2 / AdamW, fp32 and bf16 gradients, ``grad_scale`` 1 and 0.5, three beta
pairs (beta1 = 0 included), the device hyper-parameter path (with its step counter and a learning
rate rewritten between steps) and the host bias-correction path (``hyper=None``), the 16-byte
vector body with its 1..3 element tail, the scalar fallback taken when exactly one of p / g / m /
v (or the bf16 gradient, or the bf16 shadow) is misaligned, chunk boundaries (``kChunk`` = 16384:
one short, exact, one over, two chunks + 3), tensors of fewer than 4 elements, an empty tensor in
the middle of every list, channels-last 4-D parameters, the host stride check, and the bf16
shadow written in the same pass (bitwise ``p.to(bfloat16)`` after every step).

``FusedAdam`` on the GPU: gradient re-layout, mixed gradient dtypes in one group, AdamW with a
scheduler-style learning rate, and checkpoint resume into a fresh and into an already-stepped
optimizer (bitwise equal to the uninterrupted run, device step counter refreshed).

``mt_sn_sigma``: the 16-byte path, the scalar path (columns not a multiple of 4, a misaligned
weight, a misaligned slice of the permuted-v workspace), several chunks per weight, contiguous
and channels-last, bitwise repeatability, and the table cache when one address is seen again
with another shape or layout. ``mt_ema``: fp32 vector / scalar (misaligned target or source),
bf16, with and without sigma, the device-side warm-up switch. ``mt_scale`` / ``mt_sqnorm`` in
fp32 and bf16, the table cache across an eviction, and ``ModelAverage`` on its native path.

Alignment is constructed, not hoped for: operands are carved from one flat buffer and every case
asserts ``data_ptr()`` modulo the vector width; the buffer between the operands must come back
untouched. GPU tests carry ``@gpu``; the two tests at the end run without a GPU.
"""
import copy
import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu
BF16, FP32 = torch.bfloat16, torch.float32
K_CHUNK = 16384  # kChunk of multi_tensor.hip
# <4 elements, a 1..3 element vector tail, one short of / exactly / one past a chunk, two chunks
# and a tail, several chunks
SIZES = (1, 3, 37, K_CHUNK - 1, K_CHUNK, K_CHUNK + 1, 2 * K_CHUNK + 3, 70001)
EMPTY_AT = 4  # every list also holds one numel == 0 tensor here
SENTINEL = 768.0  # (exact in bf16)
ADAM_ATOL, ADAM_RTOL = 1e-6, 1e-5  # those of test_multi_tensor_adam_and_ema
EPS = 1e-8
STEPS = 5
# scale factor with 15 significant bits: bf16 (8 bits) x S is exact in fp32, so the kernel's
# single rounding to bf16 and that of the float64 product are the same rounding
S_SCALE = 24249.0 / 65536.0


def _X():
    from imaginaire_amd.ops import _ext
    return _ext.ext()


def _close(got, ref, atol, rtol, name):
    got, ref = got.detach().double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if got.numel() == 0:
        return
    err = (got - ref).abs()
    bound = atol + rtol * ref.abs()
    bad = ~(err <= bound)  # (a NaN is bad)
    assert not bool(bad.any()), '%s: %d of %d off, max err %.3e, max err / bound %.3f' % (
        name, int(bad.sum()), bad.numel(), float(err.max()), float((err / bound).max()))


# ---- operands carved from one flat buffer ----------------------------------------------------
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
    """Everything of ``buf`` outside ``views`` still holds the sentinel."""
    used = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    item = buf.element_size()
    for v in views:
        if v.numel():
            s = (v.data_ptr() - buf.data_ptr()) // item
            used[s:s + v.numel()] = True
    rest = buf[~used].float()
    assert bool((rest == SENTINEL).all()), '%s: wrote outside its operands' % name


def _with_empty(sizes):
    s = list(sizes)
    s.insert(EMPTY_AT, 0)
    return s


ALL_SIZES = _with_empty(SIZES)


def _cl_strides(shape):
    n, c, h, w = shape
    return (c * h * w, 1, w * c, c)


# ---- float64 Adam ------------------------------------------------------------------------------
def _adam64_step(p, g, m, v, lr, b1, b2, eps, step, wd, adamw, gs):
    """One step as adam_kernel documents it, on float64 tensors (g: the gradient as the kernel
    reads it, i.e. already rounded to its dtype)."""
    g = g * gs
    if wd != 0 and not adamw:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    if wd != 0 and adamw:
        p = p * (1 - lr * wd)
    p = p - lr / bc1 * m / denom
    return p, m, v


_BETAS = [(0.5, 0.999), (0.9, 0.999), (0.0, 0.999)]
_DECAY = [('plain', 0.0, False), ('l2', 0.1, False), ('adamw', 0.1, True)]
_GDT = [FP32, BF16]
_GSCALE = [1.0, 0.5]
_LR_CONST = (1e-2,) * STEPS
_LR_SCHED = (1e-2, 1e-2, 5e-3, 5e-3, 2e-2)  # rewritten before steps 3 and 5


def _sweep_rows():
    """(name, betas, wd, adamw, grad dtype, grad_scale, per-step lr, step0)."""
    rows = []
    for b in _BETAS:
        for dname, wd, adamw in _DECAY:
            for gdt in _GDT:
                for gs in _GSCALE:
                    name = 'b%g-%s-%s-gs%g' % (b[0], dname, 'bf16' if gdt is BF16 else 'fp32', gs)
                    rows.append((name, b, wd, adamw, gdt, gs, _LR_CONST, 0))
    return rows


_SWEEP = _sweep_rows()
# a learning rate that changes between steps, from a step count other than 0
_SCHED = [('sched-l2-fp32', (0.9, 0.999), 0.1, False, FP32, 1.0, _LR_SCHED, 3),
          ('sched-adamw-bf16', (0.5, 0.999), 0.1, True, BF16, 0.5, _LR_SCHED, 3)]
_ROW_BY_NAME = {r[0]: r for r in _SWEEP + _SCHED}
# the row the alignment / shadow cases run: every term of the update is live
_ALIGN_ROW_FP32 = 'b0.9-l2-fp32-gs0.5'
_ALIGN_ROW_BF16 = 'b0.9-l2-bf16-gs0.5'


@functools.lru_cache(maxsize=4)
def _adam_case(name, sizes=tuple(ALL_SIZES)):
    """CPU inputs and the float64 result of a row, shared by the tests of that row (which run
    next to each other) and never modified:
    p0 [fp32 per tensor], grads [step][tensor] in the gradient dtype, (p, m, v) float64 after
    the last step, and p after every step."""
    _, (b1, b2), wd, adamw, gdt, gs, lrs, step0 = _ROW_BY_NAME[name]
    gen = torch.Generator().manual_seed(1234)
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[torch.randn(n, generator=gen).to(gdt) for n in sizes] for _ in range(STEPS)]
    p = [t.double() for t in p0]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    p_steps = []
    for k in range(STEPS):
        for i in range(len(sizes)):
            p[i], m[i], v[i] = _adam64_step(p[i], grads[k][i].double(), m[i], v[i], lrs[k], b1,
                                            b2, EPS, step0 + k + 1, wd, adamw, gs)
        p_steps.append(list(p))
    return p0, grads, (p, m, v), p_steps


def _run_mt_adam(name, path, ps, gs_, ms, vs, shadows=(), after_step=None):
    """Drive ``mt_adam`` through the row's 5 steps on device operands ``ps, gs_, ms, vs``
    (gs_ is refilled from the row's gradients before every step)."""
    _, (b1, b2), wd, adamw, gdt, gscale, lrs, step0 = _ROW_BY_NAME[name]
    _, grads, _, _ = _adam_case(name)
    X = _X()
    hyper = None
    if path == 'hyper':
        hyper = torch.tensor([lrs[0], float(step0), 0.0, 0.0], dtype=FP32, device='cuda')
    for k in range(STEPS):
        for g_dev, g in zip(gs_, grads[k]):
            g_dev.copy_(g.reshape(g_dev.shape))
        if hyper is not None:
            if k and lrs[k] != lrs[k - 1]:
                hyper[0:1].fill_(lrs[k])
            # the lr / step arguments are ignored on this path: pass values that would show
            X.mt_adam(ps, gs_, ms, vs, list(shadows), 123.0, b1, b2, EPS, 1, wd, adamw, gscale,
                      hyper)
        else:
            X.mt_adam(ps, gs_, ms, vs, list(shadows), lrs[k], b1, b2, EPS, step0 + k + 1, wd,
                      adamw, gscale, None)
        if after_step is not None:
            after_step(k)
    if hyper is not None:
        assert float(hyper[1]) == step0 + STEPS
        assert float(hyper[0]) == float(torch.tensor(lrs[-1], dtype=FP32))
    torch.cuda.synchronize()


def _check_adam(name, ps, ms, vs):
    _, _, (rp, rm, rv), _ = _adam_case(name)
    for i, (p, m, v) in enumerate(zip(ps, ms, vs)):
        tag = '%s[%d, n=%d]' % (name, i, p.numel())
        _close(p.reshape(-1), rp[i], ADAM_ATOL, ADAM_RTOL, tag + ' p')
        _close(m.reshape(-1), rm[i], ADAM_ATOL, ADAM_RTOL, tag + ' m')
        _close(v.reshape(-1), rv[i], ADAM_ATOL, ADAM_RTOL, tag + ' v')


def _adam_operands(name, offs=None):
    """Carved device operands of a row; offs: {'p' | 'g' | 'm' | 'v': byte offset}."""
    offs = offs or {}
    gdt = _ROW_BY_NAME[name][4]
    p0 = _adam_case(name)[0]
    bufs = {}
    for key, dt in (('p', FP32), ('g', gdt), ('m', FP32), ('v', FP32)):
        mod = 16 if dt is FP32 else 8  # 4 elements: the vector width of adam_kernel
        bufs[key] = _carve(ALL_SIZES, dt, offs.get(key, 0), modulo=mod)
    for t, src in zip(bufs['p'][1], p0):
        t.copy_(src)
    for key in ('m', 'v'):
        for t in bufs[key][1]:
            t.zero_()
    return bufs


def _adam_gaps(bufs, name):
    for key, (buf, views) in bufs.items():
        _gaps_untouched(buf, views, '%s %s' % (name, key))


# ---- mt_adam -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name,path,body', [(r[0], path, body) for r in _SWEEP + _SCHED
                                            for path in ('hyper', 'host')
                                            for body in ('vector', 'scalar')])
def test_adam_sweep(name, path, body):
    """Every combination of betas x decay x gradient dtype x grad_scale, and the two rows with a
    learning rate that changes between steps, on the device hyper path and on the host
    bias-correction path; with all operands aligned (vector body + tail) and with v 4 bytes off
    (the scalar fallback has its own copy of the update)."""
    bufs = _adam_operands(name, {'v': 4} if body == 'scalar' else None)
    _run_mt_adam(name, path, bufs['p'][1], bufs['g'][1], bufs['m'][1], bufs['v'][1])
    _check_adam(name, bufs['p'][1], bufs['m'][1], bufs['v'][1])
    _adam_gaps(bufs, name)


_MISALIGNED = [('fp32-%s+%d' % (op, off), _ALIGN_ROW_FP32, {op: off})
               for op in 'pgmv' for off in (4, 8, 12)] + \
              [('bf16-g+%d' % off, _ALIGN_ROW_BF16, {'g': off}) for off in (2, 4, 6)]


@gpu
@pytest.mark.parametrize('case', _MISALIGNED, ids=[c[0] for c in _MISALIGNED])
def test_adam_one_operand_misaligned(case):
    """Exactly one operand off the vector alignment (fp32: 4 / 8 / 12 bytes past 16; bf16
    gradient: 2 / 4 / 6 bytes past 8), the others on it: the scalar fallback."""
    _, name, offs = case
    bufs = _adam_operands(name, offs)
    for key, (_, views) in bufs.items():
        mod = 16 if views[0].dtype is FP32 else 8
        for t in views:
            if t.numel():
                assert t.data_ptr() % mod == offs.get(key, 0)
    path = 'hyper' if sum(offs.values()) % 8 else 'host'
    _run_mt_adam(name, path, bufs['p'][1], bufs['g'][1], bufs['m'][1], bufs['v'][1])
    _check_adam(name, bufs['p'][1], bufs['m'][1], bufs['v'][1])
    _adam_gaps(bufs, name)


_CL_SHAPES = [(5, 6, 3, 3), (3, 5, 7, 11), (0,), (16, 2, 1, 1), (37,)]


@gpu
@pytest.mark.parametrize('gdt', ['fp32', 'bf16'])
def test_adam_channels_last(gdt):
    """Channels-last 4-D parameters with m, v and the gradient in the parameter's strides; a
    gradient laid out otherwise is rejected by the host stride check."""
    name = _ALIGN_ROW_FP32 if gdt == 'fp32' else _ALIGN_ROW_BF16
    _, (b1, b2), wd, adamw, dt, gscale, lrs, _ = _ROW_BY_NAME[name]
    gen = torch.Generator().manual_seed(77)
    p0 = [torch.randn(s, generator=gen) for s in _CL_SHAPES]
    grads = [[torch.randn(s, generator=gen).to(dt) for s in _CL_SHAPES] for _ in range(STEPS)]

    def dev(t, dtype):
        if t.dim() == 4:
            return torch.empty_strided(t.shape, _cl_strides(t.shape), dtype=dtype, device='cuda')
        return torch.empty(t.shape, dtype=dtype, device='cuda')
    ps = [dev(t, FP32).copy_(t) for t in p0]
    ms = [dev(t, FP32).zero_() for t in p0]
    vs = [dev(t, FP32).zero_() for t in p0]
    gs_ = [dev(t, dt) for t in p0]
    assert not ps[0].is_contiguous() and ps[0].is_contiguous(memory_format=torch.channels_last)
    assert ms[0].stride() == ps[0].stride() == vs[0].stride() == gs_[0].stride()
    X = _X()
    # (fresh storage: no cached table for these pointers, so the check runs)
    bad = [g.contiguous() if g.dim() == 4 else g for g in gs_]
    assert bad[0].stride() != ps[0].stride()
    with pytest.raises(RuntimeError, match='strides must match'):
        X.mt_adam(ps, bad, ms, vs, [], 1e-2, b1, b2, EPS, 1, wd, adamw, gscale, None)
    torch.cuda.synchronize()
    for p, t in zip(ps, p0):
        assert torch.equal(p.cpu(), t)  # the rejected call wrote nothing
    rp = [t.double() for t in p0]
    rm = [torch.zeros_like(t) for t in rp]
    rv = [torch.zeros_like(t) for t in rp]
    for k in range(STEPS):
        for i in range(len(ps)):
            gs_[i].copy_(grads[k][i])
            rp[i], rm[i], rv[i] = _adam64_step(rp[i], grads[k][i].double(), rm[i], rv[i], lrs[k],
                                               b1, b2, EPS, k + 1, wd, adamw, gscale)
        X.mt_adam(ps, gs_, ms, vs, [], lrs[k], b1, b2, EPS, k + 1, wd, adamw, gscale, None)
    for i in range(len(ps)):
        _close(ps[i], rp[i], ADAM_ATOL, ADAM_RTOL, 'cl p[%d]' % i)
        _close(ms[i], rm[i], ADAM_ATOL, ADAM_RTOL, 'cl m[%d]' % i)
        _close(vs[i], rv[i], ADAM_ATOL, ADAM_RTOL, 'cl v[%d]' % i)


@gpu
@pytest.mark.parametrize('path', ['hyper', 'host'])
@pytest.mark.parametrize('shadow_off', [0, 2, 4, 6])
def test_adam_shadow(shadow_off, path):
    """A bf16 shadow for six of the parameters, none (an empty tensor) for the rest: after every
    step the shadow is bitwise ``p.to(bfloat16)``. Offset 0: written by the 8-byte vector store;
    2 / 4 / 6 bytes past 8: the shadow alone is misaligned and the step takes the scalar path."""
    name = _ALIGN_ROW_FP32
    bufs = _adam_operands(name)
    ps = bufs['p'][1]
    has = [i % 3 != 1 and n > 0 for i, n in enumerate(ALL_SIZES)]
    assert [n for n, h in zip(ALL_SIZES, has) if not h] == [3, 0, 2 * K_CHUNK + 3]
    sbuf, sviews = _carve([n if h else 0 for n, h in zip(ALL_SIZES, has)], BF16, shadow_off,
                          modulo=8)
    for t, h in zip(sviews, has):
        assert t.numel() == 0 or (h and t.data_ptr() % 8 == shadow_off)
    p_steps = _adam_case(name)[3]

    def after(k):
        for i, (s, p) in enumerate(zip(sviews, ps)):
            if has[i]:
                assert torch.equal(s, p.to(BF16)), 'step %d shadow %d' % (k + 1, i)
        # the shadowed parameters took the same update as the others
        for i, p in enumerate(ps):
            _close(p, p_steps[k][i], ADAM_ATOL, ADAM_RTOL, 'step %d p[%d]' % (k + 1, i))
    _run_mt_adam(name, path, ps, bufs['g'][1], bufs['m'][1], bufs['v'][1], sviews, after)
    _check_adam(name, ps, bufs['m'][1], bufs['v'][1])
    _adam_gaps(bufs, name)
    _gaps_untouched(sbuf, sviews, 'shadow')


# ---- FusedAdam on the GPU --------------------------------------------------------------------
_FA_SHAPES = [(6, 5, 3, 3), (37,), (16, 8), (4, 3, 1, 2), (K_CHUNK + 1,)]


def _fa_params(seed, cl=True):
    gen = torch.Generator().manual_seed(seed)
    ps = []
    for s in _FA_SHAPES:
        t = torch.randn(s, generator=gen).cuda()
        if cl and t.dim() == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(t.requires_grad_(True))
    return ps


def _fa_grads(seed, steps, dtypes):
    gen = torch.Generator().manual_seed(seed)
    return [[torch.randn(s, generator=gen).to(dt) for s, dt in zip(_FA_SHAPES, dtypes)]
            for _ in range(steps)]


def _fa_reference(p0, grads, kernel_dt, lrs, b1, b2, wd, adamw):
    rp = [t.detach().double().cpu() for t in p0]
    rm = [torch.zeros_like(t) for t in rp]
    rv = [torch.zeros_like(t) for t in rp]
    for k, gk in enumerate(grads):
        for i, g in enumerate(gk):
            rp[i], rm[i], rv[i] = _adam64_step(rp[i], g.to(kernel_dt).double(), rm[i], rv[i],
                                               lrs[k], b1, b2, EPS, k + 1, wd, adamw, 1.0)
    return rp, rm, rv


def _fa_check(opt, ps, ref):
    rp, rm, rv = ref
    for i, p in enumerate(ps):
        st = opt.state[p]
        assert st['exp_avg'].stride() == p.stride() == st['exp_avg_sq'].stride()
        _close(p, rp[i], ADAM_ATOL, ADAM_RTOL, 'p[%d]' % i)
        _close(st['exp_avg'], rm[i], ADAM_ATOL, ADAM_RTOL, 'm[%d]' % i)
        _close(st['exp_avg_sq'], rv[i], ADAM_ATOL, ADAM_RTOL, 'v[%d]' % i)


@gpu
@pytest.mark.parametrize('dtypes', ['fp32', 'bf16-first', 'fp32-first'])
def test_fused_adam_relayout_and_mixed_dtypes(dtypes):
    """Channels-last parameters with contiguous ``.grad`` (re-laid out by ``step``), and
    ``.grad`` dtypes mixed within one group (the first gradient's dtype is the kernel's): the
    float64 update of the gradients as rounded to the dtype the kernel is given."""
    from imaginaire_amd.optimizers.fused_adam import FusedAdam
    n = len(_FA_SHAPES)
    dts = {'fp32': [FP32] * n, 'bf16-first': [BF16, FP32, BF16, FP32, FP32],
           'fp32-first': [FP32, BF16, FP32, BF16, BF16]}[dtypes]
    ps = _fa_params(5)
    p0 = [p.detach().clone() for p in ps]
    grads = _fa_grads(6, 3, dts)
    opt = FusedAdam(ps, lr=1e-2, betas=(0.9, 0.999), eps=EPS)
    for gk in grads:
        for p, g in zip(ps, gk):
            if g.dtype != p.dtype:
                p.grad_dtype = None  # (torch otherwise refuses a gradient of another dtype)
            p.grad = g.cuda()  # contiguous: not the channels-last strides of its parameter
            if p.dim() == 4 and p.shape[1] > 1:
                assert p.grad.stride() != p.stride()
        opt.step()
    ref = _fa_reference(p0, grads, dts[0], [1e-2] * 3, 0.9, 0.999, 0.0, False)
    _fa_check(opt, ps, ref)


@gpu
def test_fused_adam_adamw_with_scheduled_lr():
    """A group with weight decay in AdamW mode whose ``group['lr']`` changes between steps."""
    from imaginaire_amd.optimizers.fused_adam import FusedAdam
    ps = _fa_params(7)
    p0 = [p.detach().clone() for p in ps]
    lrs = [1e-2, 1e-2, 5e-3, 2e-2]
    grads = _fa_grads(8, len(lrs), [FP32] * len(_FA_SHAPES))
    opt = FusedAdam(ps, lr=lrs[0], betas=(0.5, 0.999), eps=EPS, weight_decay=0.1,
                    adam_w_mode=True)
    for lr, gk in zip(lrs, grads):
        opt.param_groups[0]['lr'] = lr
        for p, g in zip(ps, gk):
            p.grad = g.cuda().contiguous(memory_format=torch.channels_last) if g.dim() == 4 \
                else g.cuda()
        opt.step()
    _fa_check(opt, ps, _fa_reference(p0, grads, FP32, lrs, 0.5, 0.999, 0.1, True))
    g = opt.param_groups[0]
    assert g['step'] == len(lrs) and float(g['_hyper'][1]) == len(lrs)
    assert float(g['_hyper'][0]) == float(torch.tensor(lrs[-1], dtype=FP32))


@gpu
def test_fused_adam_checkpoint_resume_bitwise():
    """2 steps, ``state_dict``, ``load_state_dict`` into (A) a fresh optimizer and (B) one that
    has already stepped and owns a device step counter, 2 more steps: bitwise the 4
    uninterrupted steps (same kernel, same inputs), device counter == ``group['step']``."""
    from imaginaire_amd.optimizers.fused_adam import FusedAdam
    grads = _fa_grads(10, 4, [FP32] * len(_FA_SHAPES))
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=EPS, weight_decay=0.1)

    def steps(opt, ps, ks):
        for k in ks:
            for p, g in zip(ps, grads[k]):
                p.grad = g.cuda()
            opt.step()

    base_p = _fa_params(9)
    base = FusedAdam(base_p, **kw)
    steps(base, base_p, range(4))

    first_p = _fa_params(9)
    first = FusedAdam(first_p, **kw)
    steps(first, first_p, range(2))
    sd = first.state_dict()
    assert all('_hyper' not in g for g in sd['param_groups'])

    for variant in 'AB':
        ps = _fa_params(11)  # other values: a resumed run restores the weights as well
        opt = FusedAdam(ps, **kw)
        if variant == 'B':
            steps(opt, ps, [3, 3, 3])
            assert float(opt.param_groups[0]['_hyper'][1]) == 3
        with torch.no_grad():
            for p, q in zip(ps, first_p):
                p.copy_(q)
        opt.load_state_dict(copy.deepcopy(sd))
        assert opt.param_groups[0]['step'] == 2
        steps(opt, ps, [2, 3])
        g = opt.param_groups[0]
        assert g['step'] == 4 and float(g['_hyper'][1]) == 4, variant
        for i, (p, q) in enumerate(zip(ps, base_p)):
            assert torch.equal(p, q), 'variant %s p[%d]' % (variant, i)
            for key in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(opt.state[p][key], base.state[q][key]), (variant, key, i)


# ---- mt_sn_sigma ---------------------------------------------------------------------------------
SIG_ATOL, SIG_RTOL = 1e-4, 1e-4  # those of test_multi_tensor_adam_and_ema


def _sigma64(w, u, v):
    return float(u.double().cpu() @ w.double().cpu().reshape(w.shape[0], -1) @ v.double().cpu())


def _unit(n, gen):
    return torch.nn.functional.normalize(torch.randn(max(n, 1), generator=gen), dim=0)[:n]


# (name, shape, byte offset of W past 16). Order matters: the permuted-v workspace packs the
# column vectors back to back, so a weight's slice starts at the column total before it.
_SIG_ROWS = [
    ('linear-16x40', (16, 40), 0),          # 16-B path
    ('conv-32x16x5x5', (32, 16, 5, 5), 0),  # 16-B path, 400 columns
    ('three-chunks', (48, 32, 5, 5), 0),    # 38400 elements: 3 chunks, 16-B path
    ('empty', (4, 0), 0),
    ('w-misaligned', (12, 20), 4),          # W off 16 B, its workspace slice on it: scalar
    ('cols-27', (8, 3, 3, 3), 0),           # 27 columns: scalar
    ('vm-misaligned', (24, 8, 3, 3), 0),    # 72 columns right after 27: slice off 16 B: scalar
]


def _sig_operands(layout):
    gen = torch.Generator().manual_seed(21)
    sizes = [int(torch.Size(s).numel()) for _, s, _ in _SIG_ROWS]
    _, flat = _carve(sizes, FP32, [o for _, _, o in _SIG_ROWS])
    ws, us, vs, col0 = [], [], [], 0
    for (name, shape, off), f in zip(_SIG_ROWS, flat):
        cols = sizes[len(ws)] // shape[0]
        if len(shape) == 4 and layout == 'cl':
            w = f.as_strided(shape, _cl_strides(shape))
        else:
            w = f.view(shape)
        w.copy_(torch.randn(shape, generator=gen))
        if w.numel():
            assert w.data_ptr() % 16 == off
        if name == 'vm-misaligned':
            assert cols % 4 == 0 and col0 % 4 != 0
        elif name in ('linear-16x40', 'conv-32x16x5x5', 'three-chunks', 'w-misaligned'):
            assert cols % 4 == 0 and col0 % 4 == 0
        if name == 'three-chunks':
            assert w.numel() > 2 * K_CHUNK
        col0 += cols
        ws.append(w)
        us.append(_unit(shape[0], gen).cuda())
        vs.append(_unit(cols, gen).cuda())
    return ws, us, vs


@gpu
@pytest.mark.parametrize('layout', ['contiguous', 'cl'])
def test_sn_sigma_paths(layout):
    ws, us, vs = _sig_operands(layout)
    if layout == 'cl':
        assert not ws[1].is_contiguous()
    X = _X()
    a = X.mt_sn_sigma(ws, us, vs)
    b = X.mt_sn_sigma(ws, us, vs)
    ref = torch.tensor([_sigma64(w, u, v) for w, u, v in zip(ws, us, vs)], dtype=torch.float64)
    assert torch.equal(a, b)  # fixed reduction tree
    assert ref[3] == 0
    for i, (name, _, _) in enumerate(_SIG_ROWS):
        _close(a[i:i + 1], ref[i:i + 1], SIG_ATOL, SIG_RTOL, name)


def _view(buf, shape, layout):
    n = int(torch.Size(shape).numel())
    if layout == 'cl':
        return buf[:n].as_strided(shape, _cl_strides(shape))
    return buf[:n].view(shape)


# two views of ONE storage (same u and v storage too), called one after the other: the second
# must not be served the first one's table entry
_STALE = [
    ('cl-8x2x7x3-then-8x3x2x7', ((8, 2, 7, 3), 'cl'), ((8, 3, 2, 7), 'cl')),
    ('cl-8x3x2x7-then-8x2x7x3', ((8, 3, 2, 7), 'cl'), ((8, 2, 7, 3), 'cl')),
    ('cl-4x1x6x2-then-4x2x1x6', ((4, 1, 6, 2), 'cl'), ((4, 2, 1, 6), 'cl')),
    ('cl-4x5x6x1-then-4x6x1x5', ((4, 5, 6, 1), 'cl'), ((4, 6, 1, 5), 'cl')),
    ('8x4x3x3-contiguous-then-cl', ((8, 4, 3, 3), 'contiguous'), ((8, 4, 3, 3), 'cl')),
    ('8x64-then-16x32', ((8, 64), 'contiguous'), ((16, 32), 'contiguous')),
]


@gpu
@pytest.mark.parametrize('case', _STALE, ids=[c[0] for c in _STALE])
def test_sn_sigma_same_address_other_shape(case):
    """One buffer viewed as two weights of equal numel (and, for the first four, equal size(0)
    and equal 31·C + 7·H + W): every call returns the sigma of the view it was given."""
    _, first, second = case
    gen = torch.Generator().manual_seed(31)
    n = int(torch.Size(first[0]).numel())
    assert n == int(torch.Size(second[0]).numel())
    buf = torch.randn(n, generator=gen).cuda()
    ubuf = torch.randn(16, generator=gen).cuda()
    vbuf = torch.randn(64, generator=gen).cuda()
    X = _X()
    for k, (shape, layout) in enumerate((first, second, first)):
        w = _view(buf, shape, layout)
        u, v = ubuf[:shape[0]], vbuf[:n // shape[0]]
        assert (w.data_ptr(), u.data_ptr(), v.data_ptr()) == \
            (buf.data_ptr(), ubuf.data_ptr(), vbuf.data_ptr())
        got = X.mt_sn_sigma([w], [u], [v])
        ref = torch.tensor([_sigma64(w, u, v)], dtype=torch.float64)
        _close(got, ref, SIG_ATOL, SIG_RTOL, 'call %d %s %s' % (k + 1, shape, layout))


# ---- mt_ema --------------------------------------------------------------------------------------
EMA_ATOL, EMA_RTOL = 1e-5, 1e-5  # those of test_multi_tensor_adam_and_ema


def _ema_inputs(dtype, same_sign):
    gen = torch.Generator().manual_seed(41)
    t0 = [torch.randn(n, generator=gen).to(dtype) for n in ALL_SIZES]
    s0 = [torch.randn(n, generator=gen).to(dtype) for n in ALL_SIZES]
    if same_sign:
        # source and target of one sign per element (both signs occur): the bf16 bound below
        # is relative to the result, which holds for fp32 arithmetic only without cancellation
        s0 = [torch.copysign(s.float(), t.float()).to(dtype) for s, t in zip(s0, t0)]
    sig = torch.rand(len(ALL_SIZES), generator=gen) + 0.5
    return t0, s0, sig


def _ema64(t, s, beta, sigma):
    return beta * t.double() + (1 - beta) * s.double() / sigma


@gpu
@pytest.mark.parametrize('with_sigma', [True, False], ids=['sigma', 'nosigma'])
@pytest.mark.parametrize('case', ['aligned', 'dst+4', 'dst+8', 'src+12'])
def test_ema_fp32(case, with_sigma):
    t0, s0, sig = _ema_inputs(FP32, False)
    doff = int(case[4:]) if case.startswith('dst') else 0
    soff = int(case[4:]) if case.startswith('src') else 0
    tbuf, ts = _carve(ALL_SIZES, FP32, doff)
    sbuf, ss = _carve(ALL_SIZES, FP32, soff)
    for a, b in zip(ts + ss, t0 + s0):
        a.copy_(b)
    beta = 0.9
    _X().mt_ema(ts, ss, beta, sig.cuda() if with_sigma else None)
    for i, t in enumerate(ts):
        ref = _ema64(t0[i], s0[i], beta, float(sig[i]) if with_sigma else 1.0)
        _close(t, ref, EMA_ATOL, EMA_RTOL, '%s t[%d]' % (case, i))
        assert torch.equal(ss[i].cpu(), s0[i])
    _gaps_untouched(tbuf, ts, 'ema target')
    _gaps_untouched(sbuf, ss, 'ema source')


@gpu
@pytest.mark.parametrize('with_sigma', [True, False], ids=['sigma', 'nosigma'])
@pytest.mark.parametrize('off', [0, 2])
def test_ema_bf16(off, with_sigma):
    """bf16 targets and sources (scalar path): within 2^-8·|ref| + 1e-30 of the float64 result,
    i.e. one bf16 rounding of the result plus the fp32 arithmetic (no cancellation in the
    inputs: see _ema_inputs)."""
    t0, s0, sig = _ema_inputs(BF16, True)
    tbuf, ts = _carve(ALL_SIZES, BF16, off, modulo=8)
    sbuf, ss = _carve(ALL_SIZES, BF16, 0, modulo=8)
    for a, b in zip(ts + ss, t0 + s0):
        a.copy_(b)
    beta = 0.9
    _X().mt_ema(ts, ss, beta, sig.cuda() if with_sigma else None)
    for i, t in enumerate(ts):
        ref = _ema64(t0[i], s0[i], beta, float(sig[i]) if with_sigma else 1.0)
        err = (t.double().cpu() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 1e-30
        assert bool((err <= bound).all()), 't[%d]: max err / bound %.4f' % (
            i, float((err / bound).max()))
    _gaps_untouched(tbuf, ts, 'ema target')


@gpu
@pytest.mark.parametrize('count', [2, 3, 4, None])
def test_ema_warmup_switch(count):
    """start = 3: while the device counter is <= 3 the target becomes s / sigma whatever it held;
    past it, and without a counter, beta is used as given."""
    start, beta = 3, 0.9
    t0, s0, sig = _ema_inputs(FP32, False)
    t0 = [t * 1e6 for t in t0]  # an old value that would show through any beta != 0
    _, ts = _carve(ALL_SIZES, FP32, 0)
    _, ss = _carve(ALL_SIZES, FP32, 0)
    for a, b in zip(ts + ss, t0 + s0):
        a.copy_(b)
    cnt = None if count is None else torch.tensor([count], dtype=torch.long, device='cuda')
    _X().mt_ema(ts, ss, beta, sig.cuda(), cnt, start)
    copy_only = count is not None and count <= start
    for i, t in enumerate(ts):
        ref = _ema64(t0[i], s0[i], 0.0 if copy_only else beta, float(sig[i]))
        _close(t, ref, EMA_ATOL, EMA_RTOL, 'count %s t[%d]' % (count, i))
    if cnt is not None:
        assert int(cnt) == count


# ---- mt_scale / mt_sqnorm ------------------------------------------------------------------------
def _flat_inputs(dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen).to(dtype) for n in ALL_SIZES]


@gpu
@pytest.mark.parametrize('off', [0, 4])
@pytest.mark.parametrize('dtype', [FP32, BF16], ids=['fp32', 'bf16'])
def test_scale(dtype, off):
    x0 = _flat_inputs(dtype, 51)
    buf, xs = _carve(ALL_SIZES, dtype, off)
    for a, b in zip(xs, x0):
        a.copy_(b)
    s = torch.tensor(S_SCALE, dtype=FP32, device='cuda')
    assert s.dim() == 0 and float(s) == S_SCALE
    _X().mt_scale(xs, s)
    for i, x in enumerate(xs):
        ref = x0[i].double() * S_SCALE
        if dtype is FP32:
            _close(x, ref, 0.0, 1e-6, 'x[%d]' % i)
        else:
            assert torch.equal(x.cpu(), ref.to(BF16)), 'x[%d]' % i
    _gaps_untouched(buf, xs, 'scale')


@gpu
@pytest.mark.parametrize('dtype', [FP32, BF16], ids=['fp32', 'bf16'])
def test_sqnorm(dtype):
    x0 = _flat_inputs(dtype, 52)
    _, xs = _carve(ALL_SIZES, dtype, 0)
    for a, b in zip(xs, x0):
        a.copy_(b)
    a = _X().mt_sqnorm(xs)
    b = _X().mt_sqnorm(xs)
    ref = sum(float((x.double() ** 2).sum()) for x in x0)
    assert torch.equal(a, b)
    assert abs(float(a) - ref) <= 1e-4 * ref, (float(a), ref)
    # one tensor at a time: a list of a single short tensor, and of an empty one next to it
    for i in (0, 1, 3):
        one = _X().mt_sqnorm([xs[i], xs[EMPTY_AT]])
        r = float((x0[i].double() ** 2).sum())
        assert abs(float(one) - r) <= 1e-4 * r, (i, float(one), r)


@gpu
def test_table_cache_survives_eviction():
    """260 distinct single-tensor lists (the table cache is cleared once it holds more than 256),
    then the first and the last list again: every value right."""
    n_lists = 260
    sizes = [i % 7 + 1 for i in range(n_lists)]
    gen = torch.Generator().manual_seed(61)
    x0 = [torch.randn(n, generator=gen) for n in sizes]
    buf, xs = _carve(sizes, FP32, [4 * (i % 4) for i in range(n_lists)])
    for a, b in zip(xs, x0):
        a.copy_(b)
    assert len({x.data_ptr() for x in xs}) == n_lists
    half = torch.tensor(0.5, device='cuda')
    X = _X()
    for x in xs:
        X.mt_scale([x], half)
    X.mt_scale([xs[0]], half)
    X.mt_scale([xs[-1]], half)
    for i, x in enumerate(xs):
        f = 0.25 if i in (0, n_lists - 1) else 0.5
        assert torch.equal(x.cpu(), x0[i] * f), i
    _gaps_untouched(buf, xs, 'eviction')


# ---- ModelAverage on its native path -------------------------------------------------------------
def _ma_net():
    from torch import nn
    from torch.nn.utils import spectral_norm

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.sn_conv = spectral_norm(nn.Conv2d(6, 8, 3, padding=1))
            self.bn = nn.BatchNorm2d(8)
            self.conv = nn.Conv2d(8, 4, 3, padding=1, bias=True)
            self.sn_fc = spectral_norm(nn.Linear(20, 12))
    torch.manual_seed(71)
    return Net().cuda().to(memory_format=torch.channels_last)


@gpu
def test_model_average_native_path():
    """``ModelAverage(net, 0.9, start_iteration=2, remove_sn=True)`` over a spectral-normalised
    channels-last conv, a spectral-normalised linear layer, a BatchNorm and a plain conv: after
    each of 4 updates (weights perturbed in between) every averaged tensor equals the float64
    formula with sigma from the module's current u and v: a copy for updates 1 and 2, a lerp for
    3 and 4; ``num_batches_tracked`` is copied verbatim."""
    from imaginaire_amd.utils.model_average import ModelAverage
    net = _ma_net()
    w = net.sn_conv.weight_orig
    assert w.dim() == 4 and not w.is_contiguous() and \
        w.is_contiguous(memory_format=torch.channels_last)
    assert not net.conv.weight.is_contiguous()
    beta = 0.9
    ma = ModelAverage(net, beta, start_iteration=2, remove_sn=True)
    gen = torch.Generator().manual_seed(72)
    expect = None
    for update in range(1, 5):
        with torch.no_grad():
            for t in list(net.parameters()) + [net.bn.running_mean, net.bn.running_var]:
                t.add_(0.05 * torch.randn(t.shape, generator=gen).cuda())
            net.bn.num_batches_tracked.add_(update + 1)
        ma.update_average()
        src = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        tgt = ma.averaged_model.state_dict()
        assert not any(k.endswith(('_orig', '_u', '_v')) for k in tgt)
        b = 0.0 if update <= 2 else beta
        new = {}
        for key in tgt:
            if key + '_orig' in src:
                wo = src[key + '_orig']
                s64 = wo.double() / _sigma64(wo, src[key + '_u'], src[key + '_v'])
            elif not tgt[key].is_floating_point():
                assert torch.equal(tgt[key].cpu(), src[key]), key
                continue
            else:
                s64 = src[key].double()
            new[key] = s64 if b == 0.0 else b * expect[key] + (1 - b) * s64
            _close(tgt[key], new[key], EMA_ATOL, EMA_RTOL, 'update %d %s' % (update, key))
        assert {'sn_conv.weight', 'sn_fc.weight', 'conv.weight', 'conv.bias', 'bn.weight',
                'bn.running_mean', 'bn.running_var'} <= set(new)
        assert int(tgt['bn.num_batches_tracked']) == int(src['bn.num_batches_tracked']) > 0
        expect = new
    assert int(ma.num_updates_tracked) == 4


# ---- no GPU needed -------------------------------------------------------------------------------
def test_float64_adam_agrees_with_reference_adam():
    """The float64 reference of this file against the project's fp32 ``torch._foreach`` update
    (``_reference_adam``) on every sweep row, at the Adam tolerance: checks the reference."""
    from imaginaire_amd.optimizers.fused_adam import _reference_adam
    for row in _SWEEP + _SCHED:
        name, (b1, b2), wd, adamw, gdt, gs, lrs, step0 = row
        p0, grads, (rp, rm, rv), _ = _adam_case(name)
        ps = [t.clone() for t in p0]
        ms = [torch.zeros_like(t) for t in p0]
        vs = [torch.zeros_like(t) for t in p0]
        for k in range(STEPS):
            # (the fp32 update has no grad_scale: 1 and 0.5 scale exactly)
            gk = [g.float() * gs for g in grads[k]]
            _reference_adam(ps, gk, ms, vs, lrs[k], b1, b2, EPS, step0 + k + 1, wd, adamw)
        for i in range(len(ps)):
            _close(ps[i], rp[i], ADAM_ATOL, ADAM_RTOL, '%s p[%d]' % (name, i))
            _close(ms[i], rm[i], ADAM_ATOL, ADAM_RTOL, '%s m[%d]' % (name, i))
            _close(vs[i], rv[i], ADAM_ATOL, ADAM_RTOL, '%s v[%d]' % (name, i))
    assert len(_SWEEP) == 36


def _old_fold(shape):
    return shape[1] * 31 + shape[2] * 7 + shape[3]


def test_table_key_separates_colliding_shapes():
    """The key of the table cache (read through the extension's ``mt_table_key``, which builds
    and launches nothing) differs for channels-last weights at one address whose numel and
    size(0) agree and whose sizes folded as 31·C + 7·H + W agree too: the pairs named in the
    cases above and every such pair with sizes up to 7."""
    X = _X()
    buf = torch.zeros(8 * 7 * 7 * 7)

    def key(shape):
        w = _view(buf, shape, 'cl')
        assert w.data_ptr() == buf.data_ptr()
        return X.mt_table_key([[w]])
    named = [((8, 2, 7, 3), (8, 3, 2, 7)), ((4, 1, 6, 2), (4, 2, 1, 6)),
             ((4, 5, 6, 1), (4, 6, 1, 5)), ((2, 1, 8, 12), (2, 2, 3, 16))]
    for a, b in named:
        assert _old_fold(a) == _old_fold(b) and torch.Size(a).numel() == torch.Size(b).numel()
        assert key(a) != key(b), (a, b)
        assert key(a) == key(a)
    groups = {}
    rng = range(1, 8)
    for c in rng:
        for h in rng:
            for w in rng:
                groups.setdefault((c * h * w, _old_fold((1, c, h, w))), []).append((8, c, h, w))
    pairs = 0
    for shapes in groups.values():
        keys = [key(s) for s in shapes]
        assert len(set(keys)) == len(keys), shapes
        pairs += len(shapes) * (len(shapes) - 1) // 2
    assert pairs >= 3
    # one buffer as [8, 64] and as [16, 32], contiguous and channels-last
    assert key((8, 4, 3, 3)) != X.mt_table_key([[buf[:288].view(8, 4, 3, 3)]])
    assert X.mt_table_key([[buf[:512].view(8, 64)]]) != X.mt_table_key([[buf[:512].view(16, 32)]])
