"""``FusedFromage`` / ``FusedMadam`` without a GPU: their ``torch._foreach`` paths are bitwise the
Python ``Fromage`` / ``Madam`` (a parameter without a gradient on step 2, an all-zero gradient,
an all-zero parameter, ``g_bound`` None and set), the optimizer factory honours ``fused_opt``,
and ``Madam`` <-> ``FusedMadam`` state dicts load into each other with the resumed run equal to
the uninterrupted one."""
import copy
import types

import pytest
import torch

from imaginaire_amd.optimizers import Fromage, FusedFromage, FusedMadam, Madam

SHAPES = [(7,), (5, 3), (4, 2, 3, 3), (1,), (33, 17), (6,), (9,)]
ZERO_GRAD, ZERO_PARAM, NO_GRAD_STEP2 = 5, 6, 1  # indices into SHAPES
STEPS = 5
LR = 0.05


def _params(seed=3):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=gen) for s in SHAPES]
    ps[ZERO_PARAM].zero_()
    return [torch.nn.Parameter(p) for p in ps]


def _grads(seed=4, steps=STEPS):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for k in range(steps):
        gs = [torch.randn(s, generator=gen) for s in SHAPES]
        gs[ZERO_GRAD].zero_()
        if k == 1:
            gs[NO_GRAD_STEP2] = None
        out.append(gs)
    return out


def _run(opt, ps, grads):
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.clone()
        opt.step()


def test_foreach_fromage_is_bitwise_fromage():
    grads = _grads()
    a, b = _params(), _params()
    _run(Fromage(a, lr=LR), a, grads)
    _run(FusedFromage(b, lr=LR), b, grads)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i
    # both zero-norm branches moved their tensor (ratio 1; the 1 / sqrt(1 + lr²) shrink)
    assert bool(torch.isfinite(b[ZERO_PARAM]).all()) and bool((b[ZERO_PARAM] != 0).any())
    assert bool(torch.isfinite(b[ZERO_GRAD]).all())
    assert not torch.equal(b[ZERO_GRAD], _params()[ZERO_GRAD])


@pytest.mark.parametrize('g_bound', [None, 0.5])
def test_foreach_madam_is_bitwise_madam(g_bound):
    grads = _grads()
    a, b = _params(), _params()
    oa = Madam(a, lr=LR, scale=1.5, g_bound=g_bound)
    ob = FusedMadam(b, lr=LR, scale=1.5, g_bound=g_bound)
    _run(oa, a, grads)
    _run(ob, b, grads)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i
        sa, sb = oa.state[x], ob.state[y]
        assert sa['step'] == sb['step'] == (STEPS - 1 if i == NO_GRAD_STEP2 else STEPS)
        assert sa['max'] == sb['max']
        assert torch.equal(sa['exp_avg_sq'], sb['exp_avg_sq']), i
    assert not bool(torch.isnan(torch.cat([p.detach().reshape(-1) for p in b])).any())
    assert torch.equal(b[ZERO_PARAM], torch.zeros(SHAPES[ZERO_PARAM]))
    mx = ob.state[b[ZERO_GRAD]]['max']  # 0 / 0 -> 0: only the clamp touches it
    assert torch.equal(b[ZERO_GRAD], _params()[ZERO_GRAD].detach().clamp(-mx, mx))
    # the clamp at ±max bit somewhere (scale 1.5), so that line of the update is compared too
    assert any(bool((p.detach().abs() == ob.state[p]['max']).any()) for p in b)


def test_signatures_match_the_python_classes():
    import inspect
    assert inspect.signature(FusedFromage.__init__) == inspect.signature(Fromage.__init__)
    assert inspect.signature(FusedMadam.__init__) == inspect.signature(Madam.__init__)


def test_factory_honours_fused_opt():
    from imaginaire_amd.utils.trainer import get_optimizer_for_params
    for typ, fused, plain in (('fromage', FusedFromage, Fromage), ('madam', FusedMadam, Madam)):
        cfg = types.SimpleNamespace(type=typ, lr=0.01)
        assert type(get_optimizer_for_params(cfg, _params())) is fused
        cfg.fused_opt = True
        assert type(get_optimizer_for_params(cfg, _params())) is fused
        cfg.fused_opt = False
        assert type(get_optimizer_for_params(cfg, _params())) is plain
    cfg = types.SimpleNamespace(type='madam', lr=0.01, scale=2.0, g_bound=0.25)
    opt = get_optimizer_for_params(cfg, _params())
    assert (opt.scale, opt.g_bound, opt.param_groups[0]['lr']) == (2.0, 0.25, 0.01)


@pytest.mark.parametrize('first,second', [(Madam, FusedMadam), (FusedMadam, Madam),
                                          (FusedMadam, FusedMadam)])
def test_madam_state_dict_round_trip(first, second):
    """2 steps with ``first``, its state dict loaded into ``second`` (on other weights: a resume
    restores the weights as well), 3 more steps: bitwise the 5 uninterrupted steps."""
    grads = _grads()
    kw = dict(lr=LR, scale=1.5, g_bound=0.5)
    base = _params()
    obase = Madam(base, **kw)
    _run(obase, base, grads)

    a = _params()
    oa = first(a, **kw)
    _run(oa, a, grads[:2])
    sd = copy.deepcopy(oa.state_dict())
    assert all('_hyper' not in g for g in sd['param_groups'])
    for st in sd['state'].values():
        assert set(st) == {'max', 'step', 'exp_avg_sq'}
        assert type(st['max']) is float and type(st['step']) is int

    b = _params(seed=99)
    ob = second(b, **kw)
    with torch.no_grad():
        for p, q in zip(b, a):
            p.copy_(q)
    ob.load_state_dict(sd)
    _run(ob, b, grads[2:])
    for i, (x, y) in enumerate(zip(base, b)):
        assert torch.equal(x, y), i
        assert obase.state[x]['step'] == ob.state[y]['step']
        assert torch.equal(obase.state[x]['exp_avg_sq'], ob.state[y]['exp_avg_sq'])


def test_fused_fromage_state_dict_round_trip():
    a = _params()
    oa = FusedFromage(a, lr=LR)
    _run(oa, a, _grads()[:1])
    sd = oa.state_dict()
    assert sd['param_groups'][0]['lr'] == LR and '_hyper' not in sd['param_groups'][0]
    ob = Fromage(_params(), lr=1.0)
    ob.load_state_dict(copy.deepcopy(sd))
    assert ob.param_groups[0]['lr'] == LR
