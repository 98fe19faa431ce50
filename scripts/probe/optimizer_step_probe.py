"""A/B of the Python ``Fromage`` / ``Madam`` steps and their fused multi-tensor versions on the
SPADE generator's parameter set (``configs/bench/spade_256x512_synthetic.yaml``, random
gradients), with ``FusedAdam`` for scale.

3 warm-up and 20 timed steps per candidate, Python and fused alternating step by step, every
step timed with device events. Prints ms per step and the achieved bytes/s of the useful traffic:
5 words per element for Fromage (p and g read twice, p written) and for Madam (p, g, v read; v, p
written), 7 for Adam. Exits non-zero unless every fused step was faster than every Python step
of its pair.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from imaginaire_amd import optimizers as O  # noqa: E402


def generator_parameters(config):
    from imaginaire_amd.config import Config
    from imaginaire_amd.utils.trainer import get_model_optimizer_and_scheduler
    cfg = Config(config)
    cfg.logdir = '/tmp/optimizer_step_probe'
    nets = get_model_optimizer_and_scheduler(cfg, seed=0)
    opt_G = nets[2]
    ps = [p.detach() for g in opt_G.param_groups for p in g['params']]
    del nets
    return ps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config',
                    default=os.path.join(ROOT, 'configs', 'bench', 'spade_256x512_synthetic.yaml'))
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    args = ap.parse_args()
    torch.manual_seed(0)
    src = generator_parameters(args.config)
    numel = sum(p.numel() for p in src)
    grads = [torch.randn_like(p) * 1e-3 for p in src]
    print('SPADE generator: %d parameters in %d tensors, fp32 gradients, %s' % (
        numel, len(src), torch.cuda.get_device_name(0)))

    def candidate(make):
        ps = [torch.nn.Parameter(p.clone()) for p in src]
        for p, g in zip(ps, grads):
            p.grad = g
        return make(ps)

    cands = [
        ('Fromage', 5, candidate(lambda ps: O.Fromage(ps, lr=1e-4))),
        ('FusedFromage', 5, candidate(lambda ps: O.FusedFromage(ps, lr=1e-4))),
        ('Madam', 5, candidate(lambda ps: O.Madam(ps, lr=1e-4))),
        ('FusedMadam', 5, candidate(lambda ps: O.FusedMadam(ps, lr=1e-4))),
        ('FusedAdam', 7, candidate(lambda ps: O.FusedAdam(ps, lr=1e-4, betas=(0.0, 0.999)))),
    ]
    times = {name: [] for name, _, _ in cands}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(args.warmup + args.steps):
        for name, _, opt in cands:  # (alternating: one step of each per round)
            torch.cuda.synchronize()
            e0.record()
            opt.step()
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    rate = {}
    for name, words, _ in cands:
        t = sorted(times[name])
        mean = sum(t) / len(t)
        rate[name] = 4.0 * words * numel / (t[len(t) // 2] * 1e-3)
        print('%-13s %8.3f ms/step mean, %8.3f median, %8.3f min, %8.3f max; %d words/element: '
              '%.3f TB/s at the median' % (name, mean, t[len(t) // 2], t[0], t[-1], words,
                                           rate[name] / 1e12))
    ok = True
    for py, fused in (('Fromage', 'FusedFromage'), ('Madam', 'FusedMadam')):
        faster = max(times[fused]) < min(times[py])
        ok = ok and faster
        print('%s vs %s: slowest fused step %.3f ms, fastest Python step %.3f ms: %s; '
              '%.1fx at the median; %.0f%% of FusedAdam\'s bytes/s' % (
                  fused, py, max(times[fused]), min(times[py]),
                  'every fused step faster' if faster else 'NOT every fused step faster',
                  sorted(times[py])[len(times[py]) // 2] /
                  sorted(times[fused])[len(times[fused]) // 2],
                  100.0 * rate[fused] / rate['FusedAdam']))
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
