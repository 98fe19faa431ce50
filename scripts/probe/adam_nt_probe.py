"""Timing of the multi-tensor optimizer kernels, and the A/B of plain vs non-temporal fp32 loads /
stores of Adam and EMA (IMAGINAIRE_AMD_ADAM_NT / IMAGINAIRE_AMD_EMA_NT, read once per process:
run this script once per setting).

SPADE-recipe-sized parameter set: 415M fp32 parameters in 400 tensors (fp32 grads, a bf16
shadow on the conv weights), i.e. the optimizer traffic of one bench step. Prints one line per
kernel (mt_adam, mt_ema, mt_fromage, mt_madam): ms per call over 20 calls after 3 warm-up calls,
and the effective HBM bandwidth (Adam: 16 B read + 12 B written per parameter, + 2 B for
shadowed ones).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from imaginaire_amd.ops import _ext  # noqa: E402

ITERS = 20


def timed(call):
    """ms per call(k): k = 1..3 warm up, the next ITERS are timed."""
    for k in range(1, 4):
        call(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(4, 4 + ITERS):
        call(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def main():
    torch.manual_seed(0)
    dev = torch.device('cuda', 0)
    sizes = []
    total, target = 0, 415_000_000
    i = 0
    while total < target:
        n = [2_359_296, 1_179_648, 589_824, 147_456, 4_096, 512][i % 6]
        sizes.append(n)
        total += n
        i += 1
    p = [torch.randn(n, device=dev) for n in sizes]
    g = [torch.randn(n, device=dev) * 1e-3 for n in sizes]
    m = [torch.zeros(n, device=dev) for n in sizes]
    v = [torch.zeros(n, device=dev) for n in sizes]
    sh = [torch.empty(n, device=dev, dtype=torch.bfloat16) if n > 4096 else
          torch.empty(0, device=dev, dtype=torch.bfloat16) for n in sizes]
    nshadow = sum(n for n in sizes if n > 4096)
    ext = _ext.ext()
    ms = timed(lambda s: ext.mt_adam(p, g, m, v, sh, 1e-4, 0.0, 0.999, 1e-8, s, 0.0, False, 1.0,
                                     None))
    nbytes = 28 * total + 2 * nshadow
    print('adam NT=%s: %d params in %d tensors: %.3f ms/call, %.2f TB/s effective' % (
        os.environ.get('IMAGINAIRE_AMD_ADAM_NT', '1'), total, len(sizes), ms,
        nbytes / ms / 1e9))
    # EMA of the same set (IMAGINAIRE_AMD_EMA_NT): 8 B read + 4 B written per parameter
    avg = [torch.zeros(n, device=dev) for n in sizes]
    ms = timed(lambda _: ext.mt_ema(avg, p, 0.999, None, None, 0))
    print('ema NT=%s: %.3f ms/call, %.2f TB/s effective' % (
        os.environ.get('IMAGINAIRE_AMD_EMA_NT', '1'), ms, 12 * total / ms / 1e9))
    # Fromage: the norm pass reads p and g (8 B), the update reads them again and writes p
    # (12 B), + 2 B for shadowed parameters
    ms = timed(lambda _: ext.mt_fromage(p, g, sh, 1e-4, None))
    print('fromage: %.3f ms/call, %.2f TB/s effective' % (
        ms, (20 * total + 2 * nshadow) / ms / 1e9))
    # Madam: 12 B read (p, g, exp_avg_sq) + 8 B written, + 2 B for shadowed parameters; the
    # state of each parameter is [step, max], max set from the parameter by mt_madam_init
    for t in v:
        t.zero_()
    st = [torch.zeros(2, device=dev) for _ in sizes]
    ext.mt_madam_init(p, st, 3.0)
    ms = timed(lambda _: ext.mt_madam(p, g, v, sh, st, 1e-4, 10.0, None))
    print('madam: %.3f ms/call, %.2f TB/s effective' % (
        ms, (20 * total + 2 * nshadow) / ms / 1e9))


if __name__ == '__main__':
    main()
