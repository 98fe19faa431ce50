"""A/B the k11 epilogue in ONE process, interleaved rounds (cdna_hip_programming.md §5.4 rule 24):
IMAGINAIRE_AMD_WGRAD_EPILOGUE=0 (one dword store per accumulator register, every output through
a slab and wgrad_finalize unless it is an uncropped fp32 single slab) vs =1 (every tile
restaged through the LDS ring and stored as 16-byte pieces of whole rows; a single slab finished
by the kernel), on every k11 shape of the SPADE step (profiles/
spade_step_conv_log_r6_final_mi355x.txt), with the kernel the log names.

Two outputs per shape: plain fp32 (the epilogue stores alone) and the spectral-norm gradient
with <G, W> given as partials (the 5-element sn of the low-resolution layers: at S == 1 the
``on`` column has no slab and no wgrad_finalize_sn launch, so off - on is the epilogue gain plus
the finalize pass removed; the fp32 column's off - on is the epilogue gain alone). The last
column is the time of the wgrad_finalize_sn pass of the shape, sn5 off - fp32 off (fp32 off has
no second pass at S == 1 and wgrad_finalize at S > 1, so there it is the difference of the two
finalize kernels): at fin = yes this is what the finished output removes.

    python scripts/probe/wgrad_epilogue_probe.py
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from imaginaire_amd.ops import _ext  # noqa: E402

ext = _ext.ext()
CL = torch.channels_last
# (kernel of the log, B, Cin, H, W, Cout, k, stride, pad)
shapes = [
    ('k11', 4, 128, 128, 256, 1024, 5, 1, 2),
    ('k11', 4, 512, 128, 256, 512, 3, 1, 1),
    ('k11v2', 4, 192, 128, 256, 128, 5, 1, 2),
    ('k11v2', 4, 2048, 16, 32, 2048, 3, 1, 1),
    ('k11', 4, 128, 64, 128, 2048, 5, 1, 2),
    ('k11', 4, 1024, 32, 64, 1024, 3, 1, 1),
    ('k11', 4, 128, 64, 128, 1024, 5, 1, 2),
    ('k11', 4, 512, 64, 128, 512, 3, 1, 1),
    ('k11v2', 4, 128, 16, 32, 4096, 5, 1, 2),
    ('k11', 4, 128, 32, 64, 4096, 5, 1, 2),
    ('k11', 4, 128, 128, 256, 512, 5, 1, 2),
    ('k11v2', 4, 192, 64, 128, 128, 5, 1, 2),
    ('k11', 4, 128, 32, 64, 2048, 5, 1, 2),
    ('k11', 4, 2048, 32, 64, 1024, 3, 1, 1),
    ('k11', 4, 512, 128, 256, 256, 3, 1, 1),
    ('k11', 8, 192, 256, 512, 128, 4, 2, 1),
    ('k11', 4, 1024, 64, 128, 512, 3, 1, 1),
    ('k11v2', 4, 192, 32, 64, 128, 5, 1, 2),
    ('k11', 8, 512, 64, 128, 256, 3, 1, 1),
    ('k11v2', 4, 1024, 16, 32, 2048, 3, 1, 1),
    ('k11', 4, 256, 128, 256, 256, 3, 1, 1),
    ('k11', 4, 192, 16, 32, 128, 5, 1, 2),
    ('k11', 8, 128, 128, 256, 256, 4, 2, 1),
    ('k11', 8, 512, 32, 64, 1024, 3, 2, 1),
    ('k11', 8, 192, 128, 256, 128, 4, 2, 1),
    ('k11', 8, 256, 64, 128, 512, 4, 2, 1),
    ('k11', 8, 1024, 16, 32, 1024, 3, 2, 1),
    ('k11', 8, 512, 16, 32, 512, 4, 2, 1),
    ('k11', 8, 512, 32, 64, 512, 4, 2, 1),
    ('k11', 8, 512, 32, 64, 256, 3, 1, 1),
]
KNAME = {0: 'one-tap', 1: 'rows', 2: 'multi-tap', 3: 'v2'}
ITERS, ROUNDS = 10, 5
only = os.environ.get('ONLY')
print('%-44s %-9s %3s %4s | %-34s | %-58s' % ('shape', 'kernel', 'S', 'fin', 'fp32: off ms, on ms, '
                                            'off/on', 'sn5: off ms, on ms, off/on, off-on us, finalize_sn us'))
for kern, B, cin, H, W, cout, k, s, p in shapes:
    name = '[%d, %d, %d, %d] x [%d, %d, %d, %d] s%d p%d' % (B, cin, H, W, cout, cin, k, k, s, p)
    if only and only not in name:
        continue
    variant = 2 if kern == 'k11v2' else 1
    torch.manual_seed(0)
    x = torch.randn(B, cin, H, W, device='cuda', dtype=torch.bfloat16).contiguous(memory_format=CL)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = torch.randn(B, cout, Ho, Wo, device='cuda', dtype=torch.bfloat16).contiguous(
        memory_format=CL)
    shadow = torch.randn(cout, cin, k, k, device='cuda', dtype=torch.bfloat16).contiguous(
        memory_format=CL)
    sn5 = [shadow, torch.randn(cout, device='cuda'), torch.randn(cin * k * k, device='cuda'),
           torch.ones(1, device='cuda'), torch.randn(512, device='cuda')]
    modes = {'fp32': None, 'sn5': sn5}
    res = {(m, sw): [] for m in modes for sw in ('off', 'on')}
    plan = None
    for rnd in range(ROUNDS):
        for (m, sw), times in res.items():
            if sw == 'off':
                os.environ['IMAGINAIRE_AMD_WGRAD_EPILOGUE'] = '0'
            else:
                os.environ['IMAGINAIRE_AMD_WGRAD_EPILOGUE'] = '1'
            args = (dy, x, k, k, s, s, p, p, 1, 1, -1, -1, False, 1, variant, modes[m])
            if rnd == 0 and m == 'sn5' and sw == 'on':
                plan = ext.conv2d_wgrad_plan(*args)
            ext.conv2d_wgrad_mfma(*args)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(ITERS):
                ext.conv2d_wgrad_mfma(*args)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / ITERS * 1e3)
    os.environ.pop('IMAGINAIRE_AMD_WGRAD_EPILOGUE', None)
    t = {key: min(v) for key, v in res.items()}
    print('%-44s %-9s %3d %4s | %7.3f %7.3f %5.2fx | %7.3f %7.3f %5.2fx %7.1f %7.1f' % (
        name, KNAME[plan['kernel']], plan['S'], 'yes' if plan['finished_in_kernel'] else 'no',
        t['fp32', 'off'], t['fp32', 'on'], t['fp32', 'off'] / t['fp32', 'on'],
        t['sn5', 'off'], t['sn5', 'on'], t['sn5', 'off'] / t['sn5', 'on'],
        (t['sn5', 'off'] - t['sn5', 'on']) * 1e3,
        (t['sn5', 'off'] - t['fp32', 'off']) * 1e3), flush=True)
