"""The grouped launch of the SPADE label convs against the same layers one by one, at the four
label-map sizes of the bench step ([4, 192, h, w] x G x [128, 192, 5, 5], spectral norm, bias,
ReLU), interleaved in one process, random bf16 operands. Forward: ``conv2d_mfma_grouped``
against G ``conv2d_mfma`` calls. Backward: ``bias_act_bwd_grouped`` + ``conv2d_wgrad_mfma_grouped``
against G x (``bias_act_bwd`` + ``conv2d_wgrad_mfma`` with the spectral-norm finalize).

    python scripts/probe/label_group_probe.py
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from imaginaire_amd.ops import _ext  # noqa: E402

CL = torch.channels_last
BF = torch.bfloat16
B, CIN, CINP, COUT, K, PAD = 4, 185, 192, 128, 5, 2
shapes = [(128, 256, 5), (64, 128, 5), (32, 64, 5), (16, 32, 4)]  # h, w, layers per G forward


def timeit(fn, iters=20):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


X = _ext.ext()
torch.manual_seed(0)
print('%-10s %2s | %-34s | %-34s' % ('label map', 'G', 'forward: one by one / grouped',
                                     'k2 + wgrad: one by one / grouped'))
for h, w, G in shapes:
    x = torch.zeros(B, CINP, h, w, device='cuda', dtype=BF).contiguous(memory_format=CL)
    x[:, :CIN] = torch.randn(B, CIN, h, w, device='cuda').to(BF)
    ws = [(torch.randn(COUT, CINP, K, K, device='cuda') / (CIN * K * K) ** 0.5).to(BF)
          .contiguous(memory_format=CL) for _ in range(G)]
    sh = [t[:, :CIN].contiguous(memory_format=CL) for t in ws]
    bs = [torch.randn(COUT, device='cuda') for _ in range(G)]
    sg = [torch.full((1,), 1.0 + 0.1 * g, device='cuda') for g in range(G)]
    us = [torch.randn(COUT, device='cuda') for _ in range(G)]
    vs = [torch.randn(CIN * K * K, device='cuda') for _ in range(G)]
    dys = [torch.randn(B, COUT, h, w, device='cuda').to(BF).contiguous(memory_format=CL)
           for _ in range(G)]

    def fwd1():
        return [X.conv2d_mfma(x, ws[g], bs[g], 1, 1, PAD, PAD, 1, 1, 0.0, 1, COUT, None, sg[g], 0)
                for g in range(G)]

    def fwdg():
        return X.conv2d_mfma_grouped(x, ws, bs, sg, PAD, PAD, 0.0)

    ys = fwdg()
    assert len(ys) == G and all(torch.equal(a, b) or (a.float() - b.float()).abs().max() < 0.1
                                for a, b in zip(ys, fwd1()))

    def bwd1():
        out = []
        for g in range(G):
            dz, db = X.bias_act_bwd(ys[g], dys[g], 0.0)
            out.append(X.conv2d_wgrad_mfma(dz, x, K, K, 1, 1, PAD, PAD, 1, 1, COUT, CIN, False, 1,
                                           0, [sh[g], us[g], vs[g], sg[g]], None, 0))
        return out

    def bwdg():
        dz, db = X.bias_act_bwd_grouped(ys, dys, 0.0)
        return X.conv2d_wgrad_mfma_grouped(dz, x, G, K, K, PAD, PAD, CIN, 0,
                                           [[sh[g], us[g], vs[g], sg[g]] for g in range(G)], [])

    for a, b in zip(bwdg(), bwd1()):
        assert (a - b).abs().max().item() <= 2e-2 * max(1.0, b.abs().max().item())
    t = {k: [] for k in ('f1', 'fg', 'b1', 'bg')}
    for rnd in range(3):
        for k, fn in (('f1', fwd1), ('fg', fwdg), ('b1', bwd1), ('bg', bwdg)):
            t[k].append(timeit(fn))
    m = {k: min(v) for k, v in t.items()}
    fl = 2.0 * B * h * w * G * COUT * CINP * K * K
    print('%4dx%-5d %2d | %6.3f / %6.3f ms (%4.0f / %4.0f TF/s) | %6.3f / %6.3f ms (%.2fx)' % (
        h, w, G, m['f1'], m['fg'], fl / m['f1'] / 1e9, fl / m['fg'] / 1e9, m['b1'], m['bg'],
        m['b1'] / m['bg']), flush=True)
