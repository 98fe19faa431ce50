"""Face crop of the pose recipe: per-sample host-box path vs the device path (k17).

    python scripts/probe/roi_crop_probe.py [--out profiles/roi_crop_probe_mi355x.txt]

Recipe shape: batch 3, 512x512, the pose config's 6-channel label (3 DensePose + 3 OpenPose),
fp32 RGB image. Times ``crop_face_from_output`` forward + backward on the private per-sample
path (``.nonzero()`` + four ``.item()`` per sample, a slice and ``F.interpolate`` per sample)
and on the device path (one ``part_bbox`` + one ``roi_crop_resize`` for the batch), with device
events after a warm-up, the two paths alternating round by round. Then each k17 kernel alone
(events around a run of back-to-back launches), with the bytes it has to move computed from
the shapes and the share of HBM bandwidth that gives.
"""
import argparse
import os
import sys
from types import SimpleNamespace as NS

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    p.add_argument('--rounds', type=int, default=20)
    p.add_argument('--iters', type=int, default=50)
    args = p.parse_args()

    import torch
    from imaginaire_amd.model_utils import fs_vid2vid as M
    from imaginaire_amd.ops import _ext
    from imaginaire_amd.ops.roi_crop import part_bbox

    if not torch.cuda.is_available():
        sys.exit('roi_crop_probe.py needs a GPU')
    dev = torch.device('cuda', 0)
    cfg = NS(input_labels=['pose_maps-densepose', 'poses-openpose'], input_types=[])
    b, h, w = 3, 512, 512
    g = torch.Generator().manual_seed(0)
    label = torch.rand(b, 6, h, w, generator=g) * 1.8 - 1
    label[:, 2] = -1
    label[0, 2, 60:150, 200:270] = 1
    label[1, 2, 300:420, 30:130] = 1
    label[2, 2, 20:60, 400:440] = 1
    label = label.to(dev)
    image = (torch.rand(b, 3, h, w, generator=g) * 2 - 1).to(dev).requires_grad_(True)
    face = h // 32 * 8
    dy = torch.randn(b, 3, face, face, generator=g).to(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def old():
        out = M._crop_face_per_sample(cfg, image, label)
        return torch.autograd.grad(out, image, dy)[0]

    def new():
        out = M.crop_face_from_output(cfg, image, label)
        return torch.autograd.grad(out, image, dy)[0]

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n * 1e3  # us per call

    ga, gb = old(), new()
    say('# roi_crop probe: %s, torch %s' % (torch.cuda.get_device_name(dev), torch.__version__))
    say('# shape: batch %d, %dx%d, label 6 channels fp32, image 3 channels fp32, face %dx%d' % (
        b, h, w, face, face))
    say('# dimage per-sample path vs device path: max abs diff %.3g (max |dimage| %.3g)' % (
        (ga - gb).abs().max().item(), ga.abs().max().item()))
    for fn in (old, new):
        timed(fn, 20)
    rows = {'per-sample': [], 'device': []}
    for _ in range(args.rounds):
        rows['per-sample'].append(timed(old, args.iters))
        rows['device'].append(timed(new, args.iters))
    say('# crop_face_from_output forward + backward, us per call: %d rounds x %d calls, '
        'alternating' % (args.rounds, args.iters))
    med = {}
    for k, v in rows.items():
        s = sorted(v)
        med[k] = s[len(s) // 2]
        say('%-11s median %8.1f  min %8.1f  max %8.1f' % (k, med[k], s[0], s[-1]))
    say('speed-up (medians): %.1fx' % (med['per-sample'] / med['device']))

    X = _ext.ext()
    boxes = part_bbox(label, 2, rule='face_densepose', threshold=0.9)
    bx = boxes[:, 0].tolist()
    area = sum((min(ye, h) - ys) * (min(xe, w) - xs) for ys, ye, xs, xe, _ in bx)
    like = torch.empty_like(image, device='meta')
    img = image.detach()
    kernels = [
        ('part_bbox', lambda: X.part_bbox(label, [2], 1, False, 0.9, 0),
         b * h * w * 4 + b * 5 * 4),
        ('roi_crop_fwd', lambda: X.roi_crop_fwd(img, boxes, face, face),
         area * 3 * 4 + b * 3 * face * face * 4),
        ('roi_crop_bwd', lambda: X.roi_crop_bwd(dy, boxes, like),
         b * 3 * face * face * 4 + b * 3 * h * w * 4),
    ]
    say('# each kernel alone: %d back-to-back launches between two events (launch gaps '
        'included); bytes = what the shapes require; HBM share against %.1f TB/s spec' % (
            200, HBM_PEAK / 1e12))
    for name, fn, nbytes in kernels:
        timed(fn, 20)
        s = sorted(timed(fn, 200) for _ in range(5))
        us = s[len(s) // 2]
        say('%-13s %7.2f us (min %.2f max %.2f)  %9d bytes  %6.1f GB/s  %4.1f%% of HBM peak' % (
            name, us, s[0], s[-1], nbytes, nbytes / us / 1e3, 100.0 * nbytes / (us * 1e-6) /
            HBM_PEAK))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
