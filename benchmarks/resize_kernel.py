"""Standalone timing of the fused resize against decode + F.interpolate.

B x 480x640 RGBA frames resident in HBM -> 224x224 fp32 NCHW RGB in 'full' mode
(``ops.ResizedCrop((224, 224), mode='full')``), beside the two-kernel path the
fused kernel replaces: ``ops.decode`` of the whole frames into HBM, then
``F.interpolate(mode='bilinear', align_corners=False)``.  Device time from HIP
events over ``--iters`` back-to-back launches after ``--warmup``; one JSON row.

    python benchmarks/resize_kernel.py [--batch 8] [--iters 200] [--warmup 20]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'pytorch-blender_amd'))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--size', type=int, nargs=2, default=(224, 224))
    ap.add_argument('--resolution', default='640x480')
    args = ap.parse_args(argv)
    import torch
    import torch.nn.functional as F
    from blendtorch import ops

    ops.hip_ext()
    dev = torch.device('cuda', 0)
    W, H = (int(v) for v in args.resolution.lower().split('x'))
    size = tuple(args.size)
    x = torch.randint(0, 256, (args.batch, H, W, 4), dtype=torch.uint8, device=dev)
    rc = ops.ResizedCrop(size, mode='full')
    fused_cfg = ops.DecodeConfig.unit(channels='rgb', gamma=2.2, resize=rc)
    plain_cfg = ops.DecodeConfig.unit(channels='rgb', gamma=2.2)
    win = ops.resized_windows(rc, H, W, args.batch)
    out = torch.empty(fused_cfg.out_shape(args.batch, H, W), device=dev)
    full = torch.empty(plain_cfg.out_shape(args.batch, H, W), device=dev)

    def fused():
        ops.decode(x, fused_cfg, out=out, window=win)

    def two_kernels():
        ops.decode(x, plain_cfg, out=full)
        return F.interpolate(full, size=size, mode='bilinear', align_corners=False)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(args.iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / args.iters

    # sanity: the two paths agree to the tolerance derived in tests/test_resize_cpu.py
    fused()
    ref = two_kernels()
    tol = (4 * 2.0 ** -14 + 32 * 2.0 ** -24) * float(full.abs().max())
    err = float((out - ref).abs().max())
    rows = {'fused_us': timed(fused), 'decode_interpolate_us': timed(two_kernels),
            'decode_only_us': timed(lambda: ops.decode(x, plain_cfg, out=full))}
    print(json.dumps({'batch': args.batch, 'frame': [H, W], 'size': list(size),
                      **{k: round(v, 2) for k, v in rows.items()},
                      'fused_us_per_image': round(rows['fused_us'] / args.batch, 2),
                      'max_abs_diff_vs_interpolate': err, 'tolerance': tol}), flush=True)
    return 0 if err <= tol else 1


if __name__ == '__main__':
    sys.exit(main())
