#!/usr/bin/env python
"""The link side of the slot mirror, rectangle against block mask, without a
loader: B pinned host frames (640x480, the RGB part of rgb_a slots) with the
regions and masks a real ``cubesim`` stream reported for them, decoded to fp32
CHW by ``decode_delta`` (the reported rectangle widened to 64-pixel columns)
and by ``decode_delta_blocks`` (the reported 64x16 blocks), each against HBM
mirrors that already hold the frames.  Timed with HIP events over ``--iters``
back-to-back launches.

Each line: kernel, batch, us per image, bytes read from the host per image,
the fraction of the frame that is, and GB/s over the link while the kernel runs.
python benchmarks/slot_blocks.py [--batch 8,16] [--iters 200] [--repeat 3]
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / 'pytorch-blender_amd'))

H, W = 480, 640


def record(n, port, seed=3):
    """n frames of one cubesim with their reports: [(rgb bytes u8 [H*W*3], (y0, y1, x0, x1), band_rows, words)]."""
    from blendtorch import btt
    from blendtorch.transport import shm, zmq
    out = []
    with btt.BlenderLauncher(producer='cubesim', num_instances=1, named_sockets=['DATA'], start_port=port, proto='ipc',
                             seed=seed, instance_args=[['--mode', 'rgba', '--shm', '3']]) as bl:
        s = zmq.Context().socket(zmq.PULL)
        s.connect(bl.launch_info.addresses['DATA'][0])
        for i in range(n + 200):
            if not s.poll(20000):
                raise RuntimeError('the producer fell silent')
            msg = s.recv_pyobj()
            desc = msg[shm.KEY]
            if i == 0:   # what the loader asks of a ring it mirrors
                shm.add_hint(desc[0], shm.WANT_PLANAR_ALPHA | shm.WANT_SLOT_DELTA | shm.WANT_SLOT_BLOCKS)
            if len(desc) == 11 and desc[8] == ('rgb_a',) and len(out) < n:
                rgb = np.frombuffer(shm._open(desc[0]).mm, np.uint8, H * W * 3, desc[2]).copy()
                band_rows, mask = desc[10]
                out.append((rgb, tuple(desc[9][1:]), band_rows, [int(v) for v in np.frombuffer(mask, '<u2')]))
            shm.release(desc)
            if len(out) == n:
                break
        s.close()
    if len(out) < n:
        raise RuntimeError(f'only {len(out)} frames carried a block report')
    return out


def widen(r):
    y0, y1, x0, x1 = r
    if y1 < y0:
        return (0, -1, 0, -1)
    return (y0, y1, x0 // 64 * 64, min((x1 // 64 + 1) * 64 - 1, W - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', default='8,16')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--port', type=int, default=24500)
    a = ap.parse_args()
    import torch
    from blendtorch import ops
    ext = ops.hip_ext()
    dev = torch.device('cuda', 0)
    cfg = ops.DecodeConfig.unit(channels='rgb', gamma=2.2)
    lut = ops.device_lut(cfg, dev).data_ptr()
    batches = [int(b) for b in a.batch.split(',')]
    frames = record(max(batches), a.port)
    fb = H * W * 3
    host, host_dev = ext.host_mapped_alloc(fb * len(frames))
    for b, f in enumerate(frames):
        ctypes.memmove(host + b * fb, f[0].ctypes.data, fb)
    mirrors = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
    stream = ops._stream(dev)
    try:
        for B in batches:
            out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
            srcs = [host_dev + b * fb for b in range(B)]
            mirs = [mirrors.data_ptr() + b * fb for b in range(B)]
            rects = [widen(frames[b][1]) for b in range(B)]
            common = (out.data_ptr(), lut, B, H, W, 3, 3, list(cfg.cmap), 0, ops.OUT_DTYPES[cfg.dtype],
                      ops.LAYOUTS[cfg.layout], stream)
            kernels = {
                'decode_delta': (lambda: ext.decode_delta(srcs, mirs, [v for r in rects for v in r], *common),
                                 sum(max(0, r[1] - r[0] + 1) * max(0, r[3] - r[2] + 1) for r in rects) * 3),
                'decode_delta_blocks': (lambda: ext.decode_delta_blocks(srcs, mirs, frames[0][2],
                                                                        [frames[b][3] for b in range(B)], *common),
                                        sum(bin(wd).count('1') * 64 * min(frames[b][2], H - k * frames[b][2])
                                            for b in range(B) for k, wd in enumerate(frames[b][3])) * 3),
            }
            want = ops.reference_decode(mirrors[:B].cpu().reshape(B, H, W, 3), cfg, flip=[0] * B)
            for _ in range(a.repeat):
                for name, (run, host_bytes) in kernels.items():
                    out.zero_()
                    for _ in range(20):
                        run()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(a.iters):
                        run()
                    t1.record()
                    torch.cuda.synchronize()
                    us = t0.elapsed_time(t1) * 1e3 / a.iters
                    print(json.dumps({'kernel': name, 'batch': B, 'us_per_image': round(us / B, 2),
                                      'host_bytes_per_image': host_bytes // B,
                                      'fraction_of_frame': round(host_bytes / (B * fb), 3),
                                      'host_gbytes_per_s': round(host_bytes / us / 1e3, 2),
                                      'bad': int((out.cpu() != want).sum())}), flush=True)
    finally:
        ext.host_mapped_free(host)


if __name__ == '__main__':
    main()
