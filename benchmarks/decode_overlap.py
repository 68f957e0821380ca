#!/usr/bin/env python
"""What overlapping consecutive direct decodes is worth without producers:
``ext.bench_decode_overlap`` queues ``iters`` decodes of B registered host
frames (640x480) with no host synchronisation in between, all on one HIP
stream or alternating over several, each launch followed by one completion
event as in the stream loader.

Each line: batch, cin, streams, us per launch, GB/s of frame bytes read over
PCIe and a pixel check of every output.
python benchmarks/decode_overlap.py [--batch 8,16] [--streams 1,2]
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / 'pytorch-blender_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', default='8,16')
    ap.add_argument('--streams', default='1,2')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeat', type=int, default=3)
    a = ap.parse_args()
    import torch  # noqa: F401
    from blendtorch import ops
    e = ops.hip_ext()
    for B in (int(b) for b in a.batch.split(',')):
        for cin in (3, 4):
            for _ in range(a.repeat):
                for k in (int(s) for s in a.streams.split(',')):
                    us, gbs, bad = e.bench_decode_overlap(B, 480, 640, cin, a.iters, k)
                    print(json.dumps({'batch': B, 'cin': cin, 'streams': k, 'us_per_launch': round(us, 1),
                                      'gbytes_per_s': round(gbs, 2), 'bad': bad}), flush=True)


if __name__ == '__main__':
    main()
