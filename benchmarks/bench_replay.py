#!/usr/bin/env python
"""HBM replay throughput: frames resident in a DeviceReplayBuffer, random
batches gathered + decoded by one fused kernel per batch.

    python benchmarks/bench_replay.py [--frames 4096] [--batch 8] [--steps 2000] [--fill producers|synthetic]
                                      [--crop H W] [--pad P] [--mirror p]
                                      [--stack K [--stride S] [--nstep N [--gamma G]] [--prioritized]]

``--fill producers`` streams the frames from headless Cube producers through
a raw-u8 DeviceLoader (the record-once, train-many-epochs workflow);
``synthetic`` writes random frames (same shape) straight into the store.
``--crop H W`` samples through random windows (``--mirror p``: mirrored with
probability p; ``--pad P``: replicate padding, ``--crop 480 640 --pad 4`` is
the random shift of DrQ / RAD) inside the same launch.
``--stack K`` times frame-stacked transitions, ``--stack K --nstep N`` the
n-step sample against the 1-step one and against the path composed on top of it,
``--stack K --prioritized`` the prioritized sample against the uniform one.
Prints one JSON line (images/s of decoded fp32 CHW batches); ``effective_tbps``
counts the bytes read (the window's) plus the bytes written.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'pytorch-blender_amd'))


def bench_stack(a, rb, cfg, fill_s):
    """--stack K: three ways to a batch of K-frame transitions, timed in this process, two rounds each."""
    import numpy as np
    import torch
    from blendtorch import ops
    dev, B, K, S = rb.device, a.batch, a.stack, a.stride
    cap, crop = rb.capacity, cfg.crop
    H, W, C = rb.frame_shape
    kw = dict(stack=K, stride=S, next_keys=('reward',))
    # (a) ONE launch (two graph nodes with --graph: the sample and the counter advance)
    fused = rb.graphed_transition_sampler(B, cfg, **kw) if a.graph else (lambda: rb.sample_transitions(B, cfg, **kw))
    rng = np.random.default_rng(0)

    # (b) what the parent API offers: 2K gathers (one window per stack, uploaded from the host), two cats and
    # the successor's metadata.  It does not look at episode starts, which only makes it cheaper; the given
    # windows are a host upload, so it cannot be captured: it runs eagerly also with --graph
    def composed():
        anchor = torch.randint(S, len(rb) - S, (B,), device=dev)
        wins = [None, None]
        if crop is not None:
            h, w = crop.size
            wins = [np.stack([rng.integers(-crop.pad, H + crop.pad - h + 1, B), rng.integers(-crop.pad, W + crop.pad - w + 1, B),
                              rng.integers(0, 2, B) * (crop.mirror > 0)], axis=1) for _ in range(2)]
        sides, out = [], {}
        for d in (0, 1):
            planes = []
            for f in range(K):
                g = rb.gather((anchor - (K - 1 - f - d) * S) % cap, cfg, **({} if crop is None else dict(windows=wins[d])))
                planes.append(g['image'])
                if d == 0 and f == K - 1:
                    out.update({k: v for k, v in g.items() if k != 'image'})
            sides.append(torch.cat(planes, dim=1))
        out.update(obs=sides[0], next_obs=sides[1], next_reward=rb.meta['reward'].index_select(0, (anchor + S) % cap))
        return out

    # (c) the equal-bytes floor: the plain (cropped) sample of 2 K B images, in launches of at most 1024
    n, parts = 2 * K * B, []
    while n:
        parts.append(min(n, 1024))
        n -= parts[-1]
    plain = [rb.graphed_sampler(p, cfg) if a.graph else (lambda p=p: rb.sample(p, cfg)) for p in parts]

    def floor():
        return [s() for s in plain]

    rows = {'fused transitions': fused, 'composed gathers': composed, 'equal-bytes sample': floor}
    times = {k: [] for k in rows}
    for _ in range(2):
        for name, fn in rows.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                b = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps * 1e6)
            del b
    us = {k: min(v) for k, v in times.items()}
    for name, v in times.items():
        print(f'{name:20s} {us[name]:10.2f} us/batch   (rounds: {", ".join("%.2f" % t for t in v)})', flush=True)
    print(f'fused / composed     {us["fused transitions"] / us["composed gathers"]:10.3f}', flush=True)
    print(f'fused / equal-bytes  {us["fused transitions"] / us["equal-bytes sample"]:10.3f}', flush=True)
    h, w = (H, W) if crop is None else crop.size
    moved = 2 * K * B * h * w * (C + cfg.cout * (4 if a.dtype == 'float32' else 2))
    print(json.dumps({'metric': 'replay transitions us/batch (HBM store -> stacked obs, next_obs)',
                      'value': round(us['fused transitions'], 2), 'unit': 'us/batch', 'batch': B, 'stack': K,
                      'stride': S, 'graph': a.graph, 'dtype': a.dtype, 'frame': [H, W, C], 'frames': a.frames,
                      'us_per_batch': {k: round(v, 2) for k, v in us.items()},
                      'rounds_us': {k: [round(t, 2) for t in v] for k, v in times.items()},
                      'fused_over_composed': round(us['fused transitions'] / us['composed gathers'], 3),
                      'fused_over_equal_bytes': round(us['fused transitions'] / us['equal-bytes sample'], 3),
                      'effective_tbps': round(moved / us['fused transitions'] / 1e6, 3), 'equal_bytes_launches': parts,
                      'fill_s': round(fill_s, 2),
                      'crop': None if crop is None else {'size': list(crop.size), 'pad': crop.pad,
                                                         'mirror': crop.mirror}}), flush=True)


def bench_nstep(a, rb, cfg, fill_s):
    """--stack K --nstep N: the fused n-step sample, the fused 1-step sample and the n-step batch composed on
    top of the 1-step sample, timed in this process, two rounds each."""
    import torch
    dev, B, K, S, N = rb.device, a.batch, a.stack, a.stride, a.nstep
    cap = rb.capacity
    kw = dict(stack=K, stride=S, next_keys=('reward',))
    nkw = dict(nstep=N, gamma=a.gamma, done_key='done')
    if a.graph:
        fused_n, fused_1 = rb.graphed_transition_sampler(B, cfg, **kw, **nkw), rb.graphed_transition_sampler(B, cfg, **kw)
    else:
        fused_n, fused_1 = (lambda: rb.sample_transitions(B, cfg, **kw, **nkw)), (lambda: rb.sample_transitions(B, cfg, **kw))
    reward, done, first = rb.meta['reward'], rb.meta['done'], rb.meta['first']

    # what a user writes on the 1-step API: the fused 1-step sample, N - 1 rounds of metadata gathers with the
    # flag walk in torch, and one more transition gather at c_{m-1} for the stack at c_m.  It runs eagerly
    # also with --graph (the second gather's anchors come out of the walk)
    def composed():
        b = rb.sample_transitions(B, cfg, **kw)
        c0, alive = b['index'], b['valid'].clone()
        age0 = (rb._next - 1 - c0) % cap
        steps = alive.to(torch.int32)
        ret = torch.where(alive, b['reward'], torch.zeros_like(b['reward']))
        g = torch.full_like(ret, a.gamma)
        for j in range(1, N):
            alive = (alive & (done.index_select(0, (c0 + (j - 1) * S) % cap) == 0) & (age0 - j * S >= S)
                     & (first.index_select(0, (c0 + (j + 1) * S) % cap) == 0))
            ret = torch.where(alive, ret + g * reward.index_select(0, (c0 + j * S) % cap), ret)
            g = torch.where(alive, g * a.gamma, g)
            steps = steps + alive.to(torch.int32)
        last = (c0 + (steps.to(torch.int64) - 1).clamp(min=0) * S) % cap
        term = b['valid'] & (done.index_select(0, last) != 0)
        nxt = rb.gather_transitions(last, cfg, **kw)
        b.update(next_obs=nxt['next_obs'], next_index=nxt['next_index'], next_reward=nxt['next_reward'],
                 nstep_return=ret, nstep_discount=torch.where(term | ~b['valid'], torch.zeros_like(g), g),
                 nstep_steps=steps)
        return b

    rows = {f'fused {N}-step': fused_n, 'fused 1-step': fused_1, f'composed {N}-step': composed}
    times = {k: [] for k in rows}
    for _ in range(2):
        for name, fn in rows.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                b = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps * 1e6)
            del b
    us = {k: min(v) for k, v in times.items()}
    for name, v in times.items():
        print(f'{name:20s} {us[name]:10.2f} us/batch   (rounds: {", ".join("%.2f" % t for t in v)})', flush=True)
    un, u1, uc = (us[k] for k in rows)
    print(f'n-step / 1-step      {un / u1:10.3f}', flush=True)
    print(f'n-step / composed    {un / uc:10.3f}', flush=True)
    H, W, C = rb.frame_shape
    print(json.dumps({'metric': 'replay n-step transitions us/batch (HBM store -> obs, next_obs, n-step return)',
                      'value': round(un, 2), 'unit': 'us/batch', 'batch': B, 'stack': K, 'stride': S, 'nstep': N,
                      'gamma': a.gamma, 'graph': a.graph, 'dtype': a.dtype, 'frame': [H, W, C], 'frames': a.frames,
                      'us_per_batch': {k: round(v, 2) for k, v in us.items()},
                      'rounds_us': {k: [round(t, 2) for t in v] for k, v in times.items()},
                      'nstep_over_1step': round(un / u1, 3), 'nstep_over_composed': round(un / uc, 3),
                      'fill_s': round(fill_s, 2),
                      'crop': None if cfg.crop is None else {'size': list(cfg.crop.size), 'pad': cfg.crop.pad,
                                                             'mirror': cfg.crop.mirror}}), flush=True)


def bench_priority(a, rb, cfg, fill_s):
    """--stack K --prioritized: the prioritized transition sample (priority draw + transition launch) next to
    the uniform one of this process, the draw alone and one update_priorities call, two rounds each."""
    import torch
    from blendtorch import ops
    dev, B, K, S = rb.device, a.batch, a.stack, a.stride
    kw = dict(stack=K, stride=S, next_keys=('reward',))
    if a.nstep:
        kw.update(nstep=a.nstep, gamma=a.gamma, done_key='done')
    # priorities over three decades on every slot, as TD errors would leave them
    g = torch.Generator(device=dev).manual_seed(1)
    for s in range(0, rb.capacity, 1024):
        idx = torch.arange(s, min(s + 1024, rb.capacity), device=dev)
        rb.update_priorities(idx, 10.0 ** (3 * torch.rand(idx.numel(), device=dev, generator=g) - 1.5))
    beta = torch.full((1,), a.beta, dtype=torch.float32, device=dev)

    def draw_eager():
        return ops.priority_draw(rb._levels, rb.capacity, rb._max_mass, B, seed=rb.seed, counter=0, beta=beta)

    if a.graph:
        prio = rb.graphed_transition_sampler(B, cfg, prioritized=True, beta=a.beta, **kw)
        uniform = rb.graphed_transition_sampler(B, cfg, **kw)
        draw_eager()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            drawn = draw_eager()

        def draw():
            graph.replay()
            return drawn
    else:
        prio = lambda: rb.sample_transitions(B, cfg, prioritized=True, beta=beta, **kw)   # noqa: E731
        uniform = lambda: rb.sample_transitions(B, cfg, **kw)                             # noqa: E731
        draw = draw_eager
    up_idx = prio()['index'].clone()
    up_prio = 10.0 ** (3 * torch.rand(B, device=dev, generator=g) - 1.5)

    def update():
        return rb.update_priorities(up_idx, up_prio)

    rows = {'prioritized sample': prio, 'uniform sample': uniform, 'priority draw': draw, 'update_priorities': update}
    times = {k: [] for k in rows}
    for _ in range(2):
        for name, fn in rows.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                b = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps * 1e6)
            del b
    us = {k: min(v) for k, v in times.items()}
    for name, v in times.items():
        print(f'{name:20s} {us[name]:10.2f} us/batch   (rounds: {", ".join("%.2f" % t for t in v)})', flush=True)
    print(f'prioritized - uniform {us["prioritized sample"] - us["uniform sample"]:9.2f} us', flush=True)
    H, W, C = rb.frame_shape
    print(json.dumps({'metric': 'prioritized replay transitions us/batch (priority draw + transition launch)',
                      'value': round(us['prioritized sample'], 2), 'unit': 'us/batch', 'batch': B, 'stack': K,
                      'stride': S, 'nstep': a.nstep, 'graph': a.graph, 'dtype': a.dtype, 'frame': [H, W, C],
                      'frames': a.frames, 'tree_levels': len(rb._levels), 'alpha': rb.priority_alpha, 'beta': a.beta,
                      'us_per_batch': {k: round(v, 2) for k, v in us.items()},
                      'rounds_us': {k: [round(t, 2) for t in v] for k, v in times.items()},
                      'prioritized_minus_uniform_us': round(us['prioritized sample'] - us['uniform sample'], 2),
                      'fill_s': round(fill_s, 2),
                      'crop': None if cfg.crop is None else {'size': list(cfg.crop.size), 'pad': cfg.crop.pad,
                                                             'mirror': cfg.crop.mirror}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=4096)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--fill', choices=['producers', 'synthetic'], default='synthetic')
    ap.add_argument('--dtype', choices=['float32', 'bfloat16'], default='float32')
    ap.add_argument('--graph', action='store_true', help='replay a HIP-graph-captured sampler')
    ap.add_argument('--sampler', choices=['fused', 'legacy'], default='fused',
                    help='fused: ONE launch (Philox draw + gather + decode + metadata); legacy: randint, '
                         'decode_gather and one index_select per metadata key (the round-1 path)')
    ap.add_argument('--crop', type=int, nargs=2, metavar=('H', 'W'), default=None,
                    help='sample through random H x W windows (fused sampler only)')
    ap.add_argument('--pad', type=int, default=0, help='replicate padding of the crop (random shift)')
    ap.add_argument('--mirror', type=float, default=0.0, help='probability of a mirrored window')
    ap.add_argument('--stack', type=int, default=0, metavar='K',
                    help='frame-stacked transitions: time the fused sample_transitions, the composed path '
                         '(2K gathers + cat) and the equal-bytes plain sample (synthetic fill)')
    ap.add_argument('--stride', type=int, default=1, metavar='S', help='frames per environment step (--stack)')
    ap.add_argument('--nstep', type=int, default=0, metavar='N',
                    help='with --stack: time the fused N-step sample, the fused 1-step sample and the N-step '
                         'batch composed on top of the 1-step sample')
    ap.add_argument('--gamma', type=float, default=0.99, help='discount of --nstep')
    ap.add_argument('--prioritized', action='store_true',
                    help='with --stack: time the prioritized transition sample next to the uniform one, the '
                         'priority draw alone and an update_priorities call')
    ap.add_argument('--alpha', type=float, default=0.6, help='priority exponent of --prioritized')
    ap.add_argument('--beta', type=float, default=0.4, help='importance-weight exponent of --prioritized')
    ap.add_argument('--frame', type=int, nargs=3, metavar=('H', 'W', 'C'), default=(480, 640, 4),
                    help='frame shape of the synthetic store')
    a = ap.parse_args()
    if a.crop is None and (a.pad or a.mirror):
        ap.error('--pad and --mirror need --crop')
    if a.crop is not None and a.sampler != 'fused':
        ap.error('--crop needs the fused sampler')
    if a.stack and (a.fill != 'synthetic' or a.sampler != 'fused'):
        ap.error('--stack needs the synthetic fill and the fused sampler')
    if a.nstep and not a.stack:
        ap.error('--nstep needs --stack')
    if a.prioritized and not a.stack:
        ap.error('--prioritized needs --stack')
    if a.fill != 'synthetic' and tuple(a.frame) != (480, 640, 4):
        ap.error('--frame needs the synthetic fill')

    import torch
    from blendtorch import btt, ops
    from blendtorch.btt.replay import DeviceReplayBuffer
    dev = torch.device('cuda', 0)
    rb = DeviceReplayBuffer(a.frames, device=dev, **(dict(priority_alpha=a.alpha, priority_stride=a.stride)
                                                     if a.prioritized else {}))
    t0 = time.perf_counter()
    if a.fill == 'synthetic':
        g = torch.Generator(device=dev).manual_seed(0)
        fh, fw, fc = a.frame
        for s in range(0, a.frames, 256):
            n = min(256, a.frames - s)
            ids = torch.arange(s, s + n, device=dev)
            meta = {'frameid': ids}
            if a.stack:   # an episode starts every 100 steps of every environment
                meta.update(first=((ids // a.stride) % 100 == 0).to(torch.uint8), reward=ids.to(torch.float32))
            if a.nstep:   # every other episode terminates (its last step), the others are truncated
                meta.update(done=((ids // a.stride) % 200 == 98).to(torch.uint8))
            rb.extend(torch.randint(0, 256, (n, fh, fw, fc), dtype=torch.uint8, device=dev, generator=g), **meta)
    else:
        from blendtorch.btt.gpu import DeviceLoader
        with btt.BlenderLauncher(producer='cubesim', num_instances=8, named_sockets=['DATA'], proto='ipc',
                                 start_port=24000, instance_args=[['--mode', 'rgba', '--shm', '32']] * 8) as bl:
            dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=64, max_items=a.frames, device=dev,
                              decode=ops.DecodeConfig.raw())
            rb.fill_from(dl, a.frames)
    torch.cuda.synchronize()
    fill_s = time.perf_counter() - t0
    crop = None if a.crop is None else ops.Crop(tuple(a.crop), mirror=a.mirror, pad=a.pad)
    cfg = ops.DecodeConfig.unit(channels='rgb', gamma=2.2, dtype=a.dtype, crop=crop)
    if a.prioritized:
        return bench_priority(a, rb, cfg, fill_s)
    if a.nstep:
        return bench_nstep(a, rb, cfg, fill_s)
    if a.stack:
        return bench_stack(a, rb, cfg, fill_s)

    def legacy():
        idx = torch.randint(0, len(rb), (a.batch,), device=dev)
        out = {'image': ops.decode_gather(rb.store, idx, cfg), 'index': idx}
        out.update({k: v.index_select(0, idx) for k, v in rb.meta.items()})
        return out

    if a.sampler == 'legacy':
        sample = legacy
    else:
        sample = rb.graphed_sampler(a.batch, cfg) if a.graph else (lambda: rb.sample(a.batch, cfg))
    for _ in range(a.warmup):
        sample()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        b = sample()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    H, W, C = rb.frame_shape
    if crop is not None:   # the window's bytes: pixels outside the frame re-read an edge pixel
        H, W = crop.size
    moved = a.batch * H * W * (C + cfg.cout * (4 if a.dtype == 'float32' else 2))   # bytes read + written
    print(json.dumps({'metric': 'replay images/s (HBM store -> gather+decode)', 'value': round(a.steps * a.batch / dt, 1),
                      'sampler': a.sampler, 'us_per_batch': round(dt / a.steps * 1e6, 2),
                      'effective_tbps': round(moved * a.steps / dt / 1e12, 3),
                      'unit': 'images/s', 'batch': a.batch, 'frames': a.frames, 'store_gb': round(rb.nbytes / 1e9, 2),
                      'fill': a.fill, 'fill_s': round(fill_s, 2), 'ms_per_batch': round(dt / a.steps * 1e3, 4),
                      'dtype': a.dtype, 'graph': a.graph, 'out_shape': list(b['image'].shape),
                      'crop': None if crop is None else {'size': list(crop.size), 'pad': crop.pad,
                                                         'mirror': crop.mirror}}), flush=True)


if __name__ == '__main__':
    main()
