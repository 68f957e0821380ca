"""What a crop inside the fused decode is worth on the streaming path.

The headline configuration of bench.py (cubesim RGBA 640x480 producers over
shared-memory rings, batch 8, ``DecodeConfig.unit(channels='rgb', gamma=2.2)``,
no consumer, the producer count bench.py plans) run with no crop and with
``ops.Crop`` windows of 448x448 and 224x224 (``mirror=0.5``), 448x448 also with
``x_align=16``.  The decode kernel reads only the window's rows and columns of
every host frame, so a window moves ``h*w / (H*W)`` of the bytes over PCIe.

Every run is a child process of its own (fresh producers, fresh HIP runtime);
``resized224`` and ``resize224_full`` are ``ops.ResizedCrop((224, 224))`` rows: the
default random window (``mirror=0.5``) and the whole frame resized; their
``bytes_share`` is the windows' measured share of the frames, an upper bound of
what is read once the vertical scale exceeds 2.
the configurations alternate, ``--repeats`` rounds.  One JSON row per run on
stdout: images/s over the timed steps, the loader's ``h2d_gbytes_per_s`` and
``gpu_us_per_image`` over the same window, ``direct_batches``, CPU us per frame.

    python benchmarks/crop_stream.py [--steps 8000] [--warmup 100] [--repeats 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'pytorch-blender_amd'))

CONFIGS = {
    'none': None,
    'crop448': dict(size=(448, 448), mirror=0.5),
    'crop224': dict(size=(224, 224), mirror=0.5),
    'crop448_x16': dict(size=(448, 448), mirror=0.5, x_align=16),
    # resized crops (ops.ResizedCrop: the frame's window resized inside the decode): the default random
    # scale / ratio, and the whole frame (a plain Resize)
    'resized224': dict(resize=True, size=(224, 224), mirror=0.5),
    'resize224_full': dict(resize=True, size=(224, 224), mode='full'),
}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=8000)
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--resolution', default='640x480')
    ap.add_argument('--shm', type=int, default=48)
    ap.add_argument('--configs', default=','.join(CONFIGS), help='comma-separated subset of ' + ', '.join(CONFIGS))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def child(args):
    import bench   # the headline's own planning: cpu_budget, ensure_built
    bench.ensure_built()
    from blendtorch.utils import ensure_hw_queues
    hw_queues = ensure_hw_queues(8)
    import torch
    from blendtorch import btt, ops
    from blendtorch.btt.gpu import DeviceLoader
    from blendtorch.parallel import plan_rank_resources

    torch.cuda.set_device(0)
    device = torch.device('cuda', 0)
    cpus, budget, pin = bench.cpu_budget()
    W, H = (int(v) for v in args.resolution.lower().split('x'))
    try:
        st = os.statvfs('/dev/shm')
        shm_free = st.f_bavail * st.f_frsize
    except OSError:
        shm_free = None
    rp = plan_rank_resources(0, 0, 1, 1, cpus, budget, pin, producers=0, dist_mode='shard', shm_slots=args.shm,
                             shm_free_bytes=shm_free, frame_bytes=W * H * 4)
    if rp['numa_local']:
        os.sched_setaffinity(0, rp['domain'])
    nprod, shm_slots = rp['producers'], rp['shm_slots']
    spec = CONFIGS[args.child]
    resize = bool(spec) and spec.get('resize', False)
    crop = None if resize or not spec else ops.Crop(**spec)
    rc = ops.ResizedCrop(**{k: v for k, v in spec.items() if k != 'resize'}) if resize else None
    decode = ops.DecodeConfig.unit(channels='rgb', gamma=2.2, crop=crop, resize=rc)
    WARM_RESERVE = 2000
    total = args.warmup + args.steps + WARM_RESERVE
    with btt.BlenderLauncher(producer='cubesim', num_instances=nprod, named_sockets=['DATA'],
                             start_port=rp['start_port'], proto='ipc', seed=0, cpu_affinity=rp['affinity'],
                             instance_args=[['--mode', 'rgba', '--sndhwm', '10', '--resolution', f'{W}x{H}',
                                             '--shm', str(shm_slots), '--codec', 'none']
                                            for _ in range(nprod)]) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=args.batch, decode=decode, device=device,
                          max_items=total * args.batch, timeoutms=60000)
        it = iter(dl)
        seen, n_warm, t_warm = set(), 0, time.time()
        while n_warm < args.warmup or (len(seen) < nprod and n_warm < WARM_RESERVE and time.time() - t_warm < 20):
            b = next(it)
            seen.update(int(x) for x in b['btid'])
            n_warm += 1
        torch.cuda.synchronize()
        cg0, ru0, snap0 = bench.cgroup_cpu_stat(), os.times(), dl.snapshot()
        t0 = time.perf_counter()
        area = 0
        for _ in range(args.steps):
            b = next(it)
            if rc is not None:   # the windows' share of the frames (host metadata: no device work)
                area += int((b['window'][:, 2].long() * b['window'][:, 3].long()).sum())
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        snap1, ru1, cg1 = dl.snapshot(), os.times(), bench.cgroup_cpu_stat()
        shape = tuple(b['image'].shape)
        it.close()
    win = DeviceLoader.window(snap0, snap1)
    frames = args.steps * args.batch
    cpu = {'consumer': round(((ru1.user - ru0.user) + (ru1.system - ru0.system)) * 1e6 / frames, 2)}
    if 'usage_usec' in cg0 and 'usage_usec' in cg1:
        cpu['total'] = round((cg1['usage_usec'] - cg0['usage_usec']) / frames, 2)
    hh, ww = crop.size if crop else (H, W)
    share = area / (frames * H * W) if rc is not None else hh * ww / (H * W)
    print(json.dumps({
        'config': args.child, 'crop': spec, 'images_per_s': round(frames / elapsed, 1),
        'h2d_gbytes_per_s': round(win['h2d_gbytes_per_s'], 2),
        'gpu_us_per_image': None if win['gpu_us_per_image'] is None else round(win['gpu_us_per_image'], 2),
        'direct_batches': snap1['direct_batches'] - snap0['direct_batches'], 'batches': args.steps,
        'planar_frames': snap1['planar_frames'] - snap0['planar_frames'],
        'images_per_launch': None if win['images_per_launch'] is None else round(win['images_per_launch'], 2),
        'bytes_share': round(share, 4), 'out_shape': shape, 'cpu_us_per_frame': cpu,
        'producers': nprod, 'hw_queues': hw_queues, 'steps': args.steps, 'warmup': n_warm,
        'backlog_covers_window': win.get('backlog_covers_window'), 'elapsed_s': round(elapsed, 4)}), flush=True)
    return 0


def main(argv=None):
    args = parse_args(argv)
    if args.child:
        return child(args)
    names = [n for n in args.configs.split(',') if n]
    bad = [n for n in names if n not in CONFIGS]
    if bad:
        raise SystemExit(f'unknown configs {bad}; choose from {list(CONFIGS)}')
    base = [sys.executable, str(Path(__file__).resolve()), '--steps', str(args.steps), '--warmup', str(args.warmup),
            '--batch', str(args.batch), '--resolution', args.resolution, '--shm', str(args.shm)]
    for rep in range(args.repeats):
        for n in names:   # alternating: one run of every configuration per round
            r = subprocess.run(base + ['--child', n], stdout=subprocess.PIPE, text=True, timeout=300)
            rows = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
            if r.returncode != 0 or not rows:
                print(json.dumps({'config': n, 'repeat': rep, 'error': f'exit {r.returncode}'}), flush=True)
                return 1          # a failed run ends the series: nothing more is started on the GPU
            row = json.loads(rows[-1])
            row['repeat'] = rep
            print(json.dumps(row), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
