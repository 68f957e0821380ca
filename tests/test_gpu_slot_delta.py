"""Region reads with a slot mirror: the kernel (csrc/gpu/kernels.hip
``decode_delta``) and the stream loader (``DeviceLoader(slot_mirror=True)``).

Kernel: B = 3 images of H = 6, W = 64 / 128 per launch -- image 0 without a
mirror, image 1 flipped, per-image destinations.  The host frames (pinned,
device-mapped) hold the true bytes inside each image's region and POISON
outside it; the mirrors hold the true bytes outside and poison inside.  The
outputs, compared bit for bit with ``ops.reference_decode`` of the true frames
over their whole guard-filled buffers, therefore prove that nothing outside a
region is taken from the host and nothing inside from the mirror; afterwards
every mirror equals its true frame and the guards around the mirrors hold.

Loader: stamped 64x48 cubesim frames from 4-slot rings, batch 4, 10 batches.
"""
import os
import struct

import numpy as np
import pytest
import torch

from decode_oracle import MirrorLaunch, frames
from blendtorch import btt, ops
from blendtorch.btt.gpu import DeviceLoader
from blendtorch.ops import DecodeConfig
from blendtorch.transport import shm, zmq

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'bfloat16', 'float16', 'uint8')
LAYOUTS = ('nchw', 'nhwc')
H = 6


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    ops.hip_ext()  # must load: no silent fallback
    return torch.device('cuda', 0)


def _vcfg(channels, dtype, layout):
    if dtype == 'uint8':
        return DecodeConfig(channels=channels, gamma=2.2, dtype='uint8', layout=layout)
    return DecodeConfig.densityopt(channels=channels, gamma=2.2, dtype=dtype, layout=layout)


def _regions(W):
    """(y0, y1, x0, x1) in stored rows / pixel columns, inclusive."""
    right = W - 64
    return {
        'empty': (0, -1, 0, -1),
        'whole': (0, H - 1, 0, W - 1),
        'corner block': (0, 0, right, W - 1),
        'row band': (2, 3, 0, W - 1),
        'right bottom': (3, H - 1, right, W - 1),
    }


def _inside(region, shape):
    y0, y1, x0, x1 = region
    m = np.zeros(shape, bool)
    if y1 >= y0:
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def _launch(d, B=None, regions=None, cmap=None, W=None):
    regions = d.regions if regions is None else regions
    B = d.B if B is None else B
    ops.hip_ext().decode_delta(
        [d.host_dev + b * d.fb for b in range(min(B, d.B))],
        [0 if b == 0 or b >= d.B else d.mir.data_ptr() + d.mir_off[b] for b in range(B)],
        [v for b in range(B) for v in regions[min(b, d.B - 1)]], 0, ops.device_lut(d.cfg, d.dev).data_ptr(),
        B, d.H, d.W if W is None else W, d.Cin, d.cfg.cout, list(d.cfg.cmap) if cmap is None else cmap, 0,
        ops.OUT_DTYPES[d.cfg.dtype], ops.LAYOUTS[d.cfg.layout], ops._stream(d.dev),
        dsts=[d.outs[k].data_ptr() + off for k, off in d.dst][:B], flip_bits=[d.flip_bits])


def _Delta(dev, store, cfg, regions, flip_bits=0b010):
    """One decode_delta launch; image 0 has no mirror, images 1.. use ``regions``."""
    d = MirrorLaunch(dev, store, cfg, [_inside(r, store.shape[1:]) for r in regions], _launch, flip_bits)
    d.regions = [(0, -1, 0, -1)] + list(regions)
    d.label = f'regions {d.regions}'
    return d


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_regions_from_host_rest_from_mirror(dev, dtype, layout):
    for W in (64, 128):
        reg = _regions(W)
        names = list(reg)
        for Cin, ch in ((3, 'bgr'), (4, 'rgba'), (4, 'rgb')):
            store = frames(3, H, W, Cin, seed=500 + W + Cin)
            cfg = _vcfg(ch, dtype, layout)
            for i, name in enumerate(names):
                other = names[(i + 2) % len(names)]          # image 2 takes another kind of region
                d = _Delta(dev, store, cfg, [reg[name], reg[other]])
                try:
                    d.launch()
                    d.check(f'{name} / {other}')
                finally:
                    d.close()


def test_rejections_launch_nothing(dev):
    cfg = _vcfg('rgb', 'float32', 'nchw')
    store = frames(3, H, 128, 4, seed=77)
    d = _Delta(dev, store, cfg, [(0, 1, 64, 127), (2, 3, 0, 127)])
    try:
        for regions in ([(0, -1, 0, -1), (0, 1, 32, 127), (2, 3, 0, 127)],        # x0 off the 64-pixel grid
                        [(0, -1, 0, -1), (0, 1, 64, 100), (2, 3, 0, 127)],        # x1 + 1 off the grid, not the edge
                        [(0, -1, 0, -1), (0, H, 64, 127), (2, 3, 0, 127)],        # leaves the frame
                        [(0, -1, 0, -1), (0, 1, 64, 128), (2, 3, 0, 127)]):
            with pytest.raises((RuntimeError, ValueError)):
                d.launch(regions=regions)
            d.untouched()
        with pytest.raises((RuntimeError, ValueError)):
            d.launch(B=65)                                                         # B > 64
        d.untouched()
        with pytest.raises((RuntimeError, ValueError)):
            d.launch(cmap=[0, 1, 4, 0])                                            # channel 4 of 4
        d.untouched()
        d.launch()
        d.check('after the rejections')
    finally:
        d.close()
    # W % 64 != 0: only regions spanning full rows
    store = frames(3, H, 96, 4, seed=78)
    d = _Delta(dev, store, cfg, [(0, 1, 0, 95), (0, -1, 0, -1)])
    try:
        with pytest.raises((RuntimeError, ValueError)):
            d.launch(regions=[(0, -1, 0, -1), (0, 1, 64, 95), (0, -1, 0, -1)])
        d.untouched()
        d.launch()
        d.check('full rows at W = 96')
    finally:
        d.close()


# ---- loader -------------------------------------------------------------------------------------------------------

B, NBATCH = 4, 10
FH, FW = 48, 64
POSE = ['--rotation', '0.6', '0.4', '0.9']
_frame_cache = {}


def _args(*extra):
    return ['--mode', 'rgba', '--resolution', f'{FW}x{FH}', '--stamp', *extra]


def _fixed_frame(port):
    """The fixed pose's H x W x 4 frame through the CPU path, once."""
    if 'f' not in _frame_cache:
        with btt.BlenderLauncher(producer='cubesim', num_instances=1, named_sockets=['DATA'], start_port=port,
                                 proto='ipc', instance_args=[_args(*POSE, '--shm', '4', '--shm-layout',
                                                                   'interleaved')]) as bl:
            s = zmq.Context().socket(zmq.PULL)
            s.connect(bl.launch_info.addresses['DATA'][0])
            assert s.poll(20000)
            _frame_cache['f'] = np.ascontiguousarray(shm.resolve(s.recv_pyobj())['image'])
            s.close()
        _frame_cache['f'].setflags(write=False)
    return _frame_cache['f']


def _reference(frame, cfg, btid, seq):
    f = frame.copy()
    f.reshape(-1)[:16] = np.frombuffer(struct.pack('<2sHIQ', b'BT', btid, 0, seq), np.uint8)
    return ops.reference_decode(torch.from_numpy(f[None]), cfg, flip=[0])[0]


def _run(dev, port, cfg, producers, seed=11, nbatch=NBATCH, **kw):
    """{(btid, seq): decoded image (cpu)} of B * nbatch frames, and the loader's stats."""
    out = {}
    with btt.BlenderLauncher(producer='cubesim', num_instances=len(producers), named_sockets=['DATA'],
                             start_port=port, proto='ipc', seed=seed, instance_args=producers) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=B, max_items=B * nbatch, device=dev,
                          decode=cfg, **kw)
        for b in dl:
            img = b['image'].cpu()
            for k in range(B):
                out[(int(b['btid'][k]), int(b['seq'][k]))] = img[k]
        st = dict(dl.stats)
    assert len(out) == B * nbatch and st['bad'] == 0 and st['batches'] == nbatch and st['shm_torn'] == 0
    return out, st


def _rgb():
    return DecodeConfig.unit(channels='rgb', gamma=2.2)


def test_stream_equals_the_unmirrored_stream(dev, free_port):
    """One producer, random poses from a fixed seed: arrival order is publishing order in both runs."""
    prod = [_args('--shm', '4')]
    on, st = _run(dev, free_port, _rgb(), prod, slot_mirror=True)
    off, sto = _run(dev, free_port + 5, _rgb(), prod, slot_mirror=False)
    assert set(on) == set(off) == {(0, s) for s in range(B * NBATCH)}
    for key in on:
        assert torch.equal(on[key], off[key]), key
    assert len({v.numpy().tobytes()[64:] for v in on.values()}) > 4                       # the poses do differ
    assert st['delta_frames'] > 0 and st['mirror_bytes'] == 4 * FH * FW * 3, st
    assert st['image_bytes'] < B * NBATCH * FH * FW * 3, st
    assert st['direct_batches'] == st['batches'] and st['staged_frames'] == 0, st
    assert sto['delta_frames'] == 0 and sto['mirror_bytes'] == 0, sto
    assert sto['image_bytes'] == FH * FW * (3 * sto['planar_frames'] + 4 * (B * NBATCH - sto['planar_frames'])), sto


def test_default_leaves_small_frames_unmirrored(dev, free_port):
    """slot_mirror=None: frames below the automatic size bound are read whole."""
    got, st = _run(dev, free_port, _rgb(), [_args('--shm', '4')])
    assert st['delta_frames'] == 0 and st['mirror_bytes'] == 0, st


def test_mixed_fleet_matches_reference_and_stays_direct(dev, free_port):
    frame = _fixed_frame(free_port)
    # all three paced, the rings below the inline producer (two unpaced rings deliver every frame before
    # the inline producer's first one arrives): of the 120 frames each ring supplies about 30, so each
    # passes over its 4 slots several times
    prods = [_args(*POSE, '--shm', '4', '--fps', '100'), _args(*POSE, '--shm', '4', '--fps', '100'),
             _args(*POSE, '--fps', '200')]
    got, st = _run(dev, free_port + 5, _rgb(), prods, nbatch=30, slot_mirror=True)
    assert st['direct_batches'] == st['batches'], st
    assert st['delta_frames'] > 0 and st['shm_frames'] < st['frames'], st                  # rings and the inline producer
    assert {k[0] for k in got} == {0, 1, 2}
    for key, img in got.items():
        assert torch.equal(img, _reference(frame, _rgb(), *key)), key


def test_rgba_decode_mirrors_interleaved_slots(dev, free_port):
    frame = _fixed_frame(free_port)
    cfg = DecodeConfig.unit(channels='rgba')
    got, st = _run(dev, free_port + 5, cfg, [_args(*POSE, '--shm', '4')], slot_mirror=True)
    assert st['planar_frames'] == 0 and st['delta_frames'] > 0 and st['mirror_bytes'] == 4 * FH * FW * 4, st
    assert st['image_bytes'] < B * NBATCH * FH * FW * 4, st
    for key, img in got.items():
        assert img.shape == (4, FH, FW) and torch.equal(img, _reference(frame, cfg, *key)), key


def test_budget_of_one_byte_reads_whole_frames(dev, free_port):
    frame = _fixed_frame(free_port)
    got, st = _run(dev, free_port + 5, _rgb(), [_args(*POSE, '--shm', '4')], slot_mirror=True, slot_mirror_max_bytes=1)
    assert st['delta_frames'] == 0 and st['mirror_bytes'] == 0, st
    assert st['image_bytes'] == FH * FW * (3 * st['planar_frames'] + 4 * (B * NBATCH - st['planar_frames'])), st
    for key, img in got.items():
        assert torch.equal(img, _reference(frame, _rgb(), *key)), key


def test_early_close_mid_stream(dev, free_port):
    with btt.BlenderLauncher(producer='cubesim', num_instances=2, named_sockets=['DATA'], start_port=free_port,
                             proto='ipc', instance_args=[_args('--shm', '4')] * 2) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=B, device=dev, decode=_rgb(), prefetch=8,
                          slot_mirror=True)
        it = iter(dl)
        for _ in range(10):
            next(it)
        it.close()
        st = dl.stats
        assert st['bad'] == 0 and st['shm_torn'] == 0 and st['direct_batches'] == st['batches'] >= 10, st
        assert st['delta_frames'] > 0, st
    assert not [f for f in os.listdir('/dev/shm') if f.startswith('blendtorch-')]
    torch.cuda.synchronize(dev)
