"""The loader worker's cheaper per-frame path end to end: descriptors that are
only scanned on the worker (their metadata trees are built on the consumer's
thread), per-frame counters folded once per launch, and completion / post /
timing events reused from free lists.

Stamped cubesim frames (64x48 and 128x64, fixed pose) from 2 producers with
8-slot rings, batch 4, 40 batches -- more than an event free list keeps (32)
and five passes over every ring.  The slot mirror's size floor is lowered
(``slot_mirror=True``), so the frames take the same region-read launches as the
flagship stream.
"""
import os
import struct
import time

import numpy as np
import pytest
import torch

from blendtorch import btt, ops
from blendtorch.btt.gpu import DeviceLoader
from blendtorch.ops import DecodeConfig
from blendtorch.transport import shm

pytestmark = pytest.mark.gpu

B, NBATCH, SLOTS = 4, 40, 8
POSE = ['--rotation', '0.6', '0.4', '0.9']
HELD = 3   # csrc/transport/shmring.h SlotState
_cache = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    ops.hip_ext()  # must load: no silent fallback
    return torch.device('cuda', 0)


def _args(res, *extra):
    return ['--mode', 'rgba', '--resolution', res, '--stamp', *POSE, '--shm', str(SLOTS), *extra]


def _rgb():
    return DecodeConfig.unit(channels='rgb', gamma=2.2)


def _cpu_stream(port, res, each):
    """What RemoteIterableDataset delivers for the same producers' messages: {(btid, seq): item} of each
    producer's first `each` frames (one dataset per producer: seq 0 .. each - 1 of both), once per resolution."""
    if res not in _cache:
        items = {}
        with btt.BlenderLauncher(producer='cubesim', num_instances=2, named_sockets=['DATA'], start_port=port,
                                 proto='ipc', instance_args=[_args(res, '--shm-layout', 'interleaved')] * 2) as bl:
            for addr in bl.launch_info.addresses['DATA']:
                ds = btt.RemoteIterableDataset([addr], max_items=each, timeoutms=30000)
                for item in ds:
                    items[(int(item['btid']), int(item['seq']))] = item
        _cache[res] = items
    return _cache[res]


def _reference(frame, cfg, btid, seq):
    f = np.array(frame, copy=True)
    f.reshape(-1)[:16] = np.frombuffer(struct.pack('<2sHIQ', b'BT', btid, 0, seq), np.uint8)
    return ops.reference_decode(torch.from_numpy(f[None]), cfg, flip=[0])[0]


def _same(a, b):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    if isinstance(b, torch.Tensor):
        b = b.cpu().numpy()
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize('res', ['64x48', '128x64'])
def test_images_metadata_and_counters_over_many_launches(dev, free_port, res):
    # every (btid, seq) the GPU stream can deliver: it takes B * NBATCH frames in all
    cpu = _cpu_stream(free_port, res, B * NBATCH)
    assert set(cpu) == {(p, s) for p in range(2) for s in range(B * NBATCH)}
    frame = next(iter(cpu.values()))['image']           # fixed pose: every frame is this one plus its stamp
    meta_keys = set(next(iter(cpu.values()))) - {'image'}
    assert '_btshm' not in meta_keys and {'btid', 'seq', 'frameid', 'xy'} <= meta_keys
    seen = {}
    with btt.BlenderLauncher(producer='cubesim', num_instances=2, named_sockets=['DATA'], start_port=free_port + 5,
                             proto='ipc', instance_args=[_args(res)] * 2) as bl:
        # enough posted buffers that every batch can launch while half of them are still undelivered
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=B, max_items=B * NBATCH, device=dev,
                          decode=_rgb(), slot_mirror=True, prefetch=NBATCH // 2 + 4, timeoutms=30000)
        mid = None
        for n, b in enumerate(dl):
            assert set(b) == meta_keys | {'image'}, set(b)
            img = b['image'].cpu()
            for k in range(B):
                key = (int(b['btid'][k]), int(b['seq'][k]))
                assert key not in seen
                seen[key] = img[k]
                for name in meta_keys:
                    assert _same(b[name][k], cpu[key][name]), (key, name)
            # a snapshot at any moment, frames received since the last launch included (they are not in
            # the folded totals yet): never fewer frames than the launched batches hold, per-btid exact
            raw = dl.snapshot()
            assert raw['frames'] >= 4 * raw['batches'] >= 4 * (n + 1), raw
            assert sum(int(v) for v in raw['frames_per_btid'].values()) == raw['frames'], raw
            if n + 1 == NBATCH // 2:
                # mid-stream, at rest: the loader has taken its B * NBATCH frames and every one of them is
                # in a launched batch, while half the batches are still to be delivered
                t0 = time.monotonic()
                mid = dl.snapshot()
                while mid['batches'] < NBATCH and time.monotonic() - t0 < 20:
                    time.sleep(0.001)
                    mid = dl.snapshot()
        st = dict(dl.stats)
    for s in (mid, st):
        assert s['frames'] == 4 * s['batches'] == B * NBATCH, s
        assert sum(int(v) for v in s['frames_per_btid'].values()) == s['frames'], s
        assert {int(k) for k in s['frames_per_btid']} <= {0, 1}   # (a producer that starts late may supply none)
    assert st['bad'] == 0 and st['shm_torn'] == 0 and st['shm_frames'] == B * NBATCH, st
    assert st['direct_batches'] == st['batches'] and st['staged_frames'] == 0, st
    assert 1 <= st['launches'] <= st['batches'] and st['delta_frames'] > 0, st
    assert len(seen) == B * NBATCH and set(seen) <= set(cpu)
    for key, img in seen.items():
        assert torch.equal(img, _reference(frame, _rgb(), *key)), key


def test_close_with_work_in_flight_returns_every_slot(dev, free_port):
    with btt.BlenderLauncher(producer='cubesim', num_instances=2, named_sockets=['DATA'], start_port=free_port,
                             proto='ipc', instance_args=[_args('64x48')] * 2) as bl:
        addrs = bl.launch_info.addresses['DATA']
        dl = DeviceLoader(addrs, batch_size=B, device=dev, decode=_rgb(), slot_mirror=True, prefetch=8)
        it = iter(dl)
        for _ in range(3):
            next(it)
        it.close()          # launches in flight (8 posted buffers), descriptors queued in the sockets
        assert dl.stats['bad'] == 0 and dl.stats['shm_torn'] == 0, dl.stats
        rings = [f for f in os.listdir('/dev/shm') if f.startswith('blendtorch-')]
        assert len(rings) == 2
        for name in rings:
            states = np.array(shm._open(name).states) & 3
            assert not (states == HELD).any(), (name, states)
        # the producers go on: a second loader streams five passes over both rings
        dl2 = DeviceLoader(addrs, batch_size=B, max_items=B * 20, device=dev, decode=_rgb(), slot_mirror=True,
                           timeoutms=30000)
        got = 0
        for b in dl2:
            assert b['image'].shape == (B, 3, 48, 64)
            got += 1
        assert got == 20 and dl2.stats['bad'] == 0 and dl2.stats['shm_torn'] == 0, dl2.stats
        for name in rings:
            states = np.array(shm._open(name).states) & 3
            assert not (states == HELD).any(), (name, states)
    torch.cuda.synchronize(dev)
