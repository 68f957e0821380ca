"""Block masks that hold only what the render stored into (csrc/sim/raster.h:
``written``), end to end through the slot mirror: the loader reads the set
blocks of a frame from the ring and everything else from its copy in HBM, so
a block missing from a mask shows as stale pixels in a delivered image.

Two ``cubesim --stamp --shm 8`` producers, 128x48 RGBA frames (two column
blocks, bands of 2 rows), random poses, RGB fp32 CHW decode on the block path,
batches of one image, 2 and 8 output buffers.  136 items are more than 8 laps
over the two rings' 16 slots, so every slot is rewritten many times from a
mirror that only ever took masked reads after its first frame.  Every
delivered image must equal ``ops.reference_decode`` of the frame its metadata
names (seeded launcher: frame ``seq`` of a producer is the same in every run,
whatever its worker count), read once through the CPU path.  One case forces
three render workers."""
from collections import defaultdict

import numpy as np
import pytest
import torch

from blendtorch import btt, ops
from blendtorch.btt.gpu import DeviceLoader
from blendtorch.ops import DecodeConfig
from blendtorch.transport import shm, zmq

pytestmark = pytest.mark.gpu

SEED = 31
ITEMS = 136
H, W = 48, 128
BASE = ['--mode', 'rgba', '--resolution', f'{W}x{H}', '--stamp', '--shm', '8']
_true = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    ops.hip_ext()  # must load: no silent fallback
    return torch.device('cuda', 0)


def _cfg():
    return DecodeConfig.unit(channels='rgb', gamma=2.2)


def _launcher(port, producers):
    return btt.BlenderLauncher(producer='cubesim', num_instances=2, named_sockets=['DATA'], start_port=port,
                               proto='ipc', seed=SEED, instance_args=producers)


def _reference(port):
    """{(btid, seq): fp32 reference decode} of the first ITEMS frames of each
    producer (either may supply up to all of a run), read through the CPU path."""
    if not _true:
        raw = {}
        with _launcher(port, [BASE] * 2) as bl:
            for addr in bl.launch_info.addresses['DATA']:
                s = zmq.Context().socket(zmq.PULL)
                s.connect(addr)
                for _ in range(ITEMS):
                    assert s.poll(20000)
                    msg = shm.resolve(s.recv_pyobj(), strict=True)
                    raw[(int(msg['btid']), int(msg['seq']))] = np.ascontiguousarray(msg['image'])
                s.close()
        keys = sorted(raw)
        assert len(keys) == 2 * ITEMS and len({raw[k].tobytes()[16:] for k in keys}) > ITEMS   # the poses do differ
        ref = ops.reference_decode(torch.from_numpy(np.stack([raw[k] for k in keys])), _cfg(), flip=[0] * len(keys))
        _true.update({k: ref[i] for i, k in enumerate(keys)})
    return _true


def _stream(dev, port, producers, **kw):
    got = []
    with _launcher(port, producers) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=1, max_items=ITEMS, device=dev,
                          decode=_cfg(), slot_mirror=True, timeoutms=20000, **kw)
        for b in dl:
            img = b['image'].cpu()
            assert img.shape == (1, 3, H, W) and img.dtype == torch.float32
            got.append(((int(b['btid'][0]), int(b['seq'][0])), img[0]))
        st = dict(dl.stats)
    return got, st


def _check(got, st, true):
    assert len(got) == ITEMS, (len(got), st)                                    # every item, within the timeout
    stale = [key for key, img in got if not torch.equal(img, true[key])]
    assert not stale, (len(stale), stale[:8])                                   # the frame its metadata names
    seen = defaultdict(list)
    for (btid, seq), _ in got:
        seen[btid].append(seq)
    for seqs in seen.values():
        assert seqs == sorted(set(seqs)), seqs                                  # per producer in order, no duplicates
    assert st['bad'] == 0 and st['shm_torn'] == 0, st
    assert st['frames'] == ITEMS and st['block_frames'] > 0, st                 # on the block path


@pytest.mark.parametrize('prefetch', [2, 8])
def test_masked_reads_deliver_the_named_frame(dev, free_port, prefetch):
    true = _reference(free_port)
    got, st = _stream(dev, free_port + 5, [BASE] * 2, prefetch=prefetch)
    _check(got, st, true)


def test_three_render_workers(dev, free_port):
    true = _reference(free_port)
    got, st = _stream(dev, free_port + 5, [BASE + ['--render-threads', '3']] * 2, prefetch=8)
    _check(got, st, true)
