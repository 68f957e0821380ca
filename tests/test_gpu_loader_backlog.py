"""Batches held behind queued launches (csrc/gpu/launch_policy.h): out of posted
buffers the loader no longer forces a pending batch out while
max(1, launch_depth) launches are in flight; the held batches leave together
when one retires.  Whatever the grouping, the stream must deliver every item,
each image must be the decode of the frame its metadata names, and nothing
may hang.

Two ``cubesim --stamp --shm 8`` producers, 64x48 RGBA frames (the block grid
holds: W % 64 == 0, bands of 2 rows), random poses, RGB fp32 CHW decode on the
slot-mirror block path.  Batches of ONE image: with ``launch_depth`` 0 every
pending batch keeps its frames' ring slots until 64 images wait or the
buffers run out, and 8 buffers of larger batches would hold all 16 slots with
nothing in flight.  101 items are no multiple of 2 or 8 buffers, so the stream
ends with a partial group held.  The oracle is ``ops.reference_decode`` of
the same producers' frames through the CPU path (seeded launcher: frame
``seq`` of a producer is the same in every run), computed once.

At this frame size a kernel takes microseconds, so how many batches share a
launch is not forced in the fast-consumer cases: only 1 <= launches <= batches
is asserted there.  The last case paces the producers and lets the consumer
sleep between batches: nothing is in flight when a batch is assembled, and
every batch launches alone.
"""
import time
from collections import defaultdict

import numpy as np
import pytest
import torch

from blendtorch import btt, ops
from blendtorch.btt.gpu import DeviceLoader
from blendtorch.ops import DecodeConfig
from blendtorch.transport import shm, zmq

pytestmark = pytest.mark.gpu

SEED = 23
ITEMS = 101
BASE = ['--mode', 'rgba', '--resolution', '64x48', '--stamp', '--shm', '8']
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


def _stream(dev, port, producers, batch, items, pause=0.0, **kw):
    """Delivered (key, image) pairs in order, and the loader's stats."""
    got = []
    with _launcher(port, producers) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=batch, max_items=items, device=dev,
                          decode=_cfg(), slot_mirror=True, timeoutms=20000, **kw)
        for b in dl:
            img = b['image'].cpu()
            assert img.shape == (batch, 3, 48, 64) and img.dtype == torch.float32
            for k in range(batch):
                got.append(((int(b['btid'][k]), int(b['seq'][k])), img[k]))
            if pause:
                time.sleep(pause)
        st = dict(dl.stats)
    return got, st


def _check(got, st, true, items, batch):
    assert len(got) == items, (len(got), st)                                    # every item, within the timeout
    for key, img in got:
        assert torch.equal(img, true[key]), key                                 # the frame its metadata names
    seen = defaultdict(list)
    for (btid, seq), _ in got:
        seen[btid].append(seq)
    for seqs in seen.values():
        assert seqs == sorted(set(seqs)), seqs                                  # per producer in order, no duplicates
    assert st['bad'] == 0 and st['shm_torn'] == 0, st
    assert st['frames'] == items and st['batches'] == items // batch, st
    assert st['direct_batches'] == st['batches'] and st['block_frames'] > 0, st  # in place, on the block path
    assert 1 <= st['launches'] <= st['batches'], st


@pytest.mark.parametrize('prefetch', [2, 8])
@pytest.mark.parametrize('launch_depth', [0, 1, 2])
def test_backlogged_stream_delivers_every_frame(dev, free_port, launch_depth, prefetch):
    true = _reference(free_port)
    got, st = _stream(dev, free_port + 5, [BASE] * 2, 1, ITEMS, launch_depth=launch_depth, prefetch=prefetch)
    _check(got, st, true, ITEMS, 1)


def test_slow_consumer_launches_every_batch_alone(dev, free_port):
    """Paced producers (a frame every 2.5 ms between them, at most the two
    rings' 16 frames -- two batches, which launch_depth 2 lets go at once --
    ready at the start) and a consumer that sleeps between batches: every
    batch is assembled with no launch in flight and goes out on its own."""
    true = _reference(free_port)
    paced = [BASE + ['--fps', '200']] * 2
    got, st = _stream(dev, free_port + 5, paced, 8, 80, pause=0.002, launch_depth=2, prefetch=8)
    _check(got, st, true, 80, 8)
    assert st['launches'] == st['batches'] == 10, st
