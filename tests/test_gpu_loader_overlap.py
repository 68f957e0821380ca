"""Direct-path decode launches rotating over two HIP streams (DeviceLoader
``decode_streams``): batches still arrive in launch order with the pixels
their metadata names, decode to the same bits as on one stream, respect the
consumer's post events, and a loader closed with launches in flight on both
streams leaves nothing behind.  64x48 cubesim frames throughout."""
import os
from collections import defaultdict

import numpy as np
import pytest
import torch

from blendtorch import btt, ops
from blendtorch.btt.gpu import DeviceLoader

pytestmark = pytest.mark.gpu

RES = ['--mode', 'rgba', '--resolution', '64x48']
POSE = ['--rotation', '0.3', '0.5', '0.7']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    ops.hip_ext()
    return torch.device('cuda', 0)


def _launcher(port, producers):
    return btt.BlenderLauncher(producer='cubesim', num_instances=len(producers), named_sockets=['DATA'],
                               start_port=port, proto='ipc', instance_args=producers)


def _stamps(img):
    """(btid, seq) stamped into the first 16 bytes of every raw image of a batch."""
    head = img.reshape(img.shape[0], -1)[:, :16].cpu().numpy()
    out = []
    for st in head:
        assert bytes(st[:2]) == b'BT'
        out.append((int(st[2]) | (int(st[3]) << 8), int(np.frombuffer(st[8:16].tobytes(), '<u8')[0])))
    return out


@pytest.mark.parametrize('host_sync', [True, False], ids=['host', 'gpu'])
@pytest.mark.parametrize('decode_streams', [1, 2])
def test_integrity_under_overlap(dev, free_port, decode_streams, host_sync):
    """Every image carries the stamp of the metadata it is delivered with, per
    producer in order and without duplicates, whichever stream decoded it."""
    args = [RES + ['--stamp', '--shm', '8']] * 4
    with _launcher(free_port, args) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=4, max_items=2000, device=dev,
                          decode=ops.DecodeConfig.raw(), prefetch=4, launch_depth=2, host_sync=host_sync,
                          decode_streams=decode_streams)
        seen = defaultdict(list)
        for b in dl:
            for k, (btid, seq) in enumerate(_stamps(b['image'])):
                assert btid == int(b['btid'][k]) and seq == int(b['seq'][k]), (btid, seq, b['btid'][k], b['seq'][k])
                seen[btid].append(seq)
        st = dl.stats
    assert sum(len(v) for v in seen.values()) == 2000
    for seqs in seen.values():
        assert len(seqs) == len(set(seqs))             # no duplicates
        assert sorted(seqs) == seqs                     # per-producer order preserved
    assert st['bad'] == 0 and st['shm_torn'] == 0, st
    assert st['batches'] == 500 and st['direct_batches'] == st['batches'], st


_CFGS = {
    'f32-nchw': lambda: ops.DecodeConfig.unit(channels='rgb', gamma=2.2),
    'bf16-nhwc': lambda: ops.DecodeConfig.unit(channels='rgb', gamma=2.2, dtype='bfloat16', layout='nhwc'),
}
_first = {}     # cfg name -> first image of the one-stream run of the fixed pose (computed once, read-only)


def _fixed_pose_run(dev, port, cfg, producers, nbatch, **kw):
    with _launcher(port, producers) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=4, max_items=4 * nbatch, device=dev,
                          decode=cfg, **kw)
        imgs = [b['image'].clone() for b in dl]
        st = dict(dl.stats)
    assert len(imgs) == nbatch and st['bad'] == 0 and st['direct_batches'] == st['batches'] == nbatch, st
    return imgs, st


def _one_stream_image(dev, port, name):
    if name not in _first:
        # 32 frames over 2 x 8 ring slots: a producer can fill its ring before the loader maps it and leaves
        # its hint, so only frames past the rings' capacity are sure to be planar (16 frames gave none, once)
        imgs, st = _fixed_pose_run(dev, port, _CFGS[name](), [RES + POSE + ['--shm', '8']] * 2, 8, decode_streams=1)
        assert st['planar_frames'] > 0, st
        assert all(torch.equal(i, imgs[0][0]) for b in imgs for i in b)   # one pose: one image
        _first[name] = imgs[0][0]
    return _first[name]


@pytest.mark.parametrize('name', list(_CFGS))
def test_two_streams_decode_the_same_bits(dev, free_port, name):
    """Two fixed-pose ring producers, RGB decode (the Cin = 3 planar read on
    both streams): every image equals the one-stream run's."""
    ref = _one_stream_image(dev, free_port, name)
    imgs, st = _fixed_pose_run(dev, free_port + 5, _CFGS[name](), [RES + POSE + ['--shm', '8']] * 2, 50,
                               decode_streams=2, prefetch=4, launch_depth=2)
    assert st['planar_frames'] > 0 and st['launches'] >= 2, st
    for b in imgs:
        assert b.dtype == ref.dtype and b.shape[1:] == ref.shape
        for i in b:
            assert torch.equal(i, ref)


def test_mixed_layout_group_on_two_streams(dev, free_port):
    """A ring producer (rgb_a slots) and an inline producer (interleaved
    frames in pinned slots): a launch group holds both layouts and runs as two
    kernels, both on the group's stream.  launch_depth=0 with a posted buffer
    per batch makes the groups deterministic: 32 batches of 4 go out as two
    groups of 64 images, one per stream, and `launches` counts groups."""
    ref = _one_stream_image(dev, free_port, 'f32-nchw')
    # the ring holds 4 slots, handed back only when their launch retires: every
    # group of 64 has at most 4 ring frames, the paced inline producer supplies the rest
    prod = [RES + POSE + ['--shm', '4'], RES + POSE + ['--fps', '400']]
    runs = {}
    for i, ds in enumerate((1, 2)):
        imgs, st = _fixed_pose_run(dev, free_port + 5 + 5 * i, _CFGS['f32-nchw'](), prod, 32, decode_streams=ds,
                                   launch_depth=0, prefetch=32)
        assert 0 < st['planar_frames'] < st['frames'] and st['shm_frames'] < st['frames'], st   # both layouts
        assert st['launches'] == 2, st
        runs[ds] = imgs
    for a, b in zip(runs[1], runs[2]):
        assert torch.equal(a, b)
        for i in b:
            assert torch.equal(i, ref)


def test_output_buffers_wait_for_their_post_event(dev, free_port):
    """reuse_buffers with GPU-side ordering: a tensor is posted again two
    batches after its hand-out, and the launch that refills it -- on
    whichever stream -- must wait for the consumer's work queued before that
    post.  The consumer queues slow work and then a reduction over each batch;
    the reduction must see the batch as it was handed out."""
    args = [RES + ['--stamp', '--shm', '8']] * 2
    busy = torch.randn(1024, 1024, device=dev)
    sums = []
    with _launcher(free_port, args) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=4, max_items=4 * 60, device=dev,
                          decode=ops.DecodeConfig.raw(), prefetch=2, launch_depth=2, host_sync=False,
                          reuse_buffers=True, decode_streams=2)
        for b in dl:
            img = b['image']
            at_handout = img.clone()
            for _ in range(4):                          # keeps the stream busy past the next hand-out
                busy = torch.tanh(busy @ busy * 1e-3)
            # nothing here waits for the GPU: the consumer runs ahead of its stream
            sums.append((img.to(torch.int64).sum(dim=(1, 2, 3)), at_handout,
                         [(int(x), int(y)) for x, y in zip(b['btid'], b['seq'])]))
        st = dl.stats
    torch.cuda.synchronize(dev)
    assert len(sums) == 60 and st['direct_batches'] == st['batches'] == 60 and st['launches'] >= 2, st
    for late, at_handout, meta in sums:
        assert torch.equal(late, at_handout.to(torch.int64).sum(dim=(1, 2, 3)))
        assert _stamps(at_handout) == meta


def test_early_close_with_launches_in_flight(dev, free_port):
    """Leaving the stream after 10 batches, with launches queued on both
    streams, raises nothing and leaks no shared-memory segment; a second
    loader on the same device then streams correctly."""
    args = [RES + ['--stamp', '--shm', '8']] * 2
    for i in range(2):
        with _launcher(free_port + 5 * i, args) as bl:
            dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=4, device=dev,
                              decode=ops.DecodeConfig.raw(), prefetch=8, launch_depth=2, decode_streams=2)
            it = iter(dl)
            for _ in range(10):
                b = next(it)
                assert _stamps(b['image']) == [(int(x), int(y)) for x, y in zip(b['btid'], b['seq'])]
            it.close()
            st = dl.stats
            assert st['bad'] == 0 and st['shm_torn'] == 0 and st['direct_batches'] == st['batches'] >= 10, st
        assert not [f for f in os.listdir('/dev/shm') if f.startswith('blendtorch-')]
    torch.cuda.synchronize(dev)
