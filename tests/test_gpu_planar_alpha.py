"""rgb_a ring slots (packed RGB, then the alpha plane) through the GPU loader:
an RGB-only direct decode reads the first three quarters of each slot in
place (Cin = 3), every other consumer gets the frame re-interleaved on the
host, and either way the decoded images are bit-identical to the interleaved
path and to the CPU reference decode.  64x32 stamped frames of one fixed pose,
batch 4, 10 batches per run."""
import struct

import numpy as np
import pytest
import torch

from blendtorch import btt, ops
from blendtorch.btt.gpu import DeviceLoader
from blendtorch.transport import shm, zmq

pytestmark = pytest.mark.gpu

B, NBATCH = 4, 10
POSE = ['--rotation', '0.6', '0.4', '0.9']
_frames = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    ops.hip_ext()
    return torch.device('cuda', 0)


def _args(res, *extra):
    return ['--mode', 'rgba', '--resolution', res, '--stamp', *POSE, *extra]


def _frame(res, port):
    """The fixed pose's H x W x 4 frame through the CPU path, once per resolution."""
    if res not in _frames:
        with btt.BlenderLauncher(producer='cubesim', num_instances=1, named_sockets=['DATA'], start_port=port,
                                 proto='ipc', instance_args=[_args(res, '--shm', '8', '--shm-layout',
                                                                   'interleaved')]) as bl:
            s = zmq.Context().socket(zmq.PULL)
            s.connect(bl.launch_info.addresses['DATA'][0])
            assert s.poll(20000)
            _frames[res] = np.ascontiguousarray(shm.resolve(s.recv_pyobj())['image'])
            s.close()
        _frames[res].setflags(write=False)
    return _frames[res]


def _reference(frame, cfg, btid, seq):
    f = frame.copy()
    f.reshape(-1)[:16] = np.frombuffer(struct.pack('<2sHIQ', b'BT', btid, 0, seq), np.uint8)
    return ops.reference_decode(torch.from_numpy(f[None]), cfg, flip=[0])[0]


def _run(dev, port, cfg, producers, **kw):
    """{(btid, seq): decoded image (cpu)} of B * NBATCH frames, and the loader's stats."""
    out = {}
    with btt.BlenderLauncher(producer='cubesim', num_instances=len(producers), named_sockets=['DATA'],
                             start_port=port, proto='ipc', instance_args=producers) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=B, max_items=B * NBATCH, device=dev,
                          decode=cfg, **kw)
        for b in dl:
            img = b['image'].cpu()
            for k in range(B):
                out[(int(b['btid'][k]), int(b['seq'][k]))] = img[k]
        st = dict(dl.stats)
    assert len(out) == B * NBATCH and st['bad'] == 0 and st['batches'] == NBATCH
    return out, st


def _assert_equal_runs(a, b, frame, cfg):
    assert set(a) == set(b)
    for key in a:
        assert torch.equal(a[key], b[key]), key
        assert torch.equal(a[key], _reference(frame, cfg, *key)), key


_CFGS = {
    'f32-nchw': lambda: ops.DecodeConfig.unit(channels='rgb', gamma=2.2),
    'bf16-nhwc': lambda: ops.DecodeConfig.unit(channels='rgb', gamma=2.2, dtype='bfloat16', layout='nhwc'),
}


@pytest.mark.parametrize('res', ['64x32', '6x8'])   # 6x8: W % 4 != 0, the scalar kernel with Cin = 3
@pytest.mark.parametrize('cfg', list(_CFGS))
def test_rgb_decode_reads_planar_slots_in_place(dev, free_port, cfg, res):
    cfg = _CFGS[cfg]()
    frame = _frame(res, free_port)
    prod = [_args(res, '--shm', '8')]
    planar, st = _run(dev, free_port + 5, cfg, prod)
    assert st['planar_frames'] > 0, st
    assert st['direct_batches'] == st['batches'] and st['staged_frames'] == 0, st
    inter, sti = _run(dev, free_port + 10, cfg, prod, shm_alpha='interleaved')
    assert sti['planar_frames'] == 0 and sti['direct_batches'] == sti['batches'] and sti['staged_frames'] == 0, sti
    # the planar frames crossed the link without their alpha plane
    h, w = frame.shape[:2]
    assert sti['image_bytes'] == B * NBATCH * h * w * 4
    assert st['image_bytes'] == sti['image_bytes'] - st['planar_frames'] * h * w
    _assert_equal_runs(planar, inter, frame, cfg)


def test_mixed_fleet_two_source_layouts_stay_direct(dev, free_port):
    cfg = _CFGS['f32-nchw']()
    frame = _frame('64x32', free_port)
    # the inline producer is paced: once its queued backlog (bounded by the high-water marks, ~22
    # frames) is taken, the ring producer -- 4 slots, so at most 4 frames from before the hint --
    # has to supply the rest, as rgb_a; launch_depth=0 puts both layouts into one launch group
    got, st = _run(dev, free_port + 5, cfg, [_args('64x32', '--shm', '4'), _args('64x32', '--fps', '200')],
                   launch_depth=0)
    assert st['direct_batches'] == st['batches'], st
    assert 0 < st['planar_frames'] < st['frames'] and st['shm_frames'] < st['frames'], st   # both layouts, both routes
    assert {k[0] for k in got} == {0, 1}
    for key, img in got.items():
        assert torch.equal(img, _reference(frame, cfg, *key)), key


@pytest.mark.parametrize('consumer', ['rgba', 'copy'])
def test_forced_planar_producer_is_reinterleaved_for_other_consumers(dev, free_port, consumer):
    """A consumer that needs alpha, or takes the copy path, asks for
    interleaved frames; a producer that writes rgb_a regardless is still read
    correctly: the loader rebuilds the frame on the host."""
    frame = _frame('64x32', free_port)
    if consumer == 'rgba':
        cfg, kw = ops.DecodeConfig.unit(channels='rgba'), {}
    else:
        cfg, kw = _CFGS['f32-nchw'](), {'h2d': 'copy'}
    planar, st = _run(dev, free_port + 5, cfg, [_args('64x32', '--shm', '8', '--shm-layout', 'planar')], **kw)
    assert st['planar_frames'] == st['frames'] == B * NBATCH, st
    assert st['image_bytes'] == B * NBATCH * frame.nbytes                  # whole frames crossed the link
    if consumer == 'copy':
        assert st['direct_batches'] == 0, st
    inter, sti = _run(dev, free_port + 10, cfg, [_args('64x32', '--shm', '8', '--shm-layout', 'interleaved')], **kw)
    assert sti['planar_frames'] == 0
    _assert_equal_runs(planar, inter, frame, cfg)
    if consumer == 'rgba':
        for img in planar.values():
            assert img.shape == (4, 32, 64)
            assert (img[3].reshape(-1)[4:] == 1.0).all()                   # alpha outside the stamp's 4 pixels
