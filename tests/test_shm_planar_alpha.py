"""The ring's consumer hint and the ``rgb_a`` slot layout (packed RGB followed
by the alpha plane; csrc/common/planar_alpha.h) on the CPU: the hint bits are
sticky and shared between the Python mirror and the native module, and an RGBA
frame resolves to the same ``H x W x 4`` bytes whichever layout its slot held."""
import mmap
import os
import struct
import time

import numpy as np
import pytest

from blendtorch import _native, btt
from blendtorch.transport import shm, zmq

WANT, NEED = shm.WANT_PLANAR_ALPHA, shm.NEED_INTERLEAVED


def _frames(port, args, n, seed=7, on_frame=None):
    """Run one cubesim producer; returns [(layout tag or None, resolved H x W x C image, seq)]."""
    out = []
    with btt.BlenderLauncher(producer='cubesim', num_instances=1, named_sockets=['DATA'], start_port=port,
                             proto='ipc', seed=seed, instance_args=[args + ['--frames', str(n)]]) as bl:
        s = zmq.Context().socket(zmq.PULL)
        s.connect(bl.launch_info.addresses['DATA'][0])
        for i in range(n):
            assert s.poll(20000), f'no frame {i}'
            msg = s.recv_pyobj()
            desc = msg[shm.KEY]
            tag = desc[8][0] if len(desc) > 8 else None
            if on_frame is not None:
                on_frame(i, desc)
            msg = shm.resolve(msg, strict=True)
            out.append((tag, np.array(msg['image']), int(msg['seq'])))
        s.close()
    return out


def test_hint_round_trip_python_and_native():
    name = f'blendtorch-{os.getpid()}-hint-{time.monotonic_ns()}'
    ring = shm.ShmRing(name, 2, 64)
    try:
        seg = shm._open(name)                      # a consumer's own mapping
        assert shm.hint(name) == 0 and _native.ring_hint(seg.mm) == 0 and ring.seg.hint() == 0
        assert shm.add_hint(name, WANT) == WANT
        assert _native.ring_hint(ring.seg.mm) == WANT and ring.seg.hint() == WANT
        assert _native.ring_add_hint(seg.mm, NEED) == WANT | NEED      # OR-ed, not replaced
        assert shm.hint(name) == WANT | NEED and ring.seg.hint() == WANT | NEED
        assert shm.add_hint(name, WANT) == WANT | NEED                  # sticky: nothing clears a bit
        assert shm.add_hint(name, 0) == WANT | NEED
        assert _native.ring_hint(seg.mm) == WANT | NEED
        assert (_native.RING_VERSION, _native.WANT_PLANAR_ALPHA, _native.NEED_INTERLEAVED) == (shm.VERSION, WANT, NEED)
        # the slot words still start right behind the header, and work
        slot, off, h, w, c, gen = ring.put(np.arange(64, dtype=np.uint8).reshape(4, 16))
        got = shm.resolve({shm.KEY: (name, slot, off, h, w, c, 'image', gen)}, strict=True)
        assert (got['image'] == np.arange(64, dtype=np.uint8).reshape(4, 16)).all()
        assert shm.hint(name) == WANT | NEED
    finally:
        ring.close()


def test_old_header_version_is_rejected():
    name = f'blendtorch-{os.getpid()}-v1-{time.monotonic_ns()}'
    path = '/dev/shm/' + name
    fd = os.open(path, os.O_CREAT | os.O_EXCL | os.O_RDWR, 0o600)
    try:
        os.ftruncate(fd, 8192)
        mm = mmap.mmap(fd, 8192, mmap.MAP_SHARED, mmap.PROT_READ | mmap.PROT_WRITE)
        struct.pack_into('<QIIQQ', mm, 0, shm.MAGIC, 1, 1, 4096, 4096)      # the version-1 header: no hint word
        with pytest.raises(ValueError, match='version 1.*version 2'):
            shm._open(name)
        with pytest.raises(ValueError, match='version 1.*version 2'):
            _native.ring_hint(mm)
        with pytest.raises(ValueError, match='version 1.*version 2'):
            _native.ring_add_hint(mm, WANT)
        assert struct.unpack_from('<I', mm, 32)[0] == 0                      # nothing was written into it
        mm.close()
    finally:
        os.close(fd)
        os.unlink(path)


BASE = ['--mode', 'rgba', '--resolution', '32x8', '--shm', '4', '--stamp']


@pytest.mark.parametrize('origin', ['upper-left', 'lower-left'])
def test_layouts_resolve_identically(free_port, origin):
    args = BASE + ['--rotation', '0.6', '0.4', '0.9', '--origin', origin]
    inter = _frames(free_port, args + ['--shm-layout', 'interleaved'], 12)
    plan = _frames(free_port + 5, args + ['--shm-layout', 'planar'], 12)
    assert [t for t, _, _ in inter] == [None] * 12 and [t for t, _, _ in plan] == ['rgb_a'] * 12
    for i, ((_, a, sa), (_, b, sb)) in enumerate(zip(inter, plan)):
        assert sa == sb == i
        assert a.shape == b.shape == (8, 32, 4) and a.dtype == b.dtype == np.uint8
        assert a.tobytes() == b.tobytes(), f'frame {i}'
        flat = b.reshape(-1)
        st = struct.pack('<2sHIQ', b'BT', 0, 0, i)                            # the stamp: 16 logical HWC bytes
        assert flat[:16].tobytes() == st
        assert (flat[16:].reshape(-1, 4)[:, 3] == 255).all()                  # alpha is 255 outside the stamp
    assert len({a.tobytes()[16:] for _, a, _ in plan}) == 1                   # fixed pose: the same picture every frame
    assert len(np.unique(plan[0][1][..., :3])) > 4                            # ... and a picture, not a blank


def test_auto_follows_the_hint_and_slots_change_layout(free_port):
    """Random poses (the same seed in both runs), 4 slots: every slot holds
    interleaved, then planar, then interleaved frames again, and each frame is
    byte-identical to the all-interleaved run's."""
    args = ['--mode', 'rgba', '--resolution', '32x8', '--shm', '4', '--stamp']
    n = 36
    ref = _frames(free_port, args + ['--shm-layout', 'interleaved'], n)

    def steer(i, desc):
        if i == 8:
            assert shm.hint(desc[0]) == 0
            shm.add_hint(desc[0], WANT)
        if i == 22:
            _native.ring_add_hint(shm._open(desc[0]).mm, NEED)

    got = _frames(free_port + 5, args, n, on_frame=steer)
    tags = [t for t, _, _ in got]
    # the producer is at most 4 slots + the frame it holds ahead of the consumer
    assert tags[:9] == [None] * 9
    assert tags[14:23] == ['rgb_a'] * 9
    assert tags[28:] == [None] * (n - 28)
    for i, ((_, a, sa), (_, b, sb)) in enumerate(zip(ref, got)):
        assert sa == sb == i
        assert a.tobytes() == b.tobytes(), f'frame {i} ({tags[i]})'
    assert len({a.tobytes()[16:] for _, a, _ in got}) > 4                     # the poses do differ


def test_size_rule_keeps_unaligned_frames_interleaved(free_port):
    # 4 x 3 pixels: H*W*3 = 36 is no multiple of 16, so the alpha plane could not start aligned
    got = _frames(free_port, ['--mode', 'rgba', '--resolution', '4x3', '--shm', '4', '--stamp',
                              '--shm-layout', 'planar'], 6)
    assert [t for t, _, _ in got] == [None] * 6
    assert all(a.shape == (3, 4, 4) for _, a, _ in got)
    # ... and RGB frames have no alpha to move
    got = _frames(free_port + 5, ['--mode', 'rgb', '--resolution', '32x8', '--shm', '4', '--stamp',
                                  '--shm-layout', 'planar'], 6)
    assert [t for t, _, _ in got] == [None] * 6 and got[0][1].shape == (8, 32, 3)


def test_resolve_rejects_rgb_a_outside_its_slot():
    name = f'blendtorch-{os.getpid()}-oob-{time.monotonic_ns()}'
    ring = shm.ShmRing(name, 2, 4096)
    try:
        slot, off, h, w, c, gen = ring.put(np.zeros((8, 32, 4), np.uint8))
        for bad in [(off + 3200, 8, 32), (off, 64, 32), (off, 4, 3)]:          # past the slot end twice; unaligned plane
            desc = (name, slot, bad[0], bad[1], bad[2], 4, 'image', gen, ('rgb_a',))
            with pytest.raises(ValueError, match='rgb_a'):
                shm._interleave_rgb_a(shm._open(name), slot, *desc[2:6])
        with pytest.raises(ValueError, match='rgb_a'):
            _native.interleave_rgb_a(ring.seg.mm, off, 64, 32, off + 4096)
        with pytest.raises(ValueError, match='rgb_a'):
            _native.interleave_rgb_a(ring.seg.mm, off, 8, 32, len(ring.seg.mm) + 4096)
        # numpy fallback == native helper
        rng = np.random.default_rng(0)
        ring.seg.slot_array(slot, (1024,))[:] = rng.integers(0, 256, 1024, dtype=np.uint8)
        a = _native.interleave_rgb_a(ring.seg.mm, off, 8, 32, off + 4096)
        saved, shm._native_interleave = shm._native_interleave, None
        try:
            b = shm._interleave_rgb_a(shm._open(name), slot, off, 8, 32, 4)
        finally:
            shm._native_interleave = saved
        raw = ring.seg.slot_array(slot, (1024,))
        assert a.shape == (8, 32, 4) and a.tobytes() == b.tobytes()
        assert (a[..., :3].reshape(-1) == raw[:768]).all() and (a[..., 3].reshape(-1) == raw[768:]).all()
    finally:
        ring.close()
