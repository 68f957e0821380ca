"""The slot-delta report of a native producer on the CPU (csrc/transport/
shmring.h ``kWantSlotDelta``, csrc/sim/cubesim.cpp): without the hint bit the
descriptors are today's; with it a 10th element ``(base_gen, y0, y1, x0, x1)``
names the generation the slot was last published with and a rectangle outside
which the slot's bytes did not change -- replaying the rectangles into a numpy
copy of every slot reproduces the slots byte for byte; the element is withheld
for the one frame in which a slot changes its layout; and ``shm.resolve``
delivers the same images either way."""
import numpy as np
import pytest

from blendtorch import btt
from blendtorch.transport import shm, zmq

DELTA = shm.WANT_SLOT_DELTA
ARGS = ['--mode', 'rgba', '--resolution', '64x48', '--shm', '4', '--stamp']
H, W = 48, 64


def _stream(port, args, n, on_frame, seed=7):
    """One cubesim; ``on_frame(i, desc, raw)`` sees every descriptor and, still unclaimed, the bytes its
    slot holds for the consumer (H*W*3 of an rgb_a slot, else H*W*C).  Returns the resolved images."""
    imgs = []
    with btt.BlenderLauncher(producer='cubesim', num_instances=1, named_sockets=['DATA'], start_port=port,
                             proto='ipc', seed=seed, instance_args=[args + ['--frames', str(n)]]) as bl:
        s = zmq.Context().socket(zmq.PULL)
        s.connect(bl.launch_info.addresses['DATA'][0])
        for i in range(n):
            assert s.poll(20000), f'no frame {i}'
            msg = s.recv_pyobj()
            desc = msg[shm.KEY]
            name, slot, off, h, w, c = desc[:6]
            planar = len(desc) > 8 and bool(desc[8]) and desc[8][0] == 'rgb_a'
            raw = np.frombuffer(shm._open(name).mm, np.uint8, h * w * (3 if planar else c), off).copy()
            on_frame(i, desc, raw)
            imgs.append(np.array(shm.resolve(msg, strict=True)['image']))
        s.close()
    return imgs


class _Mirrors:
    """What a consumer with a byte copy per slot does with the reports."""

    def __init__(self):
        self.gen, self.copy, self.layout = {}, {}, {}
        self.deltas, self.flip_without_delta = [], 0

    def frame(self, i, desc, raw):
        slot, gen = desc[1], desc[7]
        cin = raw.size // (H * W)
        delta = desc[9] if len(desc) > 9 else None
        if self.layout.get(slot, cin) != cin:
            assert delta is None, f'frame {i}: a slot that changed its layout reported a rectangle'
            self.flip_without_delta += 1
        self.layout[slot] = cin
        if delta is None:
            self.copy[slot] = raw.copy()
        else:
            base, y0, y1, x0, x1 = delta
            assert base == self.gen[slot], f'frame {i}: base_gen {base}, slot {slot} was last seen with {self.gen[slot]}'
            assert y1 < y0 or (0 <= y0 <= y1 < H and 0 <= x0 <= x1 < W), delta
            m, r = self.copy[slot].reshape(H, W, cin), raw.reshape(H, W, cin)
            if y1 >= y0:
                m[y0:y1 + 1, x0:x1 + 1] = r[y0:y1 + 1, x0:x1 + 1]
            assert np.array_equal(self.copy[slot], raw), f'frame {i}: slot {slot} changed outside {delta}'
            self.deltas.append(i)
        self.gen[slot] = gen


@pytest.mark.parametrize('extra', [['--shm-layout', 'interleaved'], ['--shm-layout', 'planar'],
                                   ['--shm-layout', 'interleaved', '--origin', 'lower-left'],
                                   ['--shm-layout', 'interleaved', '--scene', 'falling_cubes']])
def test_rectangles_reproduce_every_slot(free_port, extra):
    n, at = 40, 8
    mir = _Mirrors()

    def on_frame(i, desc, raw):
        if i < at:
            assert len(desc) <= 9, desc            # no hint: today's descriptors
            assert shm.hint(desc[0]) & DELTA == 0
        if i == at:
            shm.add_hint(desc[0], DELTA)
        if len(desc) > 9:
            assert len(desc) == 10 and len(desc[9]) == 5
            assert desc[8] is None or desc[8] == ('rgb_a',)
        mir.frame(i, desc, raw)

    imgs = _stream(free_port, ARGS + extra, n, on_frame)
    # the producer runs at most 4 slots + the frame it holds ahead of the consumer; from then on every
    # frame reports (its slot was used, and published by this producer, before)
    assert mir.deltas and mir.deltas[0] > at
    assert set(range(at + 6, n)) <= set(mir.deltas), mir.deltas
    assert len({im.tobytes()[16:] for im in imgs}) > 4                         # the poses do differ
    # the rectangles are no whole frames: the Cube leaves most rows alone
    assert imgs[0].shape == (H, W, 4)


def test_report_is_withheld_when_a_slot_changes_layout(free_port):
    n = 40
    mir = _Mirrors()

    def on_frame(i, desc, raw):
        if i == 4:
            shm.add_hint(desc[0], DELTA)
        if i == 20:
            shm.add_hint(desc[0], shm.WANT_PLANAR_ALPHA)                        # auto layout: slots turn rgb_a
        mir.frame(i, desc, raw)

    _stream(free_port, ARGS, n, on_frame)
    assert mir.flip_without_delta == 4, mir.flip_without_delta                  # each of the 4 slots, once
    assert set(mir.layout.values()) == {3}
    assert [i for i in mir.deltas if i < 20] and set(range(31, n)) <= set(mir.deltas), mir.deltas


def test_resolve_returns_the_same_images_with_the_hint(free_port):
    n = 16
    plain = _stream(free_port, ARGS, n, lambda i, desc, raw: None)

    def on_frame(i, desc, raw):
        if i == 0:
            shm.add_hint(desc[0], DELTA)

    hinted = _stream(free_port + 5, ARGS, n, on_frame)
    assert len(plain) == len(hinted) == n
    for i, (a, b) in enumerate(zip(plain, hinted)):
        assert a.shape == (H, W, 4) and a.tobytes() == b.tobytes(), f'frame {i}'
