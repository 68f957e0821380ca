"""The changed-block report of a native producer on the CPU (csrc/transport/
shmring.h ``kWantSlotBlocks``, csrc/sim/cubesim.cpp): a consumer that set the
bit next to ``kWantSlotDelta`` gets an 11th descriptor element ``(band_rows,
mask)`` -- one little-endian uint16 per band of ``band_rows`` stored rows, bit
``c`` covering pixel columns [64c, 64c + 63] -- outside whose set blocks the
slot's pixel bytes did not change since ``base_gen``.  Replaying only the set
blocks into a numpy copy of every slot reproduces the slots byte for byte,
across layout flips and from the first frames before the hint; without the bit
no descriptor has an 11th element; and the loader's one-pass scan reads the
element as the full parse does."""
import pickle

import numpy as np
import pytest

from blendtorch import _native, btt
from blendtorch.transport import shm, zmq

DELTA, BLOCKS = shm.WANT_SLOT_DELTA, shm.WANT_SLOT_BLOCKS
H, W = 96, 256
ARGS = ['--mode', 'rgba', '--resolution', f'{W}x{H}', '--shm', '4', '--stamp']


def _stream(port, args, n, on_frame, seed=7):
    """One cubesim; ``on_frame(i, desc, raw)`` sees every descriptor and, still unclaimed, the pixel bytes
    its slot holds (H*W*3 of an rgb_a slot, else H*W*C)."""
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
            assert shm.resolve(msg, strict=True) is not None
        s.close()


def _block_map(desc, h, w):
    """The H x W bool map of the pixels in the set blocks of descriptor element 11."""
    band_rows, mask = desc[10]
    assert band_rows >= 1 and band_rows & (band_rows - 1) == 0, band_rows
    nb = -(-h // band_rows)
    assert isinstance(mask, bytes) and len(mask) == 2 * nb and nb <= 30, (band_rows, len(mask))
    words = np.frombuffer(mask, '<u2')
    assert not (words >> (w // 64)).any(), 'a bit past the last column block'
    m = np.zeros((h, w), bool)
    for k, word in enumerate(words):
        for c in range(w // 64):
            if (int(word) >> c) & 1:
                m[k * band_rows:(k + 1) * band_rows, 64 * c:64 * c + 64] = True
    return m


class _Mirrors:
    """A consumer with a byte copy per slot that takes only the set blocks of every report."""

    def __init__(self):
        self.gen, self.copy, self.layout = {}, {}, {}
        self.masked, self.flips, self.fraction = [], 0, []

    def frame(self, i, desc, raw):
        slot, gen = desc[1], desc[7]
        cin = raw.size // (H * W)
        if self.layout.get(slot, cin) != cin:
            assert len(desc) <= 9, f'frame {i}: a slot that changed its layout reported what changed'
            self.flips += 1
        self.layout[slot] = cin
        if len(desc) <= 9:
            self.copy[slot] = raw.copy()
        else:
            base, y0, y1, x0, x1 = desc[9]
            assert base == self.gen[slot], f'frame {i}: base_gen {base}, slot {slot} was last seen with {self.gen[slot]}'
            m, r = self.copy[slot].reshape(H, W, cin), raw.reshape(H, W, cin)
            if len(desc) > 10:
                inside = _block_map(desc, H, W)
                self.fraction.append(inside.mean())
                m[inside] = r[inside]
                self.masked.append(i)
            elif y1 >= y0:
                m[y0:y1 + 1, x0:x1 + 1] = r[y0:y1 + 1, x0:x1 + 1]
            assert np.array_equal(self.copy[slot], raw), f'frame {i}: slot {slot} changed outside its report {desc[9:]}'
        self.gen[slot] = gen


@pytest.mark.parametrize('extra', [['--shm-layout', 'interleaved'], ['--shm-layout', 'planar'],
                                   ['--shm-layout', 'interleaved', '--origin', 'lower-left'],
                                   ['--shm-layout', 'interleaved', '--scene', 'falling_cubes'],
                                   ['--shm-layout', 'interleaved', '--render-threads', '1'],
                                   ['--shm-layout', 'planar', '--render-threads', '2']])
def test_set_blocks_reproduce_every_slot(free_port, extra):
    n, at = 48, 8
    mir = _Mirrors()

    def on_frame(i, desc, raw):
        if i < at:
            assert len(desc) <= 9, desc            # no hint: the first frames are taken whole
        if i == at:
            shm.add_hint(desc[0], DELTA | BLOCKS)
        if len(desc) > 9:
            assert len(desc) == 11 and len(desc[9]) == 5 and len(desc[10]) == 2, desc
        mir.frame(i, desc, raw)

    _stream(free_port, ARGS + extra, n, on_frame)
    assert mir.masked and mir.masked[0] > at
    assert set(range(at + 6, n)) <= set(mir.masked), mir.masked
    assert min(mir.fraction) < 1.0                                            # the masks are no whole frames


def test_layout_flip_withholds_the_report_and_the_copies_stay_right(free_port):
    n = 44
    mir = _Mirrors()

    def on_frame(i, desc, raw):
        if i == 4:
            shm.add_hint(desc[0], DELTA | BLOCKS)
        if i == 20:
            shm.add_hint(desc[0], shm.WANT_PLANAR_ALPHA)                        # auto layout: slots turn rgb_a
        mir.frame(i, desc, raw)

    _stream(free_port, ARGS, n, on_frame)
    assert mir.flips == 4, mir.flips                                            # each of the 4 slots, once
    assert set(mir.layout.values()) == {3}
    assert [i for i in mir.masked if i < 20] and set(range(31, n)) <= set(mir.masked), mir.masked


def test_no_eleventh_element_without_the_new_bit(free_port):
    seen = []

    def on_frame(i, desc, raw):
        if i == 2:
            shm.add_hint(desc[0], DELTA)
        seen.append(len(desc))
        if len(desc) > 9:
            assert len(desc) == 10 and len(desc[9]) == 5, desc                   # five values, as before

    _stream(free_port, ARGS, 24, on_frame)
    assert max(seen) == 10 and 10 in seen[8:], seen


def test_no_mask_where_the_width_admits_no_grid(free_port):
    seen = []

    def on_frame(i, desc, raw):
        if i == 0:
            shm.add_hint(desc[0], DELTA | BLOCKS)
        seen.append(len(desc))

    args = ['--mode', 'rgba', '--resolution', '96x48', '--shm', '4', '--stamp']  # 96 % 64 != 0
    _stream(free_port, args, 20, on_frame)
    assert max(seen) == 10 and 10 in seen[8:], seen


# ---- the loader's descriptor scan --------------------------------------------------------------------------------

XY = np.arange(16, dtype=np.float64).reshape(8, 2)
BASE = ('blendtorch-4242-3', 17, 4096 + 17 * 1228800, 480, 640, 4, 'image', 123456)
DELTA_T = (123455, 100, 300, 200, 450)
MASK = bytes(range(60))


def _message(desc):
    return pickle.dumps({'btid': 3, 'xy': 1.5, 'frameid': 9, '_btshm': desc}, protocol=4)


@pytest.mark.parametrize('tag', [None, ('rgb_a',)])
def test_scan_reads_the_eleventh_element_as_the_parse_does(tag):
    desc = BASE + (tag, DELTA_T, (16, MASK))
    msg = _message(desc)
    tree = _native.fast_loads(msg)
    assert tree['_btshm'] == desc
    got = _native.scan_descriptor(msg)
    assert got is not None and got['elements'] == 11 and got['delta'] == DELTA_T
    assert got['blocks'] == (16, MASK) == tree['_btshm'][10]
    assert got['tag'] == tag
    # without the element: no 'blocks' entry, everything else as before
    got10 = _native.scan_descriptor(_message(BASE + (tag, DELTA_T)))
    assert got10 is not None and 'blocks' not in got10 and got10['delta'] == DELTA_T and got10['elements'] == 10


@pytest.mark.parametrize('bad', [None, 5, (16,), (16, MASK, 1), ('16', MASK), (16, 'text'), (0, MASK), (-16, MASK),
                                 (16, b''), (16, MASK[:59]), (16, bytes(130)), (2 ** 40, MASK)])
def test_a_malformed_eleventh_element_means_no_mask(bad):
    got = _native.scan_descriptor(_message(BASE + (None, DELTA_T, bad)))
    assert got is not None and 'blocks' not in got and got['delta'] == DELTA_T and got['elements'] == 11


def test_truncated_masks_never_scan():
    msg = _message(BASE + (None, DELTA_T, (16, MASK)))
    assert _native.scan_descriptor(msg) is not None
    at = msg.index(MASK)
    for cut in range(at - 4, len(msg)):
        assert _native.scan_descriptor(msg[:cut]) is None, cut
    # a length byte that claims more than the message holds
    m = bytearray(msg)
    assert m[at - 1] == len(MASK)
    m[at - 1] = 255
    assert _native.scan_descriptor(bytes(m)) is None
    # ... and twelve elements are no descriptor of this kind
    assert _native.scan_descriptor(_message(BASE + (None, DELTA_T, (16, MASK), 1))) is None
