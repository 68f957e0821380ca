"""The GPU loader's one-pass descriptor scan (csrc/codec/pickle_codec.h
``scan_descriptor``) against the full parse: for every shared-memory
descriptor message it accepts, slot, generation, offset, shape, layout tag,
delta tuple, ``origin`` and ``btid`` are what the parse tree holds; whatever it
does not model (inline images, memo reads of a CPython pickle, truncated or
garbage bytes) it declines, and the loader parses those as before.  The same
scan runs over mutated messages in exactly sized heap copies under ASan + UBSan
(csrc/tests/fuzz_descriptor_scan.cpp)."""
import os
import pickle
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blendtorch import _native

ROOT = Path(__file__).resolve().parent.parent
XY = np.arange(16, dtype=np.float64).reshape(8, 2)
BASE = ('blendtorch-4242-3', 17, 4096 + 17 * 1228800, 480, 640, 4, 'image', 123456)
RGB_A, TILE16 = ('rgb_a',), ('tile16', 'blendtorch-4242-3-key', 1)
DELTA = (123455, 100, 300, 200, 450)

DESCRIPTORS = {
    'plain': BASE,
    'rgb_a': BASE + (RGB_A,),
    'tile16': BASE + (TILE16,),
    'none_delta': BASE + (None, DELTA),
    'rgb_a_delta': BASE + (RGB_A, DELTA),
    'empty_delta': BASE + (RGB_A, (123455, 0, -1, 0, -1)),
    'big_ints': ('s', 70000, 2 ** 40, 48, 64, 3, 'image', 2 ** 30 - 1),
}


def _message(desc, origin=None, btid=3):
    d = {'btid': btid, 'xy': XY, 'frameid': 9}
    if origin is not None:
        d['origin'] = origin
    d['_btshm'] = desc
    return _native.dumps_array_dict(d)


def _expect(desc, origin, btid):
    tag = desc[8] if len(desc) > 8 and isinstance(desc[8], tuple) else None
    return {'segment': desc[0], 'slot': desc[1], 'offset': desc[2], 'shape': tuple(desc[3:6]), 'image_key': desc[6],
            'generation': desc[7], 'elements': len(desc), 'tag': tag, 'delta': desc[9] if len(desc) > 9 else None,
            'origin': origin, 'btid': btid}


@pytest.mark.parametrize('origin', [None, 'lower-left', 'upper-left'])
@pytest.mark.parametrize('name', sorted(DESCRIPTORS))
def test_scan_agrees_with_the_full_parse(name, origin):
    desc = DESCRIPTORS[name]
    msg = _message(desc, origin)
    tree = _native.fast_loads(msg)
    assert tree['_btshm'] == desc and tree['btid'] == 3 and tree.get('origin') == origin
    got = _native.scan_descriptor(msg)
    assert got == _expect(tree['_btshm'], tree.get('origin'), tree['btid'])


def test_scan_declines_what_it_does_not_model():
    img = np.zeros((4, 6, 4), np.uint8)
    # an inline image (with or without a descriptor next to it): the inline path's business
    assert _native.scan_descriptor(_native.dumps_array_dict({'btid': 1, 'image': img})) is None
    assert _native.scan_descriptor(_native.dumps_array_dict({'btid': 1, 'image': img, '_btshm': BASE})) is None
    assert _native.scan_descriptor(_native.dumps_array_dict({'btid': 1, 'pixels': img, '_btshm': BASE}),
                                   image_key='pixels') is None
    # no descriptor at all
    assert _native.scan_descriptor(_native.dumps_array_dict({'btid': 1, 'xy': XY})) is None
    # a CPython pickle of the same dict reads its memo (BINGET) for the array: the full parse takes it
    assert _native.scan_descriptor(pickle.dumps({'btid': 1, 'xy': XY, '_btshm': BASE}, protocol=4)) is None
    assert _native.scan_descriptor(pickle.dumps({'btid': 1, 'xy': XY, '_btshm': BASE}, protocol=2)) is None
    # entries of another type than the loader reads
    assert _native.scan_descriptor(_native.dumps_array_dict({'btid': 'x', '_btshm': BASE})) is None
    assert _native.scan_descriptor(_native.dumps_array_dict({'btid': 1, 'origin': 5, '_btshm': BASE})) is None
    assert _native.scan_descriptor(_native.dumps_array_dict({'btid': 1, '_btshm': BASE[:7]})) is None
    assert _native.scan_descriptor(_native.dumps_array_dict({'btid': 1, '_btshm': ('s', 'x') + BASE[2:]})) is None
    assert _native.scan_descriptor(_native.dumps_array_dict({'btid': 1, '_btshm': BASE + (None, (1, 2, 3))})) is None
    assert _native.scan_descriptor(_native.dumps_array_dict({'btid': 1, '_btshm': BASE + (None, (1, 2, 3, 4, 'x'))})) is None
    assert _native.scan_descriptor(_native.dumps_array_dict({'btid': 1, '_btshm': BASE + (('a', 'b'),)})) is None
    # a pickle without numpy memo reads is within the scan's reach whoever wrote it
    got = _native.scan_descriptor(pickle.dumps({'btid': 2, '_btshm': BASE + (RGB_A, DELTA)}, protocol=4))
    assert got == _expect(BASE + (RGB_A, DELTA), None, 2)


def test_scan_rejects_truncated_and_garbage_bytes():
    msg = _message(BASE + (RGB_A, DELTA), 'lower-left')
    assert _native.scan_descriptor(msg) is not None
    for cut in range(len(msg)):   # the binding scans an exactly sized copy
        assert _native.scan_descriptor(msg[:cut]) is None, cut
    for junk in (b'', b'\x80', b'\x80\x04garbage', b'\x80\x04}.', b'\x00' * 64, b'(' * 64, bytes(range(256))):
        assert _native.scan_descriptor(junk) is None
    rng = np.random.default_rng(7)
    for _ in range(300):   # accepted or not, a mutated message never disagrees with the parse
        m = bytearray(msg)
        for at in rng.integers(0, len(m), size=int(rng.integers(1, 4))):
            m[at] = int(rng.integers(0, 256))
        got = _native.scan_descriptor(bytes(m))
        if got is None:
            continue
        try:
            tree = _native.fast_loads(bytes(m))
        except (ValueError, TypeError):
            continue   # rejected when the tree is built (the scan does not look into the arrays it skips)
        d = tree['_btshm']
        assert got == _expect(d, tree.get('origin'), tree.get('btid'))


def test_descriptor_scan_fuzz_asan_ubsan(tmp_path):
    exe = tmp_path / 'fuzz_descriptor_scan'
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           '-pthread', str(ROOT / 'csrc/tests/fuzz_descriptor_scan.cpp'), str(ROOT / 'csrc/codec/pickle_codec.cpp'),
           '-o', str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert 'valid=16 ' in r.stdout and 'disagreed=0' in r.stdout, r.stdout
