"""The renderer's two fill paths (csrc/sim/raster.h ``raster_isa``: the scalar
bodies and the AVX2 bodies chosen by ``BLENDTORCH_RASTER_ISA``) and its
restore-after-draw order write the same bytes: ``cubesim --bench`` renders
every frame in full and incrementally (into rotating buffers, as ring slots
are) and counts the bytes that differ, and a mirror updated only inside the
rectangle the producer would report must stay equal to its buffer.  100x75 has
a width that is no multiple of 8, so vector tails and 3-byte last pixels occur
on most rows."""
import json
import os
import subprocess
from pathlib import Path

import pytest

from blendtorch import btt

EXE = Path(btt.__file__).resolve().parents[1] / 'bin' / 'cubesim'
FRAMES = 200


def _has_avx2():
    try:
        with open('/proc/cpuinfo') as f:
            return any(line.startswith('flags') and ' avx2' in line for line in f)
    except OSError:
        return False


def _bench(isa, args):
    env = dict(os.environ, BLENDTORCH_RASTER_ISA=isa)
    out = subprocess.run([str(EXE), '--bench', str(FRAMES), *args], capture_output=True, text=True, timeout=120,
                         env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    rep = json.loads(out.stdout)
    assert rep['frames'] == FRAMES and rep['isa'] == isa, rep
    assert rep['mismatched_bytes'] == 0 and rep['mirror_mismatched_bytes'] == 0, rep
    return rep


@pytest.mark.parametrize('resolution', ['640x480', '160x120', '100x75'])
@pytest.mark.parametrize('scene', ['cube', 'falling_cubes'])
@pytest.mark.parametrize('origin', ['upper-left', 'lower-left'])
@pytest.mark.parametrize('layout', ['interleaved', 'planar'])
@pytest.mark.parametrize('mode', ['rgb', 'rgba'])
def test_fill_paths_write_the_same_bytes(mode, layout, origin, scene, resolution):
    args = ['--mode', mode, '--shm-layout', layout, '--origin', origin, '--scene', scene, '--resolution', resolution]
    if scene == 'falling_cubes':
        args += ['--frame-range', '0', '40']
    scalar = _bench('scalar', args)
    if not _has_avx2():
        pytest.skip('this CPU has no AVX2: only the scalar path ran')
    avx2 = _bench('avx2', args)
    assert avx2['checksum'] == scalar['checksum']
