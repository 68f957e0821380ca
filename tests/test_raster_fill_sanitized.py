"""The renderer's fill paths and its restore-after-draw order under
AddressSanitizer + UBSan, as a stand-alone host program
(csrc/tests/raster_fill_check.cpp): incremental renders of 3 and 4 channels
into exactly sized heap buffers at 100x75 and 64x48, both row orders, with the
box cut by every side of the frame, equal full renders byte for byte -- once
with the scalar fill bodies and once with the AVX2 ones."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRCS = ['csrc/tests/raster_fill_check.cpp', 'csrc/sim/raster.cpp']


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp('raster_fill') / 'raster_fill_check'
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           '-ffp-contract=off', '-pthread', *[str(ROOT / s) for s in SRCS], '-o', str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return out


def _has_avx2():
    try:
        with open('/proc/cpuinfo') as f:
            return any(line.startswith('flags') and ' avx2' in line for line in f)
    except OSError:
        return False


@pytest.mark.parametrize('isa', ['scalar', 'avx2'])
def test_raster_fill_check_asan_ubsan(exe, isa):
    if isa == 'avx2' and not _has_avx2():
        pytest.skip('this CPU has no AVX2')
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1',
               BLENDTORCH_RASTER_ISA=isa)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert f'isa={isa} ' in r.stdout and 'mismatched=0 failed=0' in r.stdout, r.stdout
