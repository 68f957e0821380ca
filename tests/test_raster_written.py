"""The blocks ``sim::Renderer::render`` reports as stored into (csrc/sim/raster.h:
``written``) and the shadow pixels it leaves alone, under AddressSanitizer +
UBSan, as a stand-alone host program (csrc/tests/raster_written_check.cpp)
linked with the renderer, once per fill path (``BLENDTORCH_RASTER_ISA``).

Cube scene at 128x48 and 192x96, C = 3 and 4, both row orders, 3 and 8
rotating slots, 400 random poses each (the 3-slot runs stamped as ``cubesim
--stamp`` stamps), every 37th frame drawn twice running into one slot; a
falling_cubes lap on the non-deferred path.  Per frame: incremental bytes
equal a full render, a mirror fed only the reported blocks equals the slot, a
render over sentinel bytes outside the mask changes none of them, the mask is
a subset of the blocks of both frames' spans (equal to them for
falling_cubes), a repeated pose reports no shadow-only block; per run the mean
mask share lies strictly below the span masks'."""
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
RUNS = 2 * 2 * 2 * 2          # sizes x channels x row orders x slot counts


def _has_avx2():
    try:
        with open('/proc/cpuinfo') as f:
            return any(line.startswith('flags') and ' avx2' in line for line in f)
    except OSError:
        return False


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp('raster_written') / 'raster_written_check'
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=undefined', str(ROOT / 'csrc/tests/raster_written_check.cpp'),
           str(ROOT / 'csrc/sim/raster.cpp'), str(ROOT / 'csrc/sim/physics.cpp'), '-o', str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return out


@pytest.mark.parametrize('isa', ['scalar', 'avx2'])
def test_written_blocks_asan_ubsan(exe, isa):
    if isa == 'avx2' and not _has_avx2():
        pytest.skip('this CPU has no AVX2')
    env = dict(os.environ, BLENDTORCH_RASTER_ISA=isa, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1',
               UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    runs = re.findall(r'^cube (\d+)x(\d+) C=(\d) (\S+) slots=(\d) isa=(\w+): frames=(\d+) mask_share=([\d.]+) '
                      r'span_share=([\d.]+) kept_blocks=(\d+) repeats=(\d+)', r.stdout, re.M)
    assert len(runs) == RUNS and len(set(runs)) == RUNS, r.stdout
    for run in runs:
        assert run[5] == isa and int(run[6]) >= 400 and int(run[9]) > 0 and int(run[10]) == 10, run
    falling = re.findall(r'^falling_cubes \S+ C=\d \S+ isa=\w+: frames=(\d+) mask_share=([\d.]+) span_share=([\d.]+)',
                         r.stdout, re.M)
    assert len(falling) == 2 and all(int(f[0]) >= 90 and f[1] == f[2] for f in falling), r.stdout
    assert re.search(r'^checks: failed=0 isa=%s$' % isa, r.stdout, re.M), r.stdout
    assert r.stdout.rstrip().endswith('PASS'), r.stdout
