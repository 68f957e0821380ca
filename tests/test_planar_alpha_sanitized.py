"""The rgb_a slot layout under AddressSanitizer + UBSan, as a stand-alone host
program (csrc/tests/planar_alpha_check.cpp): the 3-channel incremental render
into a planar slot, re-interleaved, equals a fresh 4-channel render for 200
random poses in both row orders; the interleave helper and its range check
stay inside exact-size heap buffers; a version-1 ring header is refused."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRCS = ['csrc/tests/planar_alpha_check.cpp', 'csrc/sim/raster.cpp', 'csrc/transport/shmring.cpp']


def test_planar_alpha_check_asan_ubsan(tmp_path):
    exe = tmp_path / 'planar_alpha_check'
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           '-ffp-contract=off', '-pthread', *[str(ROOT / s) for s in SRCS], '-o', str(exe), '-lrt']
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert 'mismatched_upper=0 mismatched_lower=0 failed=0' in r.stdout
