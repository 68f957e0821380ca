"""The slot-delta report and the slot-mirror bookkeeping under AddressSanitizer
+ UBSan, as a stand-alone host program (csrc/tests/slot_delta_check.cpp): a
byte mirror updated only inside the rectangle the producer would report
(csrc/sim/raster.h ``changed_rect``), as reported and widened as the loader
widens it, stays equal to its ring buffer over 6 x 4 stamped frames for 3 and 4
channels, both row orders and both scenes; the same check with every rectangle
shrunk by one pixel reports mismatches; csrc/gpu/slot_mirror.h decides base
match, mismatch, first use, invalidate, empty and out-of-frame rectangles, the
byte budget and the widening at both frame edges."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRCS = ['csrc/tests/slot_delta_check.cpp', 'csrc/sim/raster.cpp']


def test_slot_delta_check_asan_ubsan(tmp_path):
    exe = tmp_path / 'slot_delta_check'
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           '-ffp-contract=off', '-pthread', *[str(ROOT / s) for s in SRCS], '-o', str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert 'mirror_mismatched=0 widened_mismatched=0 shrunk_detected=1 failed=0' in r.stdout
