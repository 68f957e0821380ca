"""The changed-block report, the slot mirror's block decision and the descriptor
scan's 11th element under AddressSanitizer + UBSan, as a stand-alone host
program (csrc/tests/slot_blocks_check.cpp): a byte mirror updated only inside
the set blocks of the mask a producer would send (csrc/sim/raster.h
``span_blocks``: the blocks of the slot's previous spans OR-ed with the new
ones), taken through the wire format, the scan and ``mirror::Ring::
decide_blocks``, stays equal to its ring buffer over 8 x 3 random stamped
poses at 128x48, 256x40 and 640x96, 3 and 4 channels, both row orders and both
scenes; the same with one set bit cleared per mask reports mismatches; 96x48
(W % 64 != 0) carries no mask; the bookkeeping decides reported mask,
rectangle fallback, all ones, foreign grids and malformed reports; and the
scan of truncated and mutated messages stays inside its buffer and agrees with
the full parse."""
import os
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRCS = ['csrc/tests/slot_blocks_check.cpp', 'csrc/sim/raster.cpp', 'csrc/codec/pickle_codec.cpp']


def test_slot_blocks_check_asan_ubsan(tmp_path):
    exe = tmp_path / 'slot_blocks_check'
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           '-ffp-contract=off', '-pthread', *[str(ROOT / s) for s in SRCS], '-o', str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert 'mask_mismatched=0 cleared_detected=1 failed=0' in r.stdout
    m = re.search(r'frames=(\d+) reports=(\d+) mean_fraction=([0-9.]+) scans=(\d+) mutated=(\d+) parse_threw=(\d+)', r.stdout)
    assert m, r.stdout
    frames, reports, fraction, scans, mutated = int(m[1]), int(m[2]), float(m[3]), int(m[4]), int(m[5])
    assert frames == 4 * 8 * 24 and reports > 300 and scans >= reports and mutated > 8000, r.stdout
    # inputs the scan accepted and the full parse refused (an opcode planted below the top level, whose
    # target the scan does not check): reported by the program, and rare -- under 1 % of the mutations
    assert int(m[6]) * 100 < mutated, r.stdout
    assert fraction < 1.0, r.stdout                                            # the masks are no whole frames
