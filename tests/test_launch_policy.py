"""The stream loader's launch policy (csrc/gpu/launch_policy.h) under
AddressSanitizer + UBSan, as a stand-alone host program
(csrc/tests/launch_policy_check.cpp): the policy inside a discrete-event model
of the loader's worker, the GPU queue (a launch costs a fixed part plus a part
per image) and a consumer that posts each buffer again after a delay.

Swept: launch_depth 0..3 x 1, 2, 4, 8 output buffers x 1..40 batches per stream
x batches of 8 and 3 images x GPU-bound, producer-bound and random arrivals x
no / every third batch on the copy path -- 7680 streams, the GPU-bound ones
ending with batches held.  In every one each batch is launched once and
delivered in order (the model never stands with a batch pending, nothing in
flight and no flush), no launch exceeds 64 images, copy-path batches launch
alone and at once, and with launch_depth >= 2 the GPU queue never runs empty
while a batch is held; producer-bound streams launch every batch alone and
GPU-bound streams with 8 buffers launch fewer times than they have batches.
The same sweep without the policy's max(1, launch_depth) floor must hang."""
import os
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_launch_policy_check_asan_ubsan(tmp_path):
    exe = tmp_path / 'launch_policy_check'
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           str(ROOT / 'csrc/tests/launch_policy_check.cpp'), '-o', str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r'policy: runs=(\d+) failed=(\d+) stuck=(\d+) coalesced=(\d+) ended_held=(\d+) max_group=(\d+)', r.stdout)
    assert m, r.stdout
    runs, failed, stuck, coalesced, ended_held, max_group = (int(g) for g in m.groups())
    assert runs == 4 * 4 * 40 * 2 * 3 * 2 and failed == 0 and stuck == 0, r.stdout
    assert coalesced > 0 and ended_held > 0 and 2 <= max_group <= 8, r.stdout     # 8 batches of 8: the 64-image cap
    h = re.search(r'headline model: batches=40 launches=(\d+) max_group=(\d+) stuck=0', r.stdout)
    assert h and int(h[1]) < 40 and int(h[2]) >= 2, r.stdout
    mut = re.search(r'mutant \(no floor\): runs=(\d+) stuck=(\d+)', r.stdout)
    assert mut and int(mut[1]) == runs and int(mut[2]) > 0, r.stdout               # the launch_depth = 0 hang
    assert r.stdout.rstrip().endswith('PASS'), r.stdout
