"""cubesim's render workers (csrc/sim/cubesim.cpp ``--render-threads``): frames
are drawn by T workers and retired strictly in dispatch order, so a consumer
receives the same sequence of (btid, frameid, seq, xy, image bytes) for T = 1
and T = 2 with the same seed -- over a shared-memory ring and inline --,
``--frames N`` delivers exactly N frames, ``--fault exit --fault-after k``
delivers the same k frames, and a ThreadSanitizer build streaming 300 frames
with 2 workers reports nothing."""
import os
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest

from blendtorch import btt
from blendtorch.transport import shm, zmq

ROOT = Path(__file__).resolve().parent.parent
CLANG = '/opt/rocm/lib/llvm/bin/clang++'
SRCS = ['csrc/sim/cubesim.cpp', 'csrc/sim/raster.cpp', 'csrc/sim/physics.cpp', 'csrc/transport/zmtp.cpp',
        'csrc/transport/shmring.cpp', 'csrc/codec/pickle_codec.cpp', 'csrc/codec/xform_fit.cpp']
N = 300
# (--linger: what is queued when the producer ends is still delivered)
BASE = ['--mode', 'rgba', '--resolution', '128x64', '--stamp', '--linger', '5000']
_cache = {}


def _drain(addr, n=None, proc=None, timeout_s=30.0):
    """The first ``n`` frames of one producer in arrival order; ``n`` None: every frame until the producer
    process ``proc`` has ended and nothing more arrives."""
    out = []
    s = zmq.Context().socket(zmq.PULL)
    s.connect(addr)
    t0 = time.time()
    try:
        while n is None or len(out) < n:
            assert time.time() - t0 < timeout_s, f'stream stalled after {len(out)} frames'
            ended = n is None and proc.poll() is not None                      # (looked at before the poll)
            if not s.poll(100):
                if ended:
                    break
                continue
            msg = s.recv_pyobj()
            if shm.KEY in msg:
                msg = shm.resolve(msg, strict=True)
            out.append((int(msg['btid']), int(msg['frameid']), int(msg['seq']), np.asarray(msg['xy']).tobytes(),
                        np.asarray(msg['image']).tobytes()))
    finally:
        s.close()
    return out


def _stream(port, threads, ring, extra=(), n=None, frames=N):
    key = (threads, ring, tuple(extra), n, frames)
    if key not in _cache:
        args = BASE + (['--shm', '4'] if ring else []) + ['--render-threads', str(threads), '--frames', str(frames), *extra]
        with btt.BlenderLauncher(producer='cubesim', num_instances=1, named_sockets=['DATA'], start_port=port,
                                 proto='ipc', seed=5, instance_args=[args]) as bl:
            _cache[key] = _drain(bl.launch_info.addresses['DATA'][0], n, bl.launch_info.processes[0])
    return _cache[key]


@pytest.mark.parametrize('ring', [True, False], ids=['ring', 'inline'])
def test_same_stream_for_one_and_two_workers(free_port, ring):
    one = _stream(free_port, 1, ring, n=N)
    two = _stream(free_port + 5, 2, ring, n=N)
    assert len(one) == len(two) == N
    assert [f[2] for f in one] == list(range(N))                               # seq: dispatch order is arrival order
    for i, (a, b) in enumerate(zip(one, two)):
        assert a[:3] == b[:3] and a[3] == b[3], f'frame {i}: metadata {a[:3]} vs {b[:3]}'
        assert a[4] == b[4], f'frame {i}: image bytes differ'
    assert len({f[4][16:] for f in one}) > 100                                  # the poses do differ


@pytest.mark.parametrize('threads', [1, 2])
def test_frames_n_delivers_exactly_n(free_port, threads):
    got = _stream(free_port, threads, True, frames=37)                          # drained until the producer has ended
    assert [f[2] for f in got] == list(range(37))


def test_fault_exit_delivers_the_same_frames(free_port):
    # paced: the producer dies on the spot, so every frame before the fault needs time to leave its socket
    extra = ('--fault', 'exit', '--fault-after', '23', '--fps', '500')
    one = _stream(free_port, 1, True, extra=extra)
    two = _stream(free_port + 5, 2, True, extra=extra)
    assert [f[2] for f in one] == list(range(23))
    assert one == two


def test_two_workers_under_tsan(tmp_path, free_port):
    """cubesim is a process of its own: built with ThreadSanitizer into a temporary directory and
    streamed to a plain Python consumer, nothing preloaded."""
    cxx = CLANG if os.path.exists(CLANG) else 'g++'
    exe = tmp_path / 'cubesim_tsan'
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=thread', '-pthread', '-ffp-contract=off',
           *[str(ROOT / s) for s in SRCS], '-o', str(exe), '-lrt']
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and ('tsan' in b.stderr.lower() or 'sanitize' in b.stderr.lower()):
        pytest.skip('the toolchain has no ThreadSanitizer runtime')
    assert b.returncode == 0, b.stderr[-4000:]
    addr = f'ipc:///tmp/blendtorch-tsan-{os.getpid()}-{free_port}'
    env = dict(os.environ, TSAN_OPTIONS='halt_on_error=1 second_deadlock_stack=1')
    p = subprocess.Popen([str(exe), '-btid', '0', '-btseed', '5', '-btsockets', f'DATA={addr}', *BASE, '--shm', '4',
                          '--render-threads', '2', '--frames', str(N)],
                         stderr=subprocess.PIPE, text=True, env=env)
    try:
        got = _drain(addr, N)
        _, err = p.communicate(timeout=60)
    finally:
        if p.poll() is None:
            p.kill()
    assert 'ThreadSanitizer' not in err, err[-4000:]
    assert p.returncode == 0, err[-4000:]
    assert [f[2] for f in got] == list(range(N))
    assert len({f[4][16:] for f in got}) > 100
