"""Inputs and the brute-force oracle shared by the n-step replay tests
(tests/test_replay_nstep_cpu.py, tests/test_gpu_replay_nstep.py).

``layout`` plays ``S`` environments in lockstep through a fixed schedule of
episodes -- some terminated (``done`` on their last step), some merely truncated,
one of a single frame -- and returns the metadata columns an RL loop would store
plus the episodes as per-environment Python lists.  ``simulate`` answers an
anchor slot from those lists alone, one transition at a time with its own
float32 accumulation: no ring arithmetic and no flag walk in it."""
import numpy as np
import torch

from decode_oracle import frames
from blendtorch.btt.replay import DeviceReplayBuffer

SEED = 0x9E3779B97F4A7C15
# (frames, terminated) of consecutive episodes, per environment; the schedules repeat
SCHEDULES = ([(7, True), (3, False), (1, False), (4, True), (2, True), (6, False)],
             [(3, True), (7, False), (2, False), (8, True), (1, True), (4, False)])


def layout(n, S, seed):
    """n frames of S environments (frame i: step i // S of environment i % S).  Returns
    ``(cols, episodes)``: cols the float32 ``reward``, uint8 ``done`` and uint8 ``first`` columns [n];
    episodes[e] a list of episodes, each a list of dicts (frame, reward, done) in time order."""
    rng = np.random.default_rng(seed)
    reward = rng.normal(size=n).astype(np.float32)
    done, first = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    episodes = []
    for e in range(S):
        sched, eps, q, i = SCHEDULES[e % len(SCHEDULES)], [], 0, e
        while i < n:
            length, term = sched[q % len(sched)]
            q += 1
            ep = []
            for pos in range(length):
                if i >= n:
                    break
                first[i] = pos == 0
                # the step from the last but one frame reaches the terminal observation
                done[i] = term and pos == length - 2
                ep.append(dict(frame=i, reward=reward[i], done=bool(done[i])))
                i += S
            eps.append(ep)
        episodes.append(eps)
    return dict(reward=reward, done=done, first=first), episodes


def cpu_buffer(n, cap, H, W, C, S, seed):
    """The CPU DeviceReplayBuffer an RL loop fills with ``layout(n, S, seed)``, one extend per step, with a
    12-byte and a 5-byte metadata column next to reward / done / first.  Returns ``(buffer, episodes)``."""
    cols, episodes = layout(n, S, seed)
    rng = np.random.default_rng(seed + 1)
    meta = dict(cols, action=rng.normal(size=(n, 3)).astype(np.float32),
                tag=rng.integers(0, 256, size=(n, 5), dtype=np.uint8))
    f = frames(n, H, W, C, seed=seed)
    rb = DeviceReplayBuffer(cap, device='cpu', seed=SEED)
    for s in range(0, n, S):
        rb.extend(f[s:s + S], **{k: v[s:s + S] for k, v in meta.items()})
    rb.total = n
    return rb, episodes


def simulate(slot, episodes, total, cap, S, n, gamma, k, use_done):
    """The n-step transition anchored at ring slot `slot` after `total` frames went into a ring of `cap`:
    dict(valid, steps, ret, discount, terminated, succ_frame, cut, next_frames) -- frames as global frame
    numbers (frame i lives in slot i % cap); cut: why the walk ended before n steps ('first', 'newest',
    'done' or None); next_frames: the k frames of the next stack, oldest first (None if invalid)."""
    oldest = max(0, total - cap)
    cand = [i for i in range(oldest, total) if i % cap == slot]
    out = dict(valid=False, steps=0, ret=np.float32(0), discount=np.float32(0), terminated=False, succ_frame=None,
               cut=None, next_frames=None)
    if not cand:
        return out
    i = cand[0]
    ep = next(ep for ep in episodes[i % S] if ep[0]['frame'] <= i <= ep[-1]['frame'])
    pos = (i - ep[0]['frame']) // S
    if pos + 1 >= len(ep):   # the episode's last frame (so far): no step was taken from it, or its result is not stored
        return out
    g, R, m = np.float32(1), np.float32(0), 0
    gamma = np.float32(gamma)
    cut = None
    while True:
        R = np.float32(R + np.float32(g * ep[pos]['reward']))
        g = np.float32(g * gamma)
        m += 1
        ended = use_done and ep[pos]['done']
        pos += 1
        if m == n:
            break
        if ended:
            cut = 'done'
            break
        if pos + 1 >= len(ep):
            # the next frame of this environment starts another episode -- or does not exist yet
            cut = 'first' if ep[pos]['frame'] + S < total else 'newest'
            break
    start = next(p for p in range(len(ep)) if ep[p]['frame'] >= oldest)   # older frames were overwritten
    nxt = [ep[max(pos - (k - 1 - f), start)]['frame'] for f in range(k)]
    out.update(valid=True, steps=m, ret=R, discount=np.float32(0) if ended else g, terminated=bool(ended),
               succ_frame=ep[pos]['frame'], cut=cut, next_frames=nxt)
    return out


def classes(steps, valid, discount, anchor, head, size, cap, S, n, first, has_done):
    """The classes of images in one reference result (ops.nstep_transitions' outputs and the flags alone)."""
    got = set()
    age0 = (head - 1 - anchor) % cap
    for b in range(len(anchor)):
        m = int(steps[b])
        if not valid[b]:
            got.add('invalid')
        elif m == n:
            got.add('full')
        elif has_done and discount[b] == 0:
            got.add('terminated')
        elif age0[b] - m * S < S:
            got.add('newest')
        elif first[(anchor[b] + (m + 1) * S) % cap] != 0 and 1 < m < n:
            got.add('first')
    return got


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8) if isinstance(x, np.ndarray) else \
        x.contiguous().view(torch.uint8).reshape(-1).numpy()
