"""Inputs and brute-force oracles shared by the prioritized-replay tests
(tests/test_replay_priority_cpu.py, tests/test_gpu_replay_priority.py).

The oracles know nothing of the tree: ``search_draw`` finds a slot with
``np.searchsorted`` on the exact cumulative sum of the masses, and ``Eligible``
keeps the mass of every frame an RL loop appended in a dict keyed by the frame's
global number -- no ring arithmetic, no levels."""
import numpy as np
import torch

from decode_oracle import frames
from nstep_cases import SEED, layout
from blendtorch import ops
from blendtorch.btt.replay import DeviceReplayBuffer

CAPACITIES = (50, 200, 5000)          # 1 level; 2 levels, padded; 3 levels, padded at two
TOP = 2 ** 32 - 1


def mass_patterns(cap, seed):
    """name -> uint32 [cap] masses."""
    rng = np.random.default_rng(seed)
    spread = np.rint(65536 * 10.0 ** rng.uniform(-1.5, 1.5, cap)).astype(np.uint32)
    spread[rng.random(cap) < 0.2] = 0                      # ineligible anchors in between
    single = np.zeros(cap, np.uint32)
    single[cap * 2 // 3] = 12345
    few = np.zeros(cap, np.uint32)                         # T = 3: fewer units of mass than images for B = 8, 256
    few[[1, cap // 2, cap - 1]] = 1
    top = np.ones(cap, np.uint32)
    top[cap // 3] = TOP
    tops = np.full(cap, TOP, np.uint32)                    # the largest total a store of this size can have
    return dict(spread=spread, single=single, few=few, top=top, tops=tops, empty=np.zeros(cap, np.uint32))


def strata_points(T, seed, counter, B):
    """The B points u of one stratified draw as Python ints (the contract of ops.reference_priority_draw)."""
    o0, o1, _, _ = ops._philox_blocks(seed, counter, B, 6)
    out = []
    for b in range(B):
        lo, hi = b * T // B, (b + 1) * T // B
        out.append(lo + ((((int(o0[b]) << 32) | int(o1[b])) * (hi - lo)) >> 64))
    return out


def search_draw(masses, seed, counter, B):
    """(index, mass, prob) by searchsorted on the exact cumulative sum."""
    masses = np.asarray(masses, np.uint32)
    cum = np.cumsum(masses.astype(np.uint64), dtype=np.uint64)      # < 2^45 for 5000 slots: exact
    T = int(cum[-1])
    if T == 0:
        return np.zeros(B, np.int64), np.zeros(B, np.uint32), np.zeros(B, np.float32)
    u = np.array(strata_points(T, seed, counter, B), np.uint64)
    index = np.searchsorted(cum, u, side='right').astype(np.int64)   # the first slot whose inclusive sum exceeds u
    mass = masses[index]
    prob = np.array([np.float32(int(m)) / np.float32(T) for m in mass], np.float32)   # both < 2^53: one rounding each
    return index, mass, prob


def rebuilt(levels):
    """The tree built from the leaves alone."""
    return ops.priority_tree(np.asarray(levels[0]))


def same_tree(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) and x.dtype == y.dtype
                                    for x, y in zip(a, b))


class Eligible:
    """The masses an RL loop's appends should leave behind, frame by frame: frame i lives in slot i % cap, it
    may be drawn once frame i + S is stored and is no ``first`` frame, and it takes the largest mass written
    so far at the moment it becomes drawable."""

    def __init__(self, cap, S, first):
        self.cap, self.S, self.first = cap, S, np.asarray(first) != 0
        self.total, self.max_mass, self.mass = 0, ops.PRIORITY_ONE, {}

    def append(self, n):
        for i in range(self.total, self.total + n):
            j = i - self.S                                   # the step before frame i
            if j >= 0 and not self.first[i]:
                self.mass[j] = self.max_mass
        self.total += n

    def write(self, slot, mass):
        """a priority update of the frame in `slot` (ignored unless drawable)."""
        f = self.frame(slot)
        if f is not None and f in self.mass:
            self.mass[f] = mass
            self.max_mass = max(self.max_mass, mass)

    def frame(self, slot):
        live = [i for i in range(max(0, self.total - self.cap), self.total) if i % self.cap == slot]
        return live[0] if live else None

    def leaves(self):
        out = np.zeros(self.cap, np.uint32)
        for s in range(self.cap):
            f = self.frame(s)
            # its successor must still be its own: frame f + S is stored (not yet overwritten: always, f is live)
            if f is not None and f + self.S < self.total:
                out[s] = self.mass.get(f, 0)
        return out


H, W, C = 8, 16, 3


def buffer(n, cap, S, seed, device='cpu', priority_alpha=1.0, steps=None):
    """A DeviceReplayBuffer an RL loop fills with nstep_cases.layout(n, S, seed), `steps` env steps per extend
    (default 1), with a 12-byte action column next to reward / done / first."""
    cols, _ = layout(n, S, seed)
    rng = np.random.default_rng(seed + 1)
    meta = dict(cols, action=rng.normal(size=(n, 3)).astype(np.float32))
    f = frames(n, H, W, C, seed=seed)
    rb = DeviceReplayBuffer(cap, device=device, seed=SEED, priority_alpha=priority_alpha, priority_stride=S)
    k = S * (steps or 1)
    for s in range(0, n, k):
        rb.extend(torch.from_numpy(f[s:s + k]), **{key: v[s:s + k] for key, v in meta.items()})
    return rb, (f, meta)
