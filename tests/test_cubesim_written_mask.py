"""``cubesim`` reports, as a frame's block mask, the blocks its render stored
into (csrc/sim/raster.h: ``written``) instead of the blocks of both frames'
spans.  ``cubesim --bench`` checks the rule that the slot mirror rests on at
the headline size, 640x480 with random poses over 8 rotating slots:

* ``block_mirror_mismatched_bytes``: a byte mirror brought up to date only
  inside the reported blocks stays equal to the slot;
* ``stores_outside_mask``: the slot as it was, every byte outside the mask
  replaced by a sentinel, rendered again with a copy of the slot's record --
  no sentinel byte may change (two sentinel values: a store may write either).

``mask_share`` is the mean share of the frame the masks cover.  The span
union the producer sent before covers 0.3285 (``span_mask_share``, computed by
the same run from ``sim::span_blocks``); the blocks that hold a pixel whose
bytes really differ from the slot's previous frame cover 0.2824, which a rule
that never reads the slot cannot quite reach.  Bound: 0.30."""
import json
import subprocess
from pathlib import Path

import pytest

from blendtorch import btt

EXE = Path(btt.__file__).resolve().parents[1] / 'bin' / 'cubesim'
BOUND = 0.30


@pytest.mark.parametrize('layout', ['planar', 'interleaved'])
def test_bench_masks_hold_every_store(layout):
    out = subprocess.run([str(EXE), '--bench', '300', '--mode', 'rgba', '--origin', 'lower-left', '--resolution',
                          '640x480', '--shm-layout', layout, '-btseed', '3'],
                         capture_output=True, text=True, timeout=300)
    rep = json.loads(out.stdout)
    print(f"layout {layout}: mask_share {rep['mask_share']} span_mask_share {rep['span_mask_share']}")
    assert out.returncode == 0, out.stdout + out.stderr
    assert rep['frames'] == 300 and rep['mismatched_bytes'] == 0 and rep['mirror_mismatched_bytes'] == 0, rep
    assert rep['block_mirror_mismatched_bytes'] == 0 and rep['stores_outside_mask'] == 0, rep
    assert 0.31 < rep['span_mask_share'] < 0.35, rep          # the reference: what crossed the link before
    assert 0.0 < rep['mask_share'] < rep['span_mask_share'], rep
    assert rep['mask_share'] <= BOUND, rep
