"""Writes tests/golden/layout_golden.npz: what `slq_debug_csr_layout` decides for every pattern and setting of tests/_layout_cases.py
(perm, tile_row, xcd_tile, {have_tiles, ntiles, reordered, rms_dist} each), at one host thread.

Recorded from the library that introduced csrc/slq_layout.hpp, and committed only after scripts/op_fingerprint.py had shown that
library to build the same operators as its parent on the device (profiles/layout_ab.txt). The golden guards LATER changes of the
decision; it does not prove that one. Record it again only with a change that is meant to alter a layout, and say so.

    python tests/golden/make_golden_layout.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import _layout_cases as LC

out = {}
mats = LC.matrices()
for name in LC.EXPECT_TILES:
	for setting in LC.SETTINGS:
		d = LC.decide(mats[name], setting, threads=1)
		out.update(LC.flatten(name, setting, d))
		print(f"{name:12s} {setting:16s} tiles {d['ntiles']:5d} reordered {d['reordered']} rms |i-j| {d['rms_dist']:.2f}")
np.savez_compressed(ROOT / "tests" / "golden" / "layout_golden.npz", **out)
