"""The layout of a CSR operator - row order and tiles - decided without a device: `slq_debug_csr_layout` (csrc/slq_layout.hpp:
layout_prefilter + decide_layout), on four patterns whose outcome an existing GPU test already asserts (tests/_layout_cases.py),
each under SLQ_TILES=2, SLQ_TILES=1, SLQ_TILES=2 SLQ_REORDER=0, SLQ_REORDER=2 SLQ_TILES=0 and as a plain operator.

Checked on every decision: the invariants the kernels rely on (a permutation; tiles that partition the rows, never straddle one
of the eight XCD row chunks and, for the ring-fed kernels, keep to their caps), independence of the number of host threads, and
equality with tests/golden/layout_golden.npz. The golden was recorded from the library that introduced slq_layout.hpp, and
committed only after scripts/op_fingerprint.py had shown that library to build the same operators as its parent on the device
(profiles/layout_ab.txt): it guards later changes of the decision; it does not prove that one.
scripts/layout_check.cpp runs the same invariants, and the builders behind the decision, under the host sanitizers."""

import numpy as np
import pytest

import _layout_cases as LC
from conftest import ROOT

RING_ROWS, RING_COLS, RING_NNZ = 14, 36, 112  # kRingTileRows, kRingTileCols, kRingTileNnz (csrc/slq_format.hpp)


def test_caps_are_the_format_header_s():
	"""the literals above against csrc/slq_format.hpp"""
	import re

	txt = (ROOT / "primate_amd" / "csrc" / "slq_format.hpp").read_text()
	macro = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
	assert re.search(r"constexpr int kRingTileRows = SLQ_RING_ROWS;", txt) and macro("SLQ_RING_ROWS") == RING_ROWS
	assert re.search(r"constexpr int kRingTileCols = SLQ_RING_COLS;", txt) and macro("SLQ_RING_COLS") == RING_COLS
	assert int(re.search(r"constexpr int kRingTileNnz = (\d+);", txt).group(1)) == RING_NNZ


@pytest.fixture(scope="module")
def mats():
	return LC.matrices()


@pytest.fixture(scope="module")
def golden_layout():
	return np.load(ROOT / "tests" / "golden" / "layout_golden.npz")


def check_invariants(A, setting, d):
	n = A.shape[0]
	plain = LC.SETTINGS[setting][1]
	perm, tile_row, xcd = d["perm"], d["tile_row"], d["xcd_tile"]
	assert (len(perm) == 0) == (d["reordered"] == 0)
	if d["reordered"]:
		assert len(perm) == n and np.array_equal(np.sort(perm), np.arange(n))
	if plain:
		assert not d["reordered"] and not d["have_tiles"]
	assert np.all(np.diff(xcd) >= 0) and xcd[8] == d["ntiles"]
	if not d["have_tiles"]:
		assert d["ntiles"] == 0 and np.all(xcd == 0)
		return
	assert d["reordered"]  # (the tiles ARE a row order)
	assert len(tile_row) == d["ntiles"] + 1 and tile_row[0] == 0 and tile_row[-1] == n and np.all(np.diff(tile_row) > 0)
	chunk = (n + 7) // 8
	assert np.array_equal(tile_row[:-1] // chunk, (tile_row[1:] - 1) // chunk)  # no tile straddles a boundary of the row chunks
	for x in range(9):
		assert tile_row[xcd[x]] == min(n, x * chunk)  # ... and chunk x's tiles are [xcd_tile[x], xcd_tile[x + 1])
	if LC.SETTINGS[setting][0].get("SLQ_TILES") == "2":
		B = A.tocsr()[perm][:, perm].tocsr()  # the stored pattern
		B.sort_indices()
		rows = np.diff(tile_row)
		nnz = B.indptr[tile_row[1:]] - B.indptr[tile_row[:-1]]
		assert rows.max() <= RING_ROWS and nnz.max() <= RING_NNZ
		for t in range(d["ntiles"]):
			r0, r1 = tile_row[t], tile_row[t + 1]
			lines = np.union1d(np.arange(r0, r1), B.indices[B.indptr[r0] : B.indptr[r1]])
			assert len(lines) <= RING_COLS, (t, len(lines))


@pytest.mark.parametrize("setting", list(LC.SETTINGS))
@pytest.mark.parametrize("name", list(LC.EXPECT_TILES))
def test_layout(mats, golden_layout, name, setting):
	A = mats[name]
	d = LC.decide(A, setting, threads=1)
	check_invariants(A, setting, d)
	if setting == "tiles2":
		assert bool(d["have_tiles"]) == LC.EXPECT_TILES[name]
	if not LC.EXPECT_TILES[name]:  # (the random graph and the small grid get tiles under no setting)
		assert not d["have_tiles"]
	## the same whatever the number of host threads
	d16 = LC.decide(A, setting, threads=16)
	for k in d:
		assert np.array_equal(d[k], d16[k]), k
	## ... and as recorded
	for key, want in LC.flatten(name, setting, d).items():
		assert np.array_equal(golden_layout[key], want), key


def test_golden_has_nothing_else(golden_layout):
	assert set(golden_layout.files) == {k for name in LC.EXPECT_TILES for s in LC.SETTINGS for k in LC.flatten(name, s, dict.fromkeys(("perm", "tile_row", "xcd_tile", "have_tiles", "ntiles", "reordered", "rms_dist"), 0))}


def test_rejects_what_a_creation_rejects(mats, monkeypatch):
	"""the entry validates its pattern as slq_csr_create does, and says when the tile boundaries do not fit"""
	from primate_amd import _capi

	monkeypatch.setenv("SLQ_TILES", "2")
	A = mats["lap2d_96"]
	n = A.shape[0]
	rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
	perm, tr, xcd, info = np.zeros(n, np.int32), np.zeros(n + 1, np.int32), np.zeros(9, np.int32), np.zeros(4)
	call = lambda rp_, ci_, cap: _capi.lib().slq_debug_csr_layout(n, A.nnz, _capi.ptr(rp_), _capi.ptr(ci_), 0, _capi.ptr(perm), _capi.ptr(tr), cap, _capi.ptr(xcd), _capi.ptr(info))
	assert call(rp, ci, n + 1) == _capi.SLQ_OK
	bad = ci.copy()
	bad[7] = n
	assert call(rp, bad, n + 1) == _capi.SLQ_EINVAL
	bad = rp.copy()
	bad[3] = bad[4] + 1
	assert call(bad, ci, n + 1) == _capi.SLQ_EINVAL
	assert call(rp, ci, 10) == _capi.SLQ_EINVAL  # (this grid gets some 700 tiles)
