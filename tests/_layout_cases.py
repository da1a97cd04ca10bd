"""The inputs of tests/test_layout_cpu.py and tests/golden/make_golden_layout.py: four small CSR patterns whose layout an existing GPU
test already relies on, the switch settings each is decided under, and the call of `slq_debug_csr_layout` (no device)."""

import ctypes as C
import os

import numpy as np

from primate_amd import _capi

# (name, builder, tiles expected under SLQ_TILES=2)
#  lap2d_96     __graft_entry__.smoke() relies on its ring tiles
#  lap3d_24     test_device_built_streams_equal_the_host_built_ones asserts tiles == 2
#  random_6000  the random graph of that same test: tiles == 0 (the 256-cluster sample turns it away)
#  lap2d_40     n < 4096: never tried
EXPECT_TILES = {"lap2d_96": True, "lap3d_24": True, "random_6000": False, "lap2d_40": False}
# the operator switches a case is decided under (every other SLQ_* switch unset), and plain = 1 (the affine operator's kind)
SETTINGS = {
	"tiles2": ({"SLQ_TILES": "2"}, 0),
	"tiles1": ({"SLQ_TILES": "1"}, 0),
	"tiles2_reorder0": ({"SLQ_TILES": "2", "SLQ_REORDER": "0"}, 0),
	"reorder2_tiles0": ({"SLQ_REORDER": "2", "SLQ_TILES": "0"}, 0),
	"plain": ({}, 1),
}


def matrices():
	import scipy.sparse as sp
	from conftest import laplacian_2d, laplacian_3d

	G = sp.random(6000, 6000, density=0.002, random_state=5, format="csr")
	G = (G + G.T + sp.identity(6000) * 10.0).tocsr()
	G.sort_indices()
	return {"lap2d_96": laplacian_2d(96), "lap3d_24": laplacian_3d(24), "random_6000": G, "lap2d_40": laplacian_2d(40)}


def decide(A, setting, threads=None):
	"""-> dict(perm, tile_row, xcd_tile, have_tiles, ntiles, reordered, rms_dist) as the library decides it under `setting`."""
	env, plain = SETTINGS[setting]
	saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("SLQ_")}  # (every switch of the library unset, whatever it is called)
	try:
		os.environ.update(env)
		if threads is not None:
			os.environ["SLQ_HOST_THREADS"] = str(threads)
		n = A.shape[0]
		rp, ci = np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32)
		perm, tile_row = np.full(n, -1, np.int32), np.full(n + 1, -1, np.int32)
		xcd, info = np.full(9, -1, np.int32), np.zeros(4)
		rc = _capi.lib().slq_debug_csr_layout(n, A.nnz, _capi.ptr(rp), _capi.ptr(ci), plain, _capi.ptr(perm), _capi.ptr(tile_row), n + 1, _capi.ptr(xcd), _capi.ptr(info))
		_capi.check(rc)
	finally:
		for k in [k for k in os.environ if k.startswith("SLQ_")]:
			del os.environ[k]
		os.environ.update(saved)
	have, ntiles, reordered = int(info[0]), int(info[1]), int(info[2])
	if not reordered:
		assert np.all(perm == -1)  # (nothing written)
	if not have:
		assert np.all(tile_row == -1)
	return dict(perm=perm[: n if reordered else 0].copy(), tile_row=tile_row[: ntiles + 1 if have else 0].copy(), xcd_tile=xcd.copy(),
	            have_tiles=have, ntiles=ntiles, reordered=reordered, rms_dist=float(info[3]))  # fmt: skip


def flatten(name, setting, d):
	"""the golden's entries of one decision"""
	pre = f"{name}/{setting}/"
	return {pre + "perm": d["perm"], pre + "tile_row": d["tile_row"], pre + "xcd_tile": d["xcd_tile"],
	        pre + "info": np.array([d["have_tiles"], d["ntiles"], d["reordered"], d["rms_dist"]])}  # fmt: skip
