"""Cross-covariance products of the kernel operator and GP prediction, what needs no GPU: the C-ABI symbols, the
condition and a NumPy emulation of the device evaluation inside half the bar for every cell of the GPU table, the host
`KernelCrossOperator` against the model, faults the bar must notice, the host schedule of a product, the raw entries on NULL handles
and every refusal raised before the library touches a device. (scripts/kernelcross_check.cpp runs the host part of
csrc/slq_kernelcross.hpp under the host sanitizers as a program of its own.)"""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _kernelcross_ref as X
import _kernelop_ref as R
from primate_amd import _capi
from primate_amd.operators import KernelCrossOperator, KernelOperator

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_kernel_cross_create", "slq_kernel_cross_create_device", "slq_kernel_cross_matmat", "slq_kernel_cross_dmat",
			   "slq_kernel_cross_destroy", "slq_debug_kernel_cross_points", "slq_debug_kernel_cross_schedule")  # fmt: skip
DTYPES = (np.float64, np.float32)


def test_symbols_are_declared_exported_and_bound():
	hdr = (ROOT / "include" / "slq.h").read_text()
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint {s}\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"
	assert L.slq_version() == 100


def test_the_build_lists_the_new_header_and_unit():
	import __graft_entry__ as g

	units = {name: (src, deps) for name, src, _, deps in g.UNITS}
	assert g.CSRC / "slq_kernelcross.hpp" in units["slq"][1]
	assert units["kernelcross"][0] == g.CSRC / "slq_kernelcross.hip" and g.CSRC / "slq_kernelcross.hpp" in units["kernelcross"][1]
	assert g.CSRC / "slq_kerneltile.hpp" in units["slq"][1] and g.CSRC / "slq_kerneltile.hpp" in units["kernelcross"][1]

	## every header of the kernel-operator family that a unit includes, directly or through another, is listed for that unit
	def included(path, seen):
		for name in re.findall(r'^#include "(slq_[a-z_]+\.hpp)"', path.read_text(), re.M):
			if g.CSRC / name not in seen:
				seen.add(g.CSRC / name)
				included(g.CSRC / name, seen)
		return seen

	for name in ("slq", "kernelcross"):
		src, deps = units[name]
		family = {h for h in included(src, set()) if h.name.startswith("slq_kernel") and h.name != "slq_kernels.hpp"}
		assert g.CSRC / "slq_kerneltile.hpp" in family
		assert family <= set(deps), (name, sorted(h.name for h in family - set(deps)))


## ---- the condition, and an emulation inside half the bar, for every cell of the table ---------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("trans", [False, True], ids=["forward", "adjoint"])
@pytest.mark.parametrize("idx", range(len(X.CASES)), ids=X.CASE_IDS)
def test_condition_and_emulation_for_every_cell(idx, trans, dtype):
	for name in X.PROFILES:
		D = X.case_data(idx, name, dtype, trans)
		ratio = X.check_condition(D["Y"], D["bar"], name, D["variant"], dtype)
		w = X.worst(X.emulate(D["zs"], D["z"], name, X.S, D["W"], trans), D["Y"], D["bar"])
		print(f"{X.CASE_IDS[idx]} {name} {'adjoint' if trans else 'forward'} {np.dtype(dtype).name}: bar / max |Y| = {ratio:.2e}, emulation / bar = {w:.3f}")
		assert w <= 0.5, (X.CASE_IDS[idx], name, trans, w)


def test_coincident_cases_hold_equal_points():
	for variant in ("coincident", "coincident_offset"):
		for dtype in DTYPES:
			Xt, Xn = X.case_points(48, 200, 3, variant, dtype)
			assert np.array_equal(Xn[:20], Xt[np.arange(20) * 7])
			z, zs = R.scaled_points(Xt, X.lengthscale_of(3), dtype), X.scaled_new_points(Xt, Xn, X.lengthscale_of(3), dtype)
			assert np.array_equal(zs[:20], z[np.arange(20) * 7])  # (the training centre: equal points stay equal)


## ---- the host operator against the model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idx", [1, 2, 4, 6], ids=[X.CASE_IDS[i] for i in (1, 2, 4, 6)])
def test_host_operator_products_and_transpose(idx, dtype):
	m, n, d, b, variant = X.CASES[idx]
	for name in X.PROFILES:
		Df, Da = X.case_data(idx, name, dtype, False), X.case_data(idx, name, dtype, True)
		K = KernelOperator(Df["X"], name, lengthscale=Df["ls"], outputscale=X.S, noise=0.3, dtype=dtype)
		Cx = K.cross(Df["Xnew"])
		assert isinstance(Cx, KernelCrossOperator) and Cx.shape == (m, n) and Cx.dtype == np.dtype(dtype)
		assert np.array_equal(Cx.scaled_points(), Df["zs"])
		assert Cx.T.shape == (n, m) and Cx.H.shape == (n, m) and Cx.T.T.shape == (m, n)
		wf = X.worst(Cx @ Df["W"], Df["Y"], Df["bar"])
		wa = X.worst(Cx.T @ Da["W"], Da["Y"], Da["bar"])
		wr = X.worst(Cx.rmatmat(Da["W"]), Da["Y"], Da["bar"])
		wv = X.worst(Cx.matvec(Df["W"][:, 0]), Df["Y"][:, 0], Df["bar"][:, 0])
		wtt = X.worst(Cx.T.T @ Df["W"], Df["Y"], Df["bar"])
		print(f"{X.CASE_IDS[idx]} {name} {np.dtype(dtype).name}: forward {wf:.3f} adjoint {wa:.3f} rmatmat {wr:.3f} matvec {wv:.3f} of the bar")
		assert max(wf, wa, wr, wv, wtt) <= 1.0


def test_host_operator_follows_set_parameters_and_has_no_noise():
	Xt, Xn = X.case_points(15, 17, 3, "plain", np.float64)
	K = KernelOperator(Xt, "matern32", lengthscale=0.7, outputscale=1.1, noise=0.5)
	Cx = K.cross(Xn)
	W = R.probes(17, 2)
	before = Cx @ W
	K.set_parameters(lengthscale=[0.5, 0.3, 0.8], outputscale=X.S)
	zs, z = X.scaled_new_points(Xt, Xn, [0.5, 0.3, 0.8], np.float64), R.scaled_points(Xt, [0.5, 0.3, 0.8], np.float64)
	Y, bar = X.model(zs, z, "matern32", X.S, W)
	assert X.worst(Cx @ W, Y, bar) <= 1.0 and not np.allclose(before, Cx @ W)
	K.set_parameters(noise=7.0)
	assert np.array_equal(Cx @ W, (Cx @ W))
	assert X.worst(Cx @ W, Y, bar) <= 1.0  # (no noise term)


## ---- faults the bar must notice -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_bar_notices_three_faults(dtype):
	idx = 2  # (129, 257, 3, 16)
	m, n, d, b, _ = X.CASES[idx]
	for name in X.PROFILES:
		D = X.case_data(idx, name, dtype, False)
		## the new points' own centre
		own = R.scaled_points(D["Xnew"], D["ls"], dtype)
		w_centre = X.worst(X.emulate(own, D["z"], name, X.S, D["W"]), D["Y"], D["bar"])
		## k_kernel_panel's diagonal rule applied to two different point sets
		k = np.arange(min(m, n))
		w_diag = X.worst(X.emulate(D["zs"], D["z"], name, X.S, D["W"], diagonal_rule=(k, k)), D["Y"], D["bar"])
		## the remainder tile of the summed points dropped
		W0 = np.array(D["W"])
		W0[n // 16 * 16 :] = 0
		w_tile = X.worst(X.emulate(D["zs"], D["z"], name, X.S, W0), D["Y"], D["bar"])
		print(f"{name} {np.dtype(dtype).name}: own centre {w_centre:.3g}, diagonal rule {w_diag:.3g}, dropped tile {w_tile:.3g} times the bar")
		assert w_centre > 1e2 and w_diag > 1e2 and w_tile > 1e2


## ---- the schedule ------------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 15, 16, 17, 127, 128, 129, 255, 257, 1000, 4097, 20000]


@pytest.mark.parametrize("nrows", SIZES)
def test_schedule_partitions_rows_points_and_columns(nrows):
	from primate_amd.engine import kernel_cross_schedule

	for nsum in SIZES:
		for b in (1, 16, 17, 65, 256, 260):
			for cus in (256, 8, 1):
				S = kernel_cross_schedule(nrows, nsum, b, cus)
				assert S["rows"] == 128 and S["nrb"] == -(-nrows // 128)
				first = min(b, 256)
				assert S["col_blocks"] in (1, 2, 4, 8, 16) and 16 * S["col_blocks"] >= first and (S["col_blocks"] == 1 or 8 * S["col_blocks"] < first)
				assert (S["chunks"] - 1) * 256 < b <= S["chunks"] * 256
				bg = S["begin"]
				ntiles = -(-nsum // 16)
				assert 1 <= S["slabs"] <= 64 and S["slabs"] <= ntiles and bg[0] == 0 and bg[-1] == nsum
				assert all(x < y for x, y in zip(bg, bg[1:])), "an empty slab"
				assert all(x % 16 == 0 for x in bg[:-1]) and all(v == -1 for v in S["rest"])
				## the kernel's slab range: tiles [z tps, (z + 1) tps) cut at the end
				tps = S["tiles_per_slab"]
				assert [min(nsum, 16 * min(ntiles, z * tps)) for z in range(S["slabs"] + 1)] == list(bg)
				assert S["slabs"] * tps >= ntiles


def test_schedule_splits_the_few_rows_of_a_forward_product():
	from primate_amd.engine import kernel_cross_schedule

	S = kernel_cross_schedule(128, 16384, 64, 256)
	assert S["nrb"] == 1 and S["slabs"] > 8  # (one row block: the chip is fed by slabs)
	assert kernel_cross_schedule(16384, 128, 64, 256)["slabs"] == 2  # (128 row blocks on 256 units: two slabs make one full round)
	assert kernel_cross_schedule(16384, 16384, 64, 256)["slabs"] == 2
	assert kernel_cross_schedule(32768, 128, 64, 256)["slabs"] == 1  # (256 row blocks: nothing to gain)


def test_schedule_entry_checks_its_arguments():
	L = _capi.lib()
	out = (C.c_int64 * 71)()
	assert L.slq_debug_kernel_cross_schedule(100, 100, 64, 256, out, 70) == _capi.SLQ_EINVAL
	assert L.slq_debug_kernel_cross_schedule(100, 100, 64, 256, None, 71) == _capi.SLQ_EINVAL
	for args in ((0, 100, 64, 256), (100, 0, 64, 256), (100, 100, 0, 256), (100, 100, 64, 0), (1 << 31, 100, 64, 256), (100, 1 << 31, 64, 256)):
		assert L.slq_debug_kernel_cross_schedule(*args, out, 71) == _capi.SLQ_EINVAL, args
	assert L.slq_debug_kernel_cross_schedule(100, 100, 64, 256, out, 71) == _capi.SLQ_OK


## ---- refusals that need no device -----------------------------------------------------------------------------------------------------
def test_raw_entries_refuse_null_handles_without_a_device():
	L = _capi.lib()
	h = C.c_void_p()
	buf = np.zeros(4)
	assert L.slq_kernel_cross_create(None, None, 1, _capi.ptr(buf), 1, C.byref(h)) == _capi.SLQ_EINVAL
	assert b"NULL" in L.slq_last_error()
	assert L.slq_kernel_cross_create(None, None, 1, _capi.ptr(buf), 1, None) == _capi.SLQ_EINVAL
	assert L.slq_kernel_cross_create_device(None, None, 1, None, 1, C.byref(h)) == _capi.SLQ_EINVAL
	assert L.slq_kernel_cross_matmat(None, 0, _capi.ptr(buf), 4, _capi.ptr(buf), 4, 1) == _capi.SLQ_EINVAL
	assert L.slq_kernel_cross_dmat(None, 0, None, 0, None, 0, 1) == _capi.SLQ_EINVAL
	assert L.slq_debug_kernel_cross_points(None, None, None) == _capi.SLQ_EINVAL
	assert L.slq_kernel_cross_destroy(None) == _capi.SLQ_OK


X5 = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 1.0], [6.0, 8.0], [3.0, 4.0]])


def test_python_refusals_of_the_cross_objects():
	from primate_amd import engine

	K = KernelOperator(X5, noise=0.1)
	with pytest.raises(ValueError, match=r"\(m, 2\) array"):
		K.cross(np.ones((3, 3)))
	with pytest.raises(ValueError, match=r"\(m, 2\) array"):
		K.cross(np.ones((0, 2)))
	with pytest.raises(ValueError, match="new point 1, coordinate 0 is nan"):
		K.cross(np.array([[0.0, 1.0], [np.nan, 2.0]]))
	with pytest.raises(ValueError, match="KernelOperator"):
		KernelCrossOperator(np.eye(3), np.ones((2, 2)))
	Cx = K.cross(np.ones((3, 2)))
	with pytest.raises(ValueError, match="dimension mismatch"):
		Cx.matmat(np.ones((4, 2)))
	with pytest.raises(ValueError, match="dimension mismatch"):
		Cx.T.matmat(np.ones((5, 2)))

	class _Op:
		kind, dtype = "csr", np.dtype(np.float64)

	with pytest.raises(ValueError, match="kind 'csr'"):
		engine.KernelCross(_Op(), np.ones((2, 2)))


def test_posterior_checks_its_arguments():
	import scipy.sparse as sp

	from primate_amd import gp

	K = KernelOperator(X5, noise=0.1)
	y, Xn = np.ones(5), np.ones((3, 2))
	with pytest.raises(ValueError, match="KernelOperator"):
		gp.posterior(sp.identity(5, format="csr"), y, Xn)
	with pytest.raises(ValueError, match="fp64 only.*float32"):
		gp.posterior(KernelOperator(X5.astype(np.float32), noise=0.1), y, Xn)
	with pytest.raises(ValueError, match="must be >= 1"):
		gp.posterior(K, y, Xn, deg=0)
	with pytest.raises(ValueError, match="must be >= 1"):
		gp.posterior(K, y, Xn, batch=0)
	with pytest.raises(ValueError, match=r"y must be \(5,\) or \(5, q\)"):
		gp.posterior(K, np.ones(4), Xn)
	with pytest.raises(ValueError, match=r"y must be \(5,\) or \(5, q\)"):
		gp.posterior(K, np.ones((5, 2, 1)), Xn)
	with pytest.raises(ValueError, match="finite"):
		gp.posterior(K, np.array([1.0, np.inf, 0, 0, 0]), Xn)
	with pytest.raises(ValueError, match=r"\(m, 2\) array"):
		gp.posterior(K, y, np.ones((3, 1)))
	with pytest.raises(ValueError, match="one batch"):
		gp.posterior(K, y, Xn, covariance=True, batch=2)
	with pytest.raises(ValueError, match="needs variance=True"):
		gp.posterior(K, y, Xn, covariance=True, variance=False)
