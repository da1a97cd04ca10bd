"""The adjoint feature product and weight-space GP regression, what needs no GPU: the C-ABI symbols, the condition
and a NumPy emulation of the device evaluation inside the bar for every cell of the GPU table, four faults the bar must notice, the
host schedule, the dense weight-space model of `gp.feature_posterior` against the dense function-space model, and every refusal
raised before the library touches a device. (scripts/kernelfeatureadj_check.cpp runs the host part of
csrc/slq_kernelfeatureadj.hpp under the host sanitizers as a program of its own.)"""

import re
from pathlib import Path

import numpy as np
import pytest

import _kernelfeature_ref as Fr
import _kernelfeatureadj_ref as Ar
import _kernelop_ref as R
from primate_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_kernel_feature_rmatmat", "slq_kernel_feature_rdmat", "slq_debug_kernel_feature_adjoint_schedule")
DTYPES = (np.float64, np.float32)
CELLS = [(idx, m) for idx in range(len(Ar.CASES)) for m in Ar.rows_of(idx)]
CELL_IDS = [f"{Ar.CASE_IDS[idx]}-{'own' if m is None else f'm{m}'}" for idx, m in CELLS]


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
	assert g.CSRC / "slq_kernelfeatureadj.hpp" in units["slq"][1]
	src, deps = units["kernelfeatureadj"]
	assert src == g.CSRC / "slq_kernelfeatureadj.hip"
	for h in ("slq_kernelfeatureadj.hpp", "slq_kernelfeature.hpp", "slq_kernelcross.hpp", "slq_kernelop.hpp", "slq_kerneltile.hpp"):
		assert g.CSRC / h in deps, h


def test_the_adjoint_body_reuses_the_tile_walk_and_the_accurate_functions():
	adj = (ROOT / "primate_amd" / "csrc" / "slq_kernelfeatureadj.hpp").read_text()
	for used in ("KernelTile<F, DQ>", "T::gram(", "T::stash(", "T::jr(", "kernel_tile_walk(", "kernel_sincos(", "kernel_for_ncb(", "kernel_for_dq(", "kernel_cross_schedule(", "KernelColumnLayout"):
		assert used in adj, used
	assert "__sinf" not in adj and "__cosf" not in adj and "native_" not in adj and "atomicAdd" not in adj


## ---- the condition, and an emulation inside the bar, for every cell of the table ----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("idx,m", CELLS, ids=CELL_IDS)
def test_condition_and_emulation_for_every_cell(idx, m, dtype):
	for name in Ar.PROFILES:
		D = Ar.case_data(idx, name, dtype, m)
		ratio = Ar.check_condition(D["Z"], D["bar"], name, dtype)
		w = Ar.worst(Ar.emulate(D["z"], D["omega"], Ar.S, D["U"]), D["Z"], D["bar"])
		print(f"{Ar.CASE_IDS[idx]} {name} rows {m or 'own'} {np.dtype(dtype).name}: bar / max |Z| = {ratio:.2e}, emulation / bar = {w:.3f}")
		assert w <= 1.0, (Ar.CASE_IDS[idx], name, m, w)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_bar_notices_four_faults(dtype):
	"""Cosine and sine row blocks swapped, a left out, the padded points of the last tile weighed with cos 0 = 1 against a non-zero U,
	the remainder tile of points dropped: each above 10 bars on cell (130, 17, 1.5, 33, 5), in every law."""
	idx = Ar.MUTANT_CASE
	assert Ar.CASES[idx] == (130, 17, 1.5, 33, 5)
	for name in Ar.PROFILES:
		D = Ar.case_data(idx, name, dtype)
		w = {f: Ar.worst(Ar.emulate(D["z"], D["omega"], Ar.S, D["U"], fault=f), D["Z"], D["bar"]) for f in ("swap", "no_scale", "padding", "drop_tail")}
		print(f"{name} {np.dtype(dtype).name}: " + ", ".join(f"{f} {v:.3g}" for f, v in w.items()) + " times the bar")
		assert min(w.values()) > 10.0, w


## ---- the schedule -------------------------------------------------------------------------------------------------------------------
def _check_partitions(S, f2, nrows, b, dtype):
	chunk = 128 if np.dtype(dtype) == np.float64 else 256
	assert S["rows"] == 128 and S["nrb"] == -(-f2 // 128)
	assert S["col_blocks"] in (1, 2, 4, 8, 16) and (np.dtype(dtype) != np.float64 or S["col_blocks"] <= 8)
	assert 16 * S["col_blocks"] >= min(b, chunk) and S["chunks"] == -(-b // chunk)
	assert S["chunks"] == 1 or 16 * S["col_blocks"] == chunk
	begin = S["begin"]
	assert len(begin) == S["slabs"] + 1 and begin[0] == 0 and begin[-1] == nrows and all(v == -1 for v in S["rest"])
	ntiles = -(-nrows // 16)
	for z in range(S["slabs"]):
		assert begin[z] < begin[z + 1] and begin[z] % 16 == 0
		t0 = min(ntiles, z * S["tiles_per_slab"])  # the kernel's own range of slab z
		t1 = min(ntiles, t0 + S["tiles_per_slab"])
		assert min(nrows, 16 * t0) == begin[z] and min(nrows, 16 * t1) == begin[z + 1]
	assert S["slabs"] * S["tiles_per_slab"] >= ntiles and 1 <= S["slabs"] <= 64


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_schedule_partitions_on_every_table_shape(dtype):
	from primate_amd import engine

	several = 0
	for idx, m in CELLS:
		n, d, ls, f2, b = Ar.CASES[idx]
		nrows = n if m is None else m
		for cus in (1, 8, 256, 304):
			S = engine.kernel_feature_adjoint_schedule(f2, nrows, b, cus, dtype)
			_check_partitions(S, f2, nrows, b, dtype)
		several += engine.kernel_feature_adjoint_schedule(f2, nrows, b, 256, dtype)["slabs"] > 1
	assert several >= 1
	## the seventh cell: one row block and many slabs, the last one shorter (2000 points are 125 whole tiles: the remainder tile of
	## points is that of the cells with n = 17, 129, 130, 257, 300)
	S = engine.kernel_feature_adjoint_schedule(40, 2000, 3, 256, dtype)
	assert S["nrb"] == 1 and S["slabs"] > 8 and 125 % S["tiles_per_slab"] != 0
	S = engine.kernel_feature_adjoint_schedule(500, 257, 260, 256, dtype)
	assert S["chunks"] == (3 if np.dtype(dtype) == np.float64 else 2)
	with pytest.raises(ValueError, match="slq_debug_kernel_feature_adjoint_schedule"):
		engine.kernel_feature_adjoint_schedule(0, 10, 1)


## ---- the weight-space model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mll", [("rbf", -112.4972), ("matern12", -174.5966)])
def test_weight_space_model_agrees_with_function_space(name, mll):
	"""The dense NumPy weight-space model (M = Phi^T Phi + sigma2 I, 512 x 512) against the dense function-space model (A = Phi Phi^T +
	sigma2 I, 300 x 300) on gp_case with F2 = 256: mean and variance relative to their maxima, the mll relative, at 1e-9."""
	G = Fr.gp_case(name)
	om = Fr.frequencies(name, Ar.F2_GP, 2, Ar.FREQ_SEED_GP)
	Wm, Fm = Ar.weight_space_dense(G, om), Ar.function_space_dense(G, om)
	e_mean = float(np.max(np.abs(Wm["mean"] - Fm["mean"])) / np.max(np.abs(Fm["mean"])))
	e_var = float(np.max(np.abs(Wm["var"] - Fm["var"])) / np.max(np.abs(Fm["var"])))
	e_mll = abs(Wm["mll"] / Fm["mll"] - 1.0)
	print(f"{name}: mean {e_mean:.1e}, variance {e_var:.1e}, mll {e_mll:.1e} (mll = {Wm['mll']:.4f})")
	assert e_mean <= 1e-9 and e_var <= 1e-9 and e_mll <= 1e-9
	assert abs(Wm["mll"] - mll) < 1e-3
	## the feature model is an approximation of the exact GP: the distance is a property of the method (printed, not asserted)
	print(f"{name}: feature mean at {np.max(np.abs(Wm['mean'] - G['mean'])) / np.max(np.abs(G['mean'])):.2f} of max |mean| from the exact posterior mean at F2 = {Ar.F2_GP}")


## ---- refusals raised before the library touches a device ----------------------------------------------------------------------------
def test_feature_posterior_refusals_need_no_device():
	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	X = R.points(30, 2, seed=3)
	y = np.sin(X[:, 0])
	K = KernelOperator(X, "rbf", lengthscale=0.4, noise=0.1)
	with pytest.raises(ValueError, match="needs a KernelOperator"):
		gp.feature_posterior(np.eye(3), np.ones(3))
	with pytest.raises(ValueError, match="fp64 only"):
		gp.feature_posterior(KernelOperator(X.astype(np.float32), "rbf", lengthscale=0.4, noise=0.1, dtype=np.float32), y)
	with pytest.raises(ValueError, match=r"y must be \(30,\)"):
		gp.feature_posterior(K, np.ones((30, 2)))
	with pytest.raises(ValueError, match="y must be finite"):
		gp.feature_posterior(K, np.where(np.arange(30) == 4, np.nan, y))
	with pytest.raises(ValueError, match="noise > 0.*singular when 2 F2 > n"):
		gp.feature_posterior(KernelOperator(X, "rbf", lengthscale=0.4, noise=0.0), y)
	with pytest.raises(ValueError, match="exceed the limit of 8192"):
		gp.feature_posterior(K, y, num_features=4097)
	with pytest.raises(ValueError, match="exceed the limit of 8192"):
		gp.feature_posterior(K, y, features=K.features(4097, seed=1))
	with pytest.raises(ValueError, match="KernelFeatures of this KernelOperator"):
		gp.feature_posterior(K, y, features=KernelOperator(X, "rbf", lengthscale=0.4, noise=0.1).features(8, seed=1))
