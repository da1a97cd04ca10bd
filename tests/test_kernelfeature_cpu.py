"""Random Fourier features and pathwise posterior samples, what needs no GPU: the C-ABI symbols, the condition and
a NumPy emulation of the device evaluation inside the bar for every cell of the GPU table, faults the bar must notice, the frequency
law of the four profiles, the host `KernelFeatures`, the NumPy pathwise model against the exact posterior covariance, the moment
assertions of the GPU test on NumPy draws, the host schedule and every refusal raised before the library touches a device.
(scripts/kernelfeature_check.cpp runs the host part of csrc/slq_kernelfeature.hpp under the host sanitizers as a program of its own.)"""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _kernelfeature_ref as Fr
import _kernelop_ref as R
from primate_amd import _capi
from primate_amd.operators import KernelFeatures, KernelOperator, draw_kernel_frequencies

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_kernel_feature_create", "slq_kernel_feature_matmat", "slq_kernel_feature_dmat", "slq_kernel_feature_destroy",
			   "slq_debug_kernel_feature_frequencies", "slq_debug_kernel_feature_schedule")  # fmt: skip
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
	assert g.CSRC / "slq_kernelfeature.hpp" in units["slq"][1]
	src, deps = units["kernelfeature"]
	assert src == g.CSRC / "slq_kernelfeature.hip"
	for h in ("slq_kernelfeature.hpp", "slq_kernelcross.hpp", "slq_kernelop.hpp", "slq_kerneltile.hpp"):
		assert g.CSRC / h in deps, h


def test_the_feature_body_reuses_the_tile_walk_and_the_accurate_functions():
	"""The feature body lives in its own header on the shared walk, and takes sin and cos from the device library's accurate functions."""
	feat = (ROOT / "primate_amd" / "csrc" / "slq_kernelfeature.hpp").read_text()
	for used in ("KernelTile<F, DQ>", "T::rows(", "T::gram(", "T::stash(", "T::jr(", "kernel_tile_walk(", "kernel_for_ncb(", "kernel_for_dq(", "kernel_cross_schedule("):
		assert used in feat, used
	assert "__sinf" not in feat and "__cosf" not in feat and "native_" not in feat


## ---- the condition, and an emulation inside the bar, for every cell of the table ----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("m", [None, *Fr.CROSS_M], ids=["own", "m1", "m40", "m130"])
@pytest.mark.parametrize("idx", range(len(Fr.CASES)), ids=Fr.CASE_IDS)
def test_condition_and_emulation_for_every_cell(idx, m, dtype):
	for name in Fr.PROFILES:
		D = Fr.case_data(idx, name, dtype, m)
		ratio = Fr.check_condition(D["Y"], D["bar"], dtype)
		w = Fr.worst(Fr.emulate(D["z"], D["omega"], Fr.S, D["W"]), D["Y"], D["bar"])
		gmax = float(np.max(np.abs(Fr.phases(D["z"], D["omega"]))))
		print(f"{Fr.CASE_IDS[idx]} {name} rows {m or 'own'} {np.dtype(dtype).name}: bar / max |Y| = {ratio:.2e}, emulation / bar = {w:.3f}, max |g| = {gmax:.3g}")
		assert w <= 1.0, (Fr.CASE_IDS[idx], name, m, w)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_bar_notices_four_faults(dtype):
	idx = 2  # (130, 17, 1.5, 33, 5): a remainder tile of frequencies
	n, d, ls, f2, b = Fr.CASES[idx]
	for name in Fr.PROFILES:
		D = Fr.case_data(idx, name, dtype)
		w_swap = Fr.worst(Fr.emulate(D["z"], D["omega"], Fr.S, D["W"], swap=True), D["Y"], D["bar"])
		w_scale = Fr.worst(Fr.emulate(D["z"], D["omega"], Fr.S, D["W"], no_scale=True), D["Y"], D["bar"])
		## the padded frequencies of the last tile entering with cos 0 = 1 against a weight that is not 0
		pad = np.ones(16 * -(-f2 // 16) - f2, dtype=dtype)[:, None] * np.asarray(D["W"])[:1]
		w_pad = Fr.worst(Fr.emulate(D["z"], D["omega"], Fr.S, D["W"]) + np.sqrt(dtype(Fr.S) / dtype(f2)) * pad.sum(axis=0), D["Y"], D["bar"])
		## the remainder tile dropped
		W0 = np.array(D["W"])
		W0[f2 // 16 * 16 : f2] = 0
		W0[f2 + f2 // 16 * 16 :] = 0
		w_tile = Fr.worst(Fr.emulate(D["z"], D["omega"], Fr.S, W0), D["Y"], D["bar"])
		print(f"{name} {np.dtype(dtype).name}: swapped halves {w_swap:.3g}, no a {w_scale:.3g}, padding weighed {w_pad:.3g}, dropped tile {w_tile:.3g} times the bar")
		assert min(w_swap, w_scale, w_pad, w_tile) > 1e2


## ---- the frequency law --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Fr.PROFILES)
def test_frequency_law_reproduces_the_profile(name):
	"""max |Phi Phi^T - s phi(r2)| / s <= 0.077 at F2 = 4096: 7 sigma of a mean of 4096 terms cos(omega.(z - z')) of variance <= 1/2."""
	s = 1.5
	K = KernelOperator(R.points(300, 2, seed=21), name, lengthscale=0.4, outputscale=s, noise=0.1)
	Ft = K.features(4096, seed=5)
	assert isinstance(Ft, KernelFeatures) and Ft.omega.shape == (4096, 2) and Ft.omega.dtype == np.float64 and Ft.kernel == name
	assert np.array_equal(Ft.omega, Fr.frequencies(name, 4096, 2, 5))  # (the one defined order of draws)
	P = Ft.matrix()
	assert P.shape == (300, 8192)
	z = K.scaled_points().astype(np.float64)
	exact = (s * R.phi(name, R.r2_exact(z))).astype(np.float64)
	G = P @ P.T
	err = float(np.max(np.abs(G - exact)) / s)
	diag = float(np.max(np.abs(np.diag(G) - s)) / s)
	print(f"{name}: max |Phi Phi^T - s phi| / s = {err:.4f} at F2 = 4096, diagonal within {diag:.1e}")
	assert err <= 0.077
	assert diag <= 1e-12
	## the host value against the long-double model
	assert np.max(np.abs(P - Fr.feature_matrix(z, Ft.rounded(), s).astype(np.float64))) <= 1e-12


def test_a_wrong_degree_of_freedom_is_a_wrong_kernel():
	"""The law test discriminates: matern12's frequencies (one degree of freedom) against the matern52 profile miss the bound widely."""
	s = 1.5
	K = KernelOperator(R.points(300, 2, seed=21), "matern52", lengthscale=0.4, outputscale=s)
	z = K.scaled_points().astype(np.float64)
	P = K.features(frequencies=Fr.frequencies("matern12", 4096, 2, 5)).matrix()
	assert np.max(np.abs(P @ P.T - (s * R.phi("matern52", R.r2_exact(z))).astype(np.float64))) / s > 0.2


def test_frequencies_are_reproducible_and_round_trip():
	K = KernelOperator(R.points(20, 3, seed=1), "matern32", lengthscale=[0.5, 0.3, 0.8], dtype=np.float32)
	a, b, c = K.features(64, seed=9), K.features(64, seed=9), K.features(64, seed=10)
	assert np.array_equal(a.omega, b.omega) and not np.array_equal(a.omega, c.omega)
	assert np.array_equal(a.omega, draw_kernel_frequencies("matern32", 64, 3, np.random.default_rng(9)))
	back = K.features(frequencies=a.omega)
	assert np.array_equal(back.omega, a.omega) and back.omega is not a.omega and back.num_features == 64
	assert a.rounded().dtype == np.float32 and np.array_equal(a.rounded(), a.omega.astype(np.float32))
	## the map follows the operator's parameters of now: the lengthscales through z, the outputscale through a
	before = a.matrix()
	K.set_parameters(outputscale=4.0)
	assert np.allclose(a.matrix(), 2.0 * before, rtol=1e-15)
	with pytest.raises(ValueError, match=r"\(F2, 3\) array"):
		K.features(frequencies=np.ones((4, 2)))
	with pytest.raises(ValueError, match="frequency 1, coordinate 2 is inf"):
		K.features(frequencies=np.array([[0.0, 1, 2], [0, 1, np.inf]]))
	with pytest.raises(ValueError, match="num_features = 0"):
		K.features(0)
	with pytest.raises(ValueError, match="KernelOperator"):
		KernelFeatures(np.eye(3), np.ones((2, 3)))


## ---- the pathwise model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Fr.PROFILES)
def test_pathwise_model_covariance_tends_to_the_posterior(name):
	"""Given Omega the paths' covariance is (Phi* - C A^-1 Phi_X)(...)^T + noise C A^-2 C^T: within 0.05 s of the exact posterior
	covariance at F2 = 4096 (printed at 256, 1024 and 4096 for DESIGN.md §4.21)."""
	G = Fr.gp_case(name)
	errs = {}
	for f2 in (256, 1024, 4096):
		cov = Fr.path_cov_given_omega(G, Fr.frequencies(name, f2, 2, 5))
		errs[f2] = (float(np.max(np.abs(cov - G["cov"])) / Fr.S_GP), float(np.max(np.abs(np.diag(cov - G["cov"]))) / Fr.S_GP))
	print(f"{name}: max |cov(paths | Omega) - cov| / s (overall, diagonal): " + ", ".join(f"F2 = {f2}: {e[0]:.4f}, {e[1]:.4f}" for f2, e in errs.items()))
	assert errs[4096][0] <= 0.05


@pytest.mark.parametrize("name", ["rbf", "matern12"])
def test_moments_of_the_numpy_model_with_numpy_draws(name):
	G = Fr.gp_case(name)
	rng = np.random.default_rng(2024)
	om = Fr.frequencies(name, 1024, 2, 31)
	W, E = rng.standard_normal((2048, 512)), rng.standard_normal((Fr.N_GP, 512))
	F, _ = Fr.path_dense(G, om, W, E)
	r_mean, r_var = Fr.moments_hold(F, G, om)
	print(f"{name}: sample mean at {r_mean:.3f} of its 6-standard-error bar, sample variance at {r_var:.3f} of its bar (count = 512, F2 = 1024)")
	assert r_mean <= 1.0 and r_var <= 1.0


def test_path_gradient_formula_against_differences_of_the_model():
	"""The feature term's derivative as `PosteriorPaths.evaluate` builds it - a feature product on W'[j] = Omega_jk w_{F2+j},
	W'[F2+j] = -Omega_jk w_j, over the lengthscale - against central differences of the long-double model."""
	G = Fr.gp_case("matern52")
	om = Fr.frequencies("matern52", 64, 2, 3)
	W = np.random.default_rng(4).standard_normal((128, 3))
	Xq = np.array(G["Xnew"][5:10])
	h = 1e-5
	for k in range(2):
		e = np.zeros(2)
		e[k] = h
		fd = (Fr.path_value_ld(G, "matern52", om, W, None, Xq + e) - Fr.path_value_ld(G, "matern52", om, W, None, Xq - e)) / (2 * Fr.LD(h))
		Wk = np.vstack([om[:, k][:, None] * W[64:], -om[:, k][:, None] * W[:64]])
		mean = np.cumsum(G["X"], axis=0, dtype=np.float64)[-1] / G["X"].shape[0]
		zq = ((Xq - mean) / Fr.LS_GP)
		an = Fr.feature_matrix(zq, om, Fr.S_GP) @ Wk / Fr.LS_GP
		assert np.max(np.abs(an - fd)) <= 1e-6 * np.max(np.abs(fd))


## ---- the schedule -----------------------------------------------------------------------------------------------------------------------
def test_schedule_is_the_cross_schedule_with_narrower_chunks_in_fp64():
	from primate_amd.engine import kernel_cross_schedule, kernel_feature_schedule

	for n, d, ls, f2, b in Fr.CASES:
		for rows in (n, *Fr.CROSS_M):
			for cus in (256, 8):
				S32, S64, Sx = kernel_feature_schedule(rows, f2, b, cus, np.float32), kernel_feature_schedule(rows, f2, b, cus, np.float64), kernel_cross_schedule(rows, f2, b, cus)
				assert S32 == Sx
				assert S64["col_blocks"] <= 8 and (S64["chunks"] - 1) * 128 < b <= S64["chunks"] * 128
				if b <= 128:
					assert S64 == Sx
				for S in (S32, S64):
					bg, tps, ntiles = S["begin"], S["tiles_per_slab"], -(-f2 // 16)
					assert bg[0] == 0 and bg[-1] == f2 and all(x < y for x, y in zip(bg, bg[1:])) and all(v == -1 for v in S["rest"])
					assert [min(f2, 16 * min(ntiles, z * tps)) for z in range(S["slabs"] + 1)] == list(bg)
	S = kernel_feature_schedule(40, 1024, 16, 256)
	assert S["nrb"] == 1 and S["slabs"] > 8  # (one row block: the chip is fed by slabs)
	L = _capi.lib()
	out = (C.c_int64 * 71)()
	assert L.slq_debug_kernel_feature_schedule(100, 100, 64, 256, 1, out, 70) == _capi.SLQ_EINVAL
	for args in ((0, 100, 64, 256), (100, 0, 64, 256), (100, 100, 0, 256), (100, 100, 64, 0), (100, (1 << 30) + 1, 64, 256)):
		assert L.slq_debug_kernel_feature_schedule(*args, 1, out, 71) == _capi.SLQ_EINVAL, args


## ---- refusals that need no device -----------------------------------------------------------------------------------------------------
def test_raw_entries_refuse_null_handles_without_a_device():
	L = _capi.lib()
	h = C.c_void_p()
	buf = np.zeros(4)
	assert L.slq_kernel_feature_create(None, None, 1, _capi.ptr(buf), 1, C.byref(h)) == _capi.SLQ_EINVAL
	assert b"NULL" in L.slq_last_error()
	assert L.slq_kernel_feature_create(None, None, 1, _capi.ptr(buf), 1, None) == _capi.SLQ_EINVAL
	assert L.slq_kernel_feature_matmat(None, None, _capi.ptr(buf), 4, _capi.ptr(buf), 4, 1) == _capi.SLQ_EINVAL
	assert b"feature map is NULL" in L.slq_last_error()
	assert L.slq_kernel_feature_dmat(None, None, None, 0, None, 0, 1) == _capi.SLQ_EINVAL
	assert L.slq_debug_kernel_feature_frequencies(None, None) == _capi.SLQ_EINVAL
	assert L.slq_kernel_feature_destroy(None) == _capi.SLQ_OK


X5 = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 1.0], [6.0, 8.0], [3.0, 4.0]])


def test_python_refusals_before_any_device_call():
	import scipy.sparse as sp

	from primate_amd import engine, gp

	class _Op:
		kind, dtype = "csr", np.dtype(np.float64)

	with pytest.raises(ValueError, match="kind 'csr'"):
		engine.KernelFeatureMap(_Op(), np.ones((2, 2)))
	K = KernelOperator(X5, noise=0.1)
	with pytest.raises(ValueError, match="KernelOperator"):
		gp.sample_paths(sp.identity(5, format="csr"), np.ones(5))
	with pytest.raises(ValueError, match="fp64 only.*float32"):
		gp.sample_paths(KernelOperator(X5.astype(np.float32), noise=0.1), np.ones(5))
	with pytest.raises(ValueError, match="must be >= 1"):
		gp.sample_paths(K, np.ones(5), count=0)
	with pytest.raises(ValueError, match="must be >= 1"):
		gp.sample_paths(K, np.ones(5), deg=0)
	with pytest.raises(ValueError, match="precond_rank = -1"):
		gp.sample_paths(K, np.ones(5), precond_rank=-1)
	with pytest.raises(ValueError, match=r"y must be \(5,\)"):
		gp.sample_paths(K, np.ones((5, 2)))
	with pytest.raises(ValueError, match="finite"):
		gp.sample_paths(K, np.array([1.0, np.nan, 0, 0, 0]))
	with pytest.raises(ValueError, match=r"weights must be a finite \(2 F2, count\) = \(8, 3\)"):
		gp.sample_paths(K, np.ones(5), count=3, num_features=4, weights=np.ones((8, 2)))
	with pytest.raises(ValueError, match=r"noise_draws must be a finite \(n, count\) = \(5, 3\)"):
		gp.sample_paths(K, np.ones(5), count=3, num_features=4, noise_draws=np.ones((4, 3)))
	with pytest.raises(ValueError, match="features must be a KernelFeatures of this KernelOperator"):
		gp.sample_paths(K, np.ones(5), features=KernelOperator(X5).features(4, seed=1))
