"""Random Fourier features of the kernel operator on the device (slq_kernelfeature.hpp: k_kernel_feature) against
the long-double model of tests/_kernelfeature_ref.py, elementwise within its forward bound - each cell first asserts that the bound is
a small fraction of the result - and `gp.sample_paths` against the dense NumPy pathwise model built from the same draws.

The shapes are the issue's table: the smallest shape, one exact tile of frequencies, a remainder tile with a second row block, several
slabs with a second column chunk in both dtypes (260 columns: 128-wide chunks in fp64, 256-wide in fp32), 64 tiles of frequencies, and
the deep-coordinate instantiation; each with the operator's own points as rows and with 1, 40 and 130 new points of a cross object.
Each item prints its worst ratio to the bar before it asserts (`-s`)."""

import ctypes as C
import gc

import numpy as np
import pytest

import _kernelfeature_ref as Fr
import _kernelop_ref as R

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def _operator(eng, D, name, dtype, ls=None, s=Fr.S, noise=0.25):
	from primate_amd.operators import KernelOperator

	K = KernelOperator(D["X"], name, lengthscale=D["ls"] if ls is None else ls, outputscale=s, noise=noise, dtype=dtype)
	return K, eng.DeviceOperator(K)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("idx", range(len(Fr.CASES)), ids=Fr.CASE_IDS)
def test_table_own_points_and_new_points_every_law(eng, idx, dtype):
	"""Y = Phi W through slq_kernel_feature_matmat within 1.0 bar of the model at the operator's points and at the new points of a cross
	object, after the device frequencies were found to be the rounded host ones bit for bit with zeros in the padding."""
	n, d, ls, f2, b = Fr.CASES[idx]
	for name in Fr.PROFILES:
		D = Fr.case_data(idx, name, dtype)
		K, op = _operator(eng, D, name, dtype)
		fmap = K.features(frequencies=D["omega64"]).device(op)
		crosses = []
		try:
			assert fmap.num_features == f2 and fmap.dtype == np.dtype(dtype)
			om = fmap.frequencies()
			assert np.array_equal(om, D["omega"]) and fmap.padding_is_zero and om.dtype == np.dtype(dtype)
			for m in (None, *Fr.CROSS_M):
				Dm = Fr.case_data(idx, name, dtype, m)
				ratio = Fr.check_condition(Dm["Y"], Dm["bar"], dtype)
				rows = None
				if m is not None:
					rows = eng.KernelCross(op, Dm["Xnew"])
					crosses.append(rows)
				got = fmap.matmat(Dm["W"], rows=rows)
				assert got.shape == (n if m is None else m, b) and got.dtype == np.dtype(dtype) and np.all(np.isfinite(got))
				w = Fr.worst(got, Dm["Y"], Dm["bar"])
				print(f"{Fr.CASE_IDS[idx]} {name} rows {m or 'own'} {np.dtype(dtype).name}: {w:.3f} of the bar (bar / max |Y| {ratio:.1e})")
				assert w <= 1.0, (Fr.CASE_IDS[idx], name, m, w)
		finally:
			for o in (*crosses, fmap, op):
				o.close()


@pytest.mark.parametrize("idx,m,slabs", [(1, None, 1), (4, 40, None)], ids=["one_slab", "several_slabs"])
def test_identical_calls_give_identical_bits(eng, idx, m, slabs):
	n, d, ls, f2, b = Fr.CASES[idx]
	for dtype in (F64, F32):
		S = eng.kernel_feature_schedule(n if m is None else m, f2, b, 256, dtype)
		assert S["slabs"] == 1 if slabs == 1 else S["slabs"] > 1, S
		D = Fr.case_data(idx, "matern12", dtype, m)
		K, op = _operator(eng, D, "matern12", dtype)
		fmap = eng.KernelFeatureMap(op, D["omega64"])
		rows = None if m is None else eng.KernelCross(op, D["Xnew"])
		try:
			first = fmap.matmat(D["W"], rows=rows)
			assert np.array_equal(first, fmap.matmat(D["W"], rows=rows))
			other = eng.KernelFeatureMap(op, D["omega64"])
			assert np.array_equal(first, other.matmat(D["W"], rows=rows))
			other.close()
		finally:
			if rows is not None:
				rows.close()
			fmap.close(), op.close()


@pytest.mark.parametrize("idx", [2, 3], ids=[Fr.CASE_IDS[2], Fr.CASE_IDS[3]])
def test_dmat_entry_equals_the_host_entry(eng, idx):
	n, d, ls, f2, b = Fr.CASES[idx]
	D, Dm = Fr.case_data(idx, "matern32", F64), Fr.case_data(idx, "matern32", F64, 40)
	K, op = _operator(eng, D, "matern32", F64)
	fmap = eng.KernelFeatureMap(op, D["omega64"])
	cross = eng.KernelCross(op, Dm["Xnew"])
	Wm, Nm, Mm = eng.DeviceMatrix(2 * f2, b + 3, ctx=op.ctx), eng.DeviceMatrix(n, b + 2, ctx=op.ctx), eng.DeviceMatrix(40, b + 2, ctx=op.ctx)
	try:
		Wm.set(3, D["W"])
		fmap.matmat_dmat(Wm, 3, Nm, 1, b)
		assert np.array_equal(Nm.get(1, b), fmap.matmat(D["W"]))
		assert not Nm.get(0, 1).any() and not Nm.get(b + 1, 1).any()  # (nothing outside the range)
		fmap.matmat_dmat(Wm, 3, Mm, 1, b, rows=cross)
		assert np.array_equal(Mm.get(1, b), fmap.matmat(D["W"], rows=cross))
		assert not Mm.get(0, 1).any() and not Mm.get(b + 1, 1).any()
	finally:
		for o in (Wm, Nm, Mm, cross, fmap, op):
			o.close()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_set_parameters_equals_a_fresh_pair(eng, dtype):
	idx = 1  # (17, 3, ., 16, 1): per-dimension lengthscales
	D, Dm = Fr.case_data(idx, "matern52", dtype), Fr.case_data(idx, "matern52", dtype, 40)
	new_ls, new_s = np.array([0.35, 0.6, 0.45]), 0.9
	K, op = _operator(eng, D, "matern52", dtype, ls=0.7, s=2.0)
	fmap, cross = eng.KernelFeatureMap(op, D["omega64"]), eng.KernelCross(op, Dm["Xnew"])
	K2, op2 = _operator(eng, D, "matern52", dtype, ls=new_ls, s=new_s)
	fresh, cross2 = eng.KernelFeatureMap(op2, D["omega64"]), eng.KernelCross(op2, Dm["Xnew"])
	W = R.probes(32, 7, seed=3, dtype=dtype)
	try:
		before, before_m = fmap.matmat(W), fmap.matmat(W, rows=cross)
		K.set_parameters(lengthscale=new_ls, outputscale=new_s)  # (KernelOperator.set_parameters: no code for the feature map)
		got, got_m = fmap.matmat(W), fmap.matmat(W, rows=cross)
		assert not np.array_equal(before, got) and not np.array_equal(before_m, got_m)
		assert np.array_equal(got, fresh.matmat(W)) and np.array_equal(got_m, fresh.matmat(W, rows=cross2))
		Y, bar = Fr.model(R.scaled_points(D["X"], new_ls, dtype), D["omega"], new_s, W)
		assert Fr.worst(got, Y, bar) <= 1.0
		K.set_parameters(noise=7.0)
		assert np.array_equal(fmap.matmat(W), got)  # (no noise term)
	finally:
		for o in (cross, cross2, fmap, fresh, op, op2):
			o.close()


def test_every_device_refusal_and_the_operator_is_untouched(eng):
	from primate_amd import _capi
	from primate_amd.engine import Context, DeviceMatrix, DeviceOperator

	L = _capi.lib()
	D, Dm = Fr.case_data(1, "rbf", F64), Fr.case_data(1, "rbf", F64, 40)
	n, d, ls, f2, b = Fr.CASES[1]  # (17, 3, 0.5, 16, 1)
	K, op = _operator(eng, D, "rbf", F64)
	K32, op32 = _operator(eng, Fr.case_data(1, "rbf", F32), "rbf", F32)
	Kb, opb = _operator(eng, Dm, "rbf", F64)  # another operator, for a cross object that is not this map's
	pre = DeviceOperator(K.preconditioned(8))
	fmap, fmap32 = eng.KernelFeatureMap(op, D["omega64"]), eng.KernelFeatureMap(op32, D["omega64"])
	cross, cross_b = eng.KernelCross(op, Dm["Xnew"]), eng.KernelCross(opb, Dm["Xnew"])
	Wm, Nm, Mm = DeviceMatrix(2 * f2, 4, ctx=op.ctx), DeviceMatrix(n, 4, ctx=op.ctx), DeviceMatrix(40, 4, ctx=op.ctx)
	other = Context(device=op.ctx.device)
	Wo = DeviceMatrix(2 * f2, 4, ctx=other)
	dense = DeviceOperator(np.eye(4))
	h = C.c_void_p()
	om = np.ascontiguousarray(D["omega64"])
	V = R.probes(n, 4, seed=5)
	before = op.matmat(V)

	def refused(rc, text):
		assert rc == _capi.SLQ_EINVAL and text in L.slq_last_error().decode(), (rc, L.slq_last_error())

	try:
		## create
		refused(L.slq_kernel_feature_create(op.ctx._h, dense._h, f2, _capi.ptr(om), d, C.byref(h)), "kind 'dense'")
		refused(L.slq_kernel_feature_create(op.ctx._h, pre._h, f2, _capi.ptr(om), d, C.byref(h)), "kind 'kernel_precond'")
		refused(L.slq_kernel_feature_create(other._h, op._h, f2, _capi.ptr(om), d, C.byref(h)), "another context")
		refused(L.slq_kernel_feature_create(op.ctx._h, op._h, 0, _capi.ptr(om), d, C.byref(h)), "F2 = 0")
		refused(L.slq_kernel_feature_create(op.ctx._h, op._h, f2, _capi.ptr(om), d - 1, C.byref(h)), "ld = 2")
		refused(L.slq_kernel_feature_create(op.ctx._h, op._h, f2, None, d, C.byref(h)), "NULL")
		refused(L.slq_kernel_feature_create(None, op._h, f2, _capi.ptr(om), d, C.byref(h)), "NULL")
		bad = om.copy()
		bad[4, 1] = np.nan
		refused(L.slq_kernel_feature_create(op.ctx._h, op._h, f2, _capi.ptr(bad), d, C.byref(h)), "frequency 4, coordinate 1 is not finite")
		with pytest.raises(ValueError, match="frequency 4, coordinate 1"):
			eng.KernelFeatureMap(op, bad)
		with pytest.raises(ValueError, match=r"\(F2, 3\) array"):
			eng.KernelFeatureMap(op, np.ones((4, 2)))
		with pytest.raises(ValueError, match="kind 'kernel_precond'"):
			eng.KernelFeatureMap(pre, om)
		assert not h.value
		## host products
		W = np.asfortranarray(D["W"])
		Y = np.zeros((40, b), order="F")
		refused(L.slq_kernel_feature_matmat(None, None, _capi.ptr(W), 2 * f2, _capi.ptr(Y), n, b), "feature map is NULL")
		refused(L.slq_kernel_feature_matmat(fmap._h, None, None, 2 * f2, _capi.ptr(Y), n, b), "NULL")
		refused(L.slq_kernel_feature_matmat(fmap._h, cross_b._h, _capi.ptr(W), 2 * f2, _capi.ptr(Y), 40, b), "another operator")
		refused(L.slq_kernel_feature_matmat(fmap._h, None, _capi.ptr(W), 2 * f2, _capi.ptr(Y), n, 0), "b = 0")
		refused(L.slq_kernel_feature_matmat(fmap._h, None, _capi.ptr(W), 2 * f2 - 1, _capi.ptr(Y), n, b), f"ldw = {2 * f2 - 1}")
		refused(L.slq_kernel_feature_matmat(fmap._h, None, _capi.ptr(W), 2 * f2, _capi.ptr(Y), n - 1, b), f"ldy = {n - 1}")
		refused(L.slq_kernel_feature_matmat(fmap._h, cross._h, _capi.ptr(W), 2 * f2, _capi.ptr(Y), 39, b), "ldy = 39")
		with pytest.raises(ValueError, match="dimension mismatch"):
			fmap.matmat(np.ones((f2, 2)))
		with pytest.raises(ValueError, match="KernelCross"):
			fmap.matmat(W, rows=op)
		## device matrices
		with pytest.raises(ValueError, match="fp32"):
			fmap32.matmat_dmat(Wm, 0, Nm, 0, 2)
		with pytest.raises(ValueError, match="another operator"):
			fmap.matmat_dmat(Wm, 0, Mm, 0, 2, rows=cross_b)
		with pytest.raises(ValueError, match=f"IN has {n} rows.*reads {2 * f2}"):
			fmap.matmat_dmat(Nm, 0, Nm, 2, 2)
		with pytest.raises(ValueError, match=f"OUT has 40 rows.*writes {n}"):
			fmap.matmat_dmat(Wm, 0, Mm, 0, 2)
		with pytest.raises(ValueError, match=f"OUT has {n} rows.*writes 40"):
			fmap.matmat_dmat(Wm, 0, Nm, 0, 2, rows=cross)
		with pytest.raises(ValueError, match=r"\(IN\): columns \[3, 5\)"):
			fmap.matmat_dmat(Wm, 3, Nm, 0, 2)
		with pytest.raises(ValueError, match=r"\(OUT\): columns \[-1, 1\)"):
			fmap.matmat_dmat(Wm, 0, Nm, -1, 2)
		with pytest.raises(ValueError, match="b = 0"):
			fmap.matmat_dmat(Wm, 0, Nm, 0, 0)
		with pytest.raises(ValueError, match="another context"):
			fmap.matmat_dmat(Wo, 0, Nm, 0, 2)
		with pytest.raises(ValueError, match="matrix is NULL"):
			_capi.check(L.slq_kernel_feature_dmat(fmap._h, None, None, 0, Nm._h, 0, 2))
		## nothing was written by any refused call, and the operator's own product is bitwise what it was
		assert not Mm.get().any() and not Nm.get().any() and not Y.any()
		assert np.array_equal(op.matmat(V), before)
		got = fmap.matmat(D["W"])
		assert Fr.worst(got, D["Y"], D["bar"]) <= 1.0
		assert np.array_equal(op.matmat(V), before)
	finally:
		for o in (Wm, Nm, Mm, Wo, cross, cross_b, fmap, fmap32, pre, op, op32, opb, dense, other):
			o.close()


def test_overlapping_columns_of_one_matrix_are_refused(eng):
	from primate_amd.operators import KernelOperator

	K = KernelOperator(R.points(20, 2, seed=3), "rbf", lengthscale=0.4)
	op = eng.DeviceOperator(K)
	fmap = K.features(10, seed=1).device(op)  # (2 F2 == n: one matrix can be both operands)
	Mx = eng.DeviceMatrix(20, 6, ctx=op.ctx)
	try:
		with pytest.raises(ValueError, match="overlap"):
			fmap.matmat_dmat(Mx, 0, Mx, 2, 3)
		Mx.set(0, R.probes(20, 3))
		fmap.matmat_dmat(Mx, 0, Mx, 3, 3)
		assert np.array_equal(Mx.get(3, 3), fmap.matmat(Mx.get(0, 3)))
	finally:
		Mx.close(), fmap.close(), op.close()


## ---- gp.sample_paths --------------------------------------------------------------------------------------------------------------------
def _gp_operator(G, name):
	from primate_amd.operators import KernelOperator

	return KernelOperator(G["X"], name, lengthscale=G["ls"], outputscale=Fr.S_GP, noise=G["noise"])


@pytest.mark.parametrize("rank", [0, 50], ids=["plain", "precond50"])
@pytest.mark.parametrize("name", ["rbf", "matern12"])
def test_paths_against_the_dense_pathwise_model(name, rank):
	"""evaluate(Xnew) within 1e-9 max |F| of the dense NumPy paths built from the same Omega, W and the eps read back (`posterior`'s bar)."""
	from primate_amd import gp

	G = Fr.gp_case(name)
	K = _gp_operator(G, name)
	Wh = np.random.default_rng(8).standard_normal((512, 8))
	with gp.sample_paths(K, G["y"], count=8, num_features=256, deg=100, precond_rank=rank, seed=3, weights=Wh) as paths:
		assert np.array_equal(paths.features.omega, Fr.frequencies(name, 256, 2, 3)) and np.array_equal(paths.weights, Wh)
		E = paths.noise_draws()
		assert E.shape == (Fr.N_GP, 8) and abs(E.std() - 1.0) < 0.1 and abs(E.mean()) < 0.1
		F = paths.evaluate(G["Xnew"])
		ref, _ = Fr.path_dense(G, paths.features.rounded(), Wh, E)
		err = float(np.max(np.abs(F - ref)) / np.max(np.abs(ref)))
		print(f"paths {name} rank {rank}: steps {paths.info['steps']}, within {err:.2e} of max |F|")
		assert F.shape == (Fr.M_GP, 8) and paths.info["deg"] == 100 and len(paths.info["steps"]) == 1
		assert paths.info["rank"] == (50 if rank else 0)
		assert err <= 1e-9
		## explicit noise draws give the same paths as the device draw they were read from
		with gp.sample_paths(K, G["y"], count=8, deg=100, precond_rank=rank, features=paths.features, weights=Wh, noise_draws=E) as again:
			assert np.array_equal(again.evaluate(G["Xnew"]), F)


def test_prior_paths_and_noise_free_paths():
	from primate_amd import engine, gp

	G = Fr.gp_case("matern32")
	K = _gp_operator(G, "matern32")
	with gp.sample_paths(K, None, count=5, num_features=100, seed=11) as prior:
		assert prior.noise_draws() is None and prior.info["steps"] == [] and prior.weights.shape == (200, 5)
		F = prior.evaluate(G["Xnew"])
		Y, bar = Fr.model(G["zs"], prior.features.rounded(), Fr.S_GP, prior.weights)  # Phi(X*) W alone
		assert Fr.worst(F, Y, bar) <= 1.0
		rng = np.random.default_rng(11)  # the defined order of the draws: the frequencies, then the weights
		assert np.array_equal(prior.features.omega, Fr.frequencies("matern32", 100, 2, 11))
		from primate_amd.operators import draw_kernel_frequencies

		draw_kernel_frequencies("matern32", 100, 2, rng)
		assert np.array_equal(prior.weights, rng.standard_normal((200, 5)))
	## noise = 0 on a well-conditioned case (matern12 at a short lengthscale: cond A = 23): no eps is drawn
	G0 = Fr.gp_case("matern12", noise=0.0, ls=0.02)
	K0 = _gp_operator(G0, "matern12")
	with gp.sample_paths(K0, G0["y"], count=4, num_features=64, deg=100, seed=2) as paths:
		assert paths.noise_draws() is None
		F = paths.evaluate(G0["Xnew"])
		ref, _ = Fr.path_dense(G0, paths.features.rounded(), paths.weights, None)
		err = float(np.max(np.abs(F - ref)) / np.max(np.abs(ref)))
		print(f"noise-free paths: within {err:.2e} of max |F|")
		assert err <= 1e-9
		assert np.max(np.abs(F[:5] - G0["y"][[3, 50, 120, 200, 299], None])) <= 1e-9 * np.max(np.abs(ref))  # (every path interpolates the data)
	assert isinstance(engine.default_context(), engine.Context)


@pytest.mark.parametrize("name", ["rbf", "matern52"])
def test_path_gradients_against_central_differences(name):
	"""dF against central differences (h = 1e-5) of the long-double path model at 5 new points, within 1e-6 max |dF|: truncation
	h^2 f''' and rounding eps / h are both ~1e-10 relative at these scales."""
	from primate_amd import gp

	G = Fr.gp_case(name)
	K = _gp_operator(G, name)
	Xq = np.array(G["Xnew"][5:10])
	h = 1e-5
	with gp.sample_paths(K, G["y"], count=3, num_features=128, deg=100, seed=6) as paths:
		F, dF = paths.evaluate(Xq, grad=True)
		assert F.shape == (5, 3) and dF.shape == (5, 2, 3)
		assert np.array_equal(F, paths.evaluate(Xq))
		om, Wh = paths.features.rounded(), paths.weights
		_, V = Fr.path_dense(G, om, Wh, paths.noise_draws())
		fd = np.zeros((5, 2, 3))
		for k in range(2):
			e = np.zeros(2)
			e[k] = h
			fd[:, k, :] = ((Fr.path_value_ld(G, name, om, Wh, V, Xq + e) - Fr.path_value_ld(G, name, om, Wh, V, Xq - e)) / (2 * Fr.LD(h))).astype(F64)
		err = float(np.max(np.abs(dF - fd)) / np.max(np.abs(fd)))
		print(f"path gradients {name}: within {err:.2e} of max |dF| = {np.max(np.abs(fd)):.3g}")
		assert err <= 1e-6
	with gp.sample_paths(K, None, count=3, num_features=128, seed=6) as prior:  # the feature term alone
		F, dF = prior.evaluate(Xq, grad=True)
		for k in range(2):
			e = np.zeros(2)
			e[k] = h
			fd[:, k, :] = ((Fr.path_value_ld(G, name, om, Wh, None, Xq + e) - Fr.path_value_ld(G, name, om, Wh, None, Xq - e)) / (2 * Fr.LD(h))).astype(F64)
		assert np.array_equal(prior.weights, Wh)
		assert np.max(np.abs(dF - fd)) <= 1e-6 * np.max(np.abs(fd))


@pytest.mark.parametrize("name", ["rbf", "matern12"])
def test_moments_with_the_default_draws(name):
	"""count = 512 paths with device-drawn eps: per new point the sample mean within 6 standard errors of the exact posterior mean
	C A^-1 y and the sample variance within 6 sqrt(2 / 511) relative of the model's variance given Omega (both bars derived; no
	random-feature bias enters either)."""
	from primate_amd import gp

	G = Fr.gp_case(name)
	K = _gp_operator(G, name)
	with gp.sample_paths(K, G["y"], count=512, num_features=1024, deg=60, seed=41) as paths:
		assert len(paths.info["steps"]) == 4  # (chunks of 128 columns)
		F = paths.evaluate(G["Xnew"])
		r_mean, r_var = Fr.moments_hold(F, G, paths.features.rounded())
		print(f"moments {name}: sample mean at {r_mean:.3f} of its 6-standard-error bar, sample variance at {r_var:.3f} of its bar")
		assert r_mean <= 1.0 and r_var <= 1.0
		E = paths.noise_draws()
		assert abs(np.corrcoef(E[:, 0], E[:, 200])[0, 1]) < 0.3 and not np.array_equal(E[:, :128], E[:, 128:256])  # (the chunks draw their own eps)


def test_paths_outlive_the_python_operator_and_refuse_changed_parameters():
	from primate_amd import gp

	G = Fr.gp_case("matern52")
	K = _gp_operator(G, "matern52")
	paths = gp.sample_paths(K, G["y"], count=2, num_features=32, deg=60, seed=1)
	want = paths.evaluate(G["Xnew"])
	del K
	gc.collect()
	assert np.array_equal(paths.evaluate(G["Xnew"]), want)  # (the paths keep the operator alive, as a plan does)
	paths.K.set_parameters(outputscale=2.0)
	with pytest.raises(ValueError, match="hyperparameters have changed"):
		paths.evaluate(G["Xnew"])
	paths.K.set_parameters(outputscale=Fr.S_GP)
	assert np.array_equal(paths.evaluate(G["Xnew"]), want)
	paths.close()
	with pytest.raises(ValueError, match="closed"):
		paths.evaluate(G["Xnew"])
