"""The adjoint feature product on the device (slq_kernelfeatureadj.hpp: k_kernel_feature_adjoint) against the
long-double model of tests/_kernelfeatureadj_ref.py, elementwise within its forward bound - each cell first asserts that the bound is a
small fraction of the result - the adjoint identity against the forward product, the bitwise properties, `KernelFeatureMap.gram`, and
`gp.feature_posterior` against the dense NumPy weight-space model built from the same frequencies.

The shapes are the forward table's six cells and a seventh of the adjoint's own (2000 points against 40 frequencies: one row block,
many slabs); the first six with the operator's own points as rows and with 1, 40 and 130 new points of a cross object. Each item prints
its worst ratio to the bar before it asserts (`-s`)."""

import numpy as np
import pytest

import _kernelfeature_ref as Fr
import _kernelfeatureadj_ref as Ar
import _kernelop_ref as R

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
LD = np.longdouble


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def _operator(eng, D, name, dtype, ls=None, s=Ar.S, noise=0.25):
	from primate_amd.operators import KernelOperator

	K = KernelOperator(D["X"], name, lengthscale=D["ls"] if ls is None else ls, outputscale=s, noise=noise, dtype=dtype)
	return K, eng.DeviceOperator(K)


def _device_points(op, n, d, dtype):
	"""(z^T, |z|^2, params) as the kernels read them (slq_debug_kernel_points)."""
	from primate_amd import _capi

	dpad, npad = (d + 3) // 4 * 4, (n + 15) // 16 * 16
	zt, nrm, par = np.empty((dpad, npad), dtype), np.empty(npad, dtype), np.empty(2, dtype)
	_capi.check(_capi.lib().slq_debug_kernel_points(op._h, _capi.ptr(zt), _capi.ptr(nrm), _capi.ptr(par)))
	return zt, nrm, par


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("idx", range(len(Ar.CASES)), ids=Ar.CASE_IDS)
def test_table_own_points_and_new_points_every_law(eng, idx, dtype):
	"""Z = Phi^T U through slq_kernel_feature_rmatmat within 1.0 bar of the model at the operator's points and at the new points of a
	cross object, after the device frequencies and points were found to be the rounded host ones bit for bit."""
	n, d, ls, f2, b = Ar.CASES[idx]
	for name in Ar.PROFILES:
		D = Ar.case_data(idx, name, dtype)
		K, op = _operator(eng, D, name, dtype)
		fmap = K.features(frequencies=D["omega64"]).device(op)
		crosses = []
		try:
			om = fmap.frequencies()
			assert np.array_equal(om, D["omega"]) and fmap.padding_is_zero and om.dtype == np.dtype(dtype)
			zt, _, par = _device_points(op, n, d, dtype)
			assert np.array_equal(zt[:d, :n].T, D["z"]) and not zt[d:].any() and not zt[:, n:].any() and par[0] == dtype(Ar.S)
			for m in Ar.rows_of(idx):
				Dm = Ar.case_data(idx, name, dtype, m)
				ratio = Ar.check_condition(Dm["Z"], Dm["bar"], name, dtype)
				rows = None
				if m is not None:
					rows = eng.KernelCross(op, Dm["Xnew"])
					crosses.append(rows)
					assert np.array_equal(rows.scaled_points()[0], Dm["z"]) and rows.padding_is_zero
				got = fmap.rmatmat(Dm["U"], rows=rows)
				assert got.shape == (2 * f2, b) and got.dtype == np.dtype(dtype) and np.all(np.isfinite(got))
				w = Ar.worst(got, Dm["Z"], Dm["bar"])
				print(f"{Ar.CASE_IDS[idx]} {name} rows {m or 'own'} {np.dtype(dtype).name}: {w:.3f} of the bar (bar / max |Z| {ratio:.1e})")
				assert w <= 1.0, (Ar.CASE_IDS[idx], name, m, w)
		finally:
			for o in (*crosses, fmap, op):
				o.close()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("idx", [2, 4], ids=[Ar.CASE_IDS[2], Ar.CASE_IDS[4]])
def test_adjoint_identity(eng, idx, dtype):
	"""<Phi W, U> against <W, Phi^T U>, both inner products in long double on the device results, within the sum of the two products'
	bars contracted with |U| and |W|."""
	n, d, ls, f2, b = Ar.CASES[idx]
	for name in Ar.PROFILES:
		Df, Da = Fr.case_data(idx, name, dtype), Ar.case_data(idx, name, dtype)
		K, op = _operator(eng, Da, name, dtype)
		fmap = eng.KernelFeatureMap(op, Da["omega64"])
		try:
			Y, Z = fmap.matmat(Df["W"]), fmap.rmatmat(Da["U"])
			W, U = Df["W"].astype(LD), Da["U"].astype(LD)
			lhs, rhs = np.sum(Y.astype(LD) * U, axis=0), np.sum(W * Z.astype(LD), axis=0)
			bar = np.sum(Df["bar"] * np.abs(U), axis=0) + np.sum(np.abs(W) * Da["bar"], axis=0)
			w = float(np.max(np.abs(lhs - rhs) / bar))
			print(f"adjoint identity {Ar.CASE_IDS[idx]} {name} {np.dtype(dtype).name}: {w:.3f} of the bar")
			assert w <= 1.0
		finally:
			fmap.close(), op.close()


@pytest.mark.parametrize("idx,m,slabs", [(4, 1, 1), (4, None, None), (6, None, None), (4, 130, None)], ids=["one_slab", "several_slabs", "many_slabs", "cross_rows"])
def test_identical_calls_give_identical_bits(eng, idx, m, slabs):
	n, d, ls, f2, b = Ar.CASES[idx]
	for dtype in (F64, F32):
		S = eng.kernel_feature_adjoint_schedule(f2, n if m is None else m, b, 256, dtype)
		assert S["slabs"] == 1 if slabs == 1 else S["slabs"] > 1, S
		D = Ar.case_data(idx, "matern12", dtype, m)
		K, op = _operator(eng, D, "matern12", dtype)
		fmap = eng.KernelFeatureMap(op, D["omega64"])
		rows = None if m is None else eng.KernelCross(op, D["Xnew"])
		try:
			first = fmap.rmatmat(D["U"], rows=rows)
			assert np.array_equal(first, fmap.rmatmat(D["U"], rows=rows))
			other = eng.KernelFeatureMap(op, D["omega64"])
			assert np.array_equal(first, other.rmatmat(D["U"], rows=rows))
			other.close()
		finally:
			if rows is not None:
				rows.close()
			fmap.close(), op.close()


@pytest.mark.parametrize("idx", [2, 3], ids=[Ar.CASE_IDS[2], Ar.CASE_IDS[3]])
def test_dmat_entry_equals_the_host_entry(eng, idx):
	n, d, ls, f2, b = Ar.CASES[idx]
	D, Dm = Ar.case_data(idx, "matern32", F64), Ar.case_data(idx, "matern32", F64, 40)
	K, op = _operator(eng, D, "matern32", F64)
	fmap = eng.KernelFeatureMap(op, D["omega64"])
	cross = eng.KernelCross(op, Dm["Xnew"])
	Nm, Mm, Zm = eng.DeviceMatrix(n, b + 3, ctx=op.ctx), eng.DeviceMatrix(40, b + 3, ctx=op.ctx), eng.DeviceMatrix(2 * f2, b + 2, ctx=op.ctx)
	try:
		Nm.set(3, D["U"]), Mm.set(3, Dm["U"])
		fmap.rmatmat_dmat(Nm, 3, Zm, 1, b)
		assert np.array_equal(Zm.get(1, b), fmap.rmatmat(D["U"]))
		assert not Zm.get(0, 1).any() and not Zm.get(b + 1, 1).any()  # (nothing outside the range)
		fmap.rmatmat_dmat(Mm, 3, Zm, 1, b, rows=cross)
		assert np.array_equal(Zm.get(1, b), fmap.rmatmat(Dm["U"], rows=cross))
		assert not Zm.get(0, 1).any() and not Zm.get(b + 1, 1).any()
	finally:
		for o in (Nm, Mm, Zm, cross, fmap, op):
			o.close()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_set_parameters_equals_a_fresh_pair(eng, dtype):
	idx = 1  # (17, 3, ., 16, 1): per-dimension lengthscales
	D, Dm = Ar.case_data(idx, "matern52", dtype), Ar.case_data(idx, "matern52", dtype, 40)
	new_ls, new_s = np.array([0.35, 0.6, 0.45]), 0.9
	K, op = _operator(eng, D, "matern52", dtype, ls=0.7, s=2.0)
	fmap, cross = eng.KernelFeatureMap(op, D["omega64"]), eng.KernelCross(op, Dm["Xnew"])
	K2, op2 = _operator(eng, D, "matern52", dtype, ls=new_ls, s=new_s)
	fresh, cross2 = eng.KernelFeatureMap(op2, D["omega64"]), eng.KernelCross(op2, Dm["Xnew"])
	U, Um = R.probes(17, 7, seed=3, dtype=dtype), R.probes(40, 7, seed=4, dtype=dtype)
	try:
		before, before_m = fmap.rmatmat(U), fmap.rmatmat(Um, rows=cross)
		K.set_parameters(lengthscale=new_ls, outputscale=new_s)  # (KernelOperator.set_parameters: no code for the feature map)
		got, got_m = fmap.rmatmat(U), fmap.rmatmat(Um, rows=cross)
		assert not np.array_equal(before, got) and not np.array_equal(before_m, got_m)
		assert np.array_equal(got, fresh.rmatmat(U)) and np.array_equal(got_m, fresh.rmatmat(Um, rows=cross2))
		Z, bar = Ar.model(R.scaled_points(D["X"], new_ls, dtype), D["omega"], new_s, U)
		assert Ar.worst(got, Z, bar) <= 1.0
		K.set_parameters(noise=7.0)
		assert np.array_equal(fmap.rmatmat(U), got)  # (no noise term)
	finally:
		for o in (cross, cross2, fmap, fresh, op, op2):
			o.close()


def test_every_device_refusal_and_the_products_are_untouched(eng):
	from primate_amd import _capi
	from primate_amd.engine import Context, DeviceMatrix

	L = _capi.lib()
	D, Dm = Ar.case_data(1, "rbf", F64), Ar.case_data(1, "rbf", F64, 40)
	n, d, ls, f2, b = Ar.CASES[1]  # (17, 3, 0.5, 16, 1)
	K, op = _operator(eng, D, "rbf", F64)
	K32, op32 = _operator(eng, Ar.case_data(1, "rbf", F32), "rbf", F32)
	Kb, opb = _operator(eng, Dm, "rbf", F64)  # another operator, for a cross object that is not this map's
	fmap, fmap32 = eng.KernelFeatureMap(op, D["omega64"]), eng.KernelFeatureMap(op32, D["omega64"])
	cross, cross_b = eng.KernelCross(op, Dm["Xnew"]), eng.KernelCross(opb, Dm["Xnew"])
	Zm, Nm, Mm = DeviceMatrix(2 * f2, 4, ctx=op.ctx), DeviceMatrix(n, 4, ctx=op.ctx), DeviceMatrix(40, 4, ctx=op.ctx)
	other = Context(device=op.ctx.device)
	No = DeviceMatrix(n, 4, ctx=other)
	V = R.probes(n, 4, seed=5)
	Wf = Fr.case_data(1, "rbf", F64)["W"]
	before, before_f = op.matmat(V), fmap.matmat(Wf)

	def refused(rc, text):
		assert rc == _capi.SLQ_EINVAL and text in L.slq_last_error().decode(), (rc, L.slq_last_error())

	try:
		## host products
		U = np.asfortranarray(D["U"])
		Z = np.zeros((2 * f2, b), order="F")
		refused(L.slq_kernel_feature_rmatmat(None, None, _capi.ptr(U), n, _capi.ptr(Z), 2 * f2, b), "feature map is NULL")
		refused(L.slq_kernel_feature_rmatmat(fmap._h, None, None, n, _capi.ptr(Z), 2 * f2, b), "NULL")
		refused(L.slq_kernel_feature_rmatmat(fmap._h, None, _capi.ptr(U), n, None, 2 * f2, b), "NULL")
		refused(L.slq_kernel_feature_rmatmat(fmap._h, cross_b._h, _capi.ptr(U), 40, _capi.ptr(Z), 2 * f2, b), "another operator")
		refused(L.slq_kernel_feature_rmatmat(fmap._h, None, _capi.ptr(U), n, _capi.ptr(Z), 2 * f2, 0), "b = 0")
		refused(L.slq_kernel_feature_rmatmat(fmap._h, None, _capi.ptr(U), n - 1, _capi.ptr(Z), 2 * f2, b), f"ldu = {n - 1}")
		refused(L.slq_kernel_feature_rmatmat(fmap._h, cross._h, _capi.ptr(U), 39, _capi.ptr(Z), 2 * f2, b), "ldu = 39")
		refused(L.slq_kernel_feature_rmatmat(fmap._h, None, _capi.ptr(U), n, _capi.ptr(Z), 2 * f2 - 1, b), f"ldz = {2 * f2 - 1}")
		with pytest.raises(ValueError, match="dimension mismatch"):
			fmap.rmatmat(np.ones((n + 1, 2)))
		with pytest.raises(ValueError, match="dimension mismatch"):
			fmap.rmatmat(np.ones((n, 2)), rows=cross)
		with pytest.raises(ValueError, match="KernelCross"):
			fmap.rmatmat(U, rows=op)
		## device matrices
		with pytest.raises(ValueError, match="fp32"):
			fmap32.rmatmat_dmat(Nm, 0, Zm, 0, 2)
		with pytest.raises(ValueError, match="another operator"):
			fmap.rmatmat_dmat(Mm, 0, Zm, 0, 2, rows=cross_b)
		with pytest.raises(ValueError, match=f"IN has {2 * f2} rows.*reads {n}"):
			fmap.rmatmat_dmat(Zm, 0, Zm, 2, 2)
		with pytest.raises(ValueError, match=f"IN has {n} rows.*reads 40"):
			fmap.rmatmat_dmat(Nm, 0, Zm, 0, 2, rows=cross)
		with pytest.raises(ValueError, match=f"OUT has {n} rows.*writes {2 * f2}"):
			fmap.rmatmat_dmat(Nm, 0, Nm, 2, 2)
		with pytest.raises(ValueError, match=r"\(IN\): columns \[3, 5\)"):
			fmap.rmatmat_dmat(Nm, 3, Zm, 0, 2)
		with pytest.raises(ValueError, match=r"\(OUT\): columns \[-1, 1\)"):
			fmap.rmatmat_dmat(Nm, 0, Zm, -1, 2)
		with pytest.raises(ValueError, match="b = 0"):
			fmap.rmatmat_dmat(Nm, 0, Zm, 0, 0)
		with pytest.raises(ValueError, match="another context"):
			fmap.rmatmat_dmat(No, 0, Zm, 0, 2)
		with pytest.raises(ValueError, match="matrix is NULL"):
			_capi.check(L.slq_kernel_feature_rdmat(fmap._h, None, None, 0, Zm._h, 0, 2))
		with pytest.raises(ValueError, match="feature map is NULL"):
			_capi.check(L.slq_kernel_feature_rdmat(None, None, Nm._h, 0, Zm._h, 0, 2))
		with pytest.raises(ValueError, match="fp64 only"):
			fmap32.gram()
		## nothing was written by any refused call; the operator's product and the forward feature product are bitwise what they were
		assert not Zm.get().any() and not Nm.get().any() and not Mm.get().any() and not Z.any()
		assert np.array_equal(op.matmat(V), before) and np.array_equal(fmap.matmat(Wf), before_f)
		got = fmap.rmatmat(D["U"])
		assert Ar.worst(got, D["Z"], D["bar"]) <= 1.0
		assert np.array_equal(op.matmat(V), before) and np.array_equal(fmap.matmat(Wf), before_f)
	finally:
		for o in (Zm, Nm, Mm, No, cross, cross_b, fmap, fmap32, op, op32, opb, other):
			o.close()


def test_overlapping_columns_of_one_matrix_are_refused(eng):
	from primate_amd.operators import KernelOperator

	K = KernelOperator(R.points(20, 2, seed=3), "rbf", lengthscale=0.4)
	op = eng.DeviceOperator(K)
	fmap = K.features(10, seed=1).device(op)  # (2 F2 == n: one matrix can be both operands)
	Mx = eng.DeviceMatrix(20, 6, ctx=op.ctx)
	try:
		with pytest.raises(ValueError, match="overlap"):
			fmap.rmatmat_dmat(Mx, 0, Mx, 2, 3)
		Mx.set(0, R.probes(20, 3))
		fmap.rmatmat_dmat(Mx, 0, Mx, 3, 3)
		assert np.array_equal(Mx.get(3, 3), fmap.rmatmat(Mx.get(0, 3)))
	finally:
		Mx.close(), fmap.close(), op.close()


def test_gram_within_the_propagated_bar(eng):
	"""Phi^T Phi on the operator of cell (300, 8, 1.0, 1024, 16) with F2 = 100: within the Gram model's propagated bar, the asymmetry
	reported, and G[j, j] + G[F2 + j, F2 + j] = a^2 n to 1e-12 relative (cos^2 + sin^2 = 1)."""
	idx, f2 = 4, 100
	n = Ar.CASES[idx][0]
	D = Ar.case_data(idx, "matern32", F64)
	K, op = _operator(eng, D, "matern32", F64)
	om64 = Fr.frequencies("matern32", f2, Ar.CASES[idx][1], 9)
	fmap = eng.KernelFeatureMap(op, om64)
	try:
		G = fmap.gram(chunk=64)  # (200 columns: three full chunks and a remainder)
		ref, bar = Ar.gram_model(D["z"], om64.astype(F64), Ar.S)
		bar = 0.5 * (bar + bar.T)  # (the symmetrised result: each element is the mean of two within their bars)
		w = Ar.worst(G, 0.5 * (ref + ref.T), bar)
		print(f"gram: {w:.3f} of the propagated bar (bar / max |G| {float(np.max(bar) / np.max(np.abs(ref))):.1e}), asymmetry {fmap.gram_asymmetry:.2e}")
		assert G.shape == (2 * f2, 2 * f2) and G.dtype == F64 and np.array_equal(G, G.T)
		assert w <= 1.0
		assert 0.0 <= fmap.gram_asymmetry <= 2.0 * float(np.max(bar))
		pair = np.diag(G)[:f2] + np.diag(G)[f2:]
		a2n = Ar.S / f2 * n
		e = float(np.max(np.abs(pair / a2n - 1.0)))
		print(f"gram: G[j, j] + G[F2 + j, F2 + j] within {e:.1e} of a^2 n")
		assert e <= 1e-12
		assert np.array_equal(G, fmap.gram(chunk=64)) and np.max(np.abs(G - fmap.gram())) <= 2.0 * float(np.max(bar))
	finally:
		fmap.close(), op.close()


## ---- gp.feature_posterior -----------------------------------------------------------------------------------------------------------------
def _gp_operator(G, name, noise=None, dtype=F64):
	from primate_amd.operators import KernelOperator

	return KernelOperator(G["X"].astype(dtype), name, lengthscale=G["ls"], outputscale=Fr.S_GP, noise=G["noise"] if noise is None else noise, dtype=dtype)


@pytest.mark.parametrize("name", ["rbf", "matern12"])
def test_feature_posterior_against_the_dense_weight_space_model(name):
	"""mean_weights, the predictive mean and variance (with and without the noise) and the mll at 1e-9 of their maxima against the dense
	NumPy model from the same frequencies; the sample functions against Phi* (w_bar 1^T + sqrt(sigma2) L^-T Xi) at the same bar."""
	from primate_amd import gp

	G = Fr.gp_case(name)
	K = _gp_operator(G, name)
	Ft = K.features(frequencies=Fr.frequencies(name, Ar.F2_GP, 2, Ar.FREQ_SEED_GP))
	M = Ar.weight_space_dense(G, Ft.rounded())
	m2 = 2 * Ar.F2_GP
	with gp.feature_posterior(K, G["y"], features=Ft) as post:
		assert post.features is Ft and post.info["num_features"] == Ar.F2_GP and post.mean_weights.shape == (m2,)
		assert 0.0 <= post.info["gram_asymmetry"] < 1e-10 and G["noise"] < post.info["m_diag_min"] <= post.info["m_diag_max"]
		rel = lambda got, ref: float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))  # noqa: E731
		mean, var = post.predict(G["Xnew"])
		_, var_n = post.predict(G["Xnew"], include_noise=True)
		mean_only, none = post.predict(G["Xnew"], variance=False)
		e = dict(weights=rel(post.mean_weights, M["wbar"]), mean=rel(mean, M["mean"]), var=rel(var, M["var"]), var_noise=rel(var_n, M["var"] + G["noise"]),
				 mll=abs(post.mll / M["mll"] - 1.0))  # fmt: skip
		print(f"feature_posterior {name}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()) + f"; mll = {post.mll:.4f}")
		assert none is None and np.array_equal(mean_only, mean)
		assert max(e.values()) <= 1e-9, e
		## the feature model against the exact GP: a property of the method, printed and not asserted
		print(f"feature_posterior {name}: mean at {rel(mean, G['mean']):.2f} of max |mean| from the exact posterior mean at F2 = {Ar.F2_GP}")
		## sample functions
		Xi = np.random.default_rng(8).standard_normal((m2, 8))
		Wref = M["wbar"][:, None] + np.sqrt(G["noise"]) * np.linalg.solve(M["L"].T, Xi)
		with post.sample_paths(count=8, normals=Xi) as paths:
			F = paths.evaluate(G["Xnew"])
			e_w, e_f = rel(paths.weights, Wref), rel(F, M["Ps"] @ Wref)
			print(f"feature_posterior {name}: sample weights {e_w:.1e}, sample functions {e_f:.1e}")
			assert F.shape == (Fr.M_GP, 8) and paths.noise_draws() is None and e_w <= 1e-9 and e_f <= 1e-9
		with post.sample_paths(count=3, seed=4) as drawn:  # the defined draw
			Wd = M["wbar"][:, None] + np.sqrt(G["noise"]) * np.linalg.solve(M["L"].T, np.random.default_rng(4).standard_normal((m2, 3)))
			assert rel(drawn.weights, Wd) <= 1e-9
		## the draw of the frequencies is that of sample_paths
	with gp.feature_posterior(K, G["y"], num_features=32, seed=3) as drawn:
		assert np.array_equal(drawn.features.omega, Fr.frequencies(name, 32, 2, 3))


def test_feature_path_gradients_against_central_differences():
	"""dF of the weight-space sample functions against central differences (h = 1e-5) of the long-double model at 5 new points, within
	1e-6 max |dF|, as the pathwise test does."""
	from primate_amd import gp

	G = Fr.gp_case("rbf")
	K = _gp_operator(G, "rbf")
	Xq = np.array(G["Xnew"][5:10])
	h = 1e-5
	with gp.feature_posterior(K, G["y"], num_features=128, seed=6) as post, post.sample_paths(count=3, seed=7) as paths:
		F, dF = paths.evaluate(Xq, grad=True)
		assert F.shape == (5, 3) and dF.shape == (5, 2, 3) and np.array_equal(F, paths.evaluate(Xq))
		om, Wh = paths.features.rounded(), paths.weights
		fd = np.zeros((5, 2, 3))
		for k in range(2):
			e = np.zeros(2)
			e[k] = h
			fd[:, k, :] = ((Ar.path_value_ld(G, om, Wh, Xq + e) - Ar.path_value_ld(G, om, Wh, Xq - e)) / (2 * LD(h))).astype(F64)
		err = float(np.max(np.abs(dF - fd)) / np.max(np.abs(fd)))
		print(f"feature path gradients: within {err:.2e} of max |dF| = {np.max(np.abs(fd)):.3g}")
		assert err <= 1e-6


def test_feature_posterior_refusals_and_changed_parameters():
	from primate_amd import gp

	G = Fr.gp_case("rbf")
	K = _gp_operator(G, "rbf")
	with pytest.raises(ValueError, match="noise > 0.*singular when 2 F2 > n"):
		gp.feature_posterior(_gp_operator(G, "rbf", noise=0.0), G["y"], num_features=16)
	with pytest.raises(ValueError, match="fp64 only"):
		gp.feature_posterior(_gp_operator(G, "rbf", dtype=F32), G["y"], num_features=16)
	with pytest.raises(ValueError, match="exceed the limit of 8192"):
		gp.feature_posterior(K, G["y"], num_features=4097)
	post = gp.feature_posterior(K, G["y"], num_features=16, seed=1)
	mean, var = post.predict(G["Xnew"])
	K.set_parameters(outputscale=2.0)
	with pytest.raises(ValueError, match="predict: .*hyperparameters have changed"):
		post.predict(G["Xnew"])
	with pytest.raises(ValueError, match="sample_paths: .*hyperparameters have changed"):
		post.sample_paths(2)
	K.set_parameters(outputscale=Fr.S_GP)
	again, _ = post.predict(G["Xnew"])
	assert np.array_equal(again, mean)
	paths = post.sample_paths(2, seed=1)
	K.set_parameters(lengthscale=0.7)
	with pytest.raises(ValueError, match="hyperparameters have changed"):
		paths.evaluate(G["Xnew"])
	paths.close(), post.close()
	with pytest.raises(ValueError, match="closed"):
		post.predict(G["Xnew"])
