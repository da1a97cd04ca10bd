"""Cross-covariance products of the kernel operator on the device (slq_kernelcross.hpp: k_kernel_cross,
k_kernel_cross_sum) against the long-double model of tests/_kernelcross_ref.py, elementwise within its forward bound - each cell
first asserts that the bound is a small fraction of the result - and `gp.posterior` against a dense float64 solve.

The shapes are the issue's table: the smallest shape, partial tiles on both sides, a second row block of one row with a remainder
tile, several slabs with both sides of a 64-column edge, the deep-coordinate instantiation, a second 256-column chunk, and new
points equal to training points, plain and moved by 1e4. Each item prints its worst ratio to the bar before it asserts (`-s`)."""

import ctypes as C
import gc

import numpy as np
import pytest

import _kernelcross_ref as X
import _kernelop_ref as R

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
PERDIM = np.array([0.5, 0.3, 0.8])


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def _operator(eng, D, name, dtype, ls=None, s=X.S, noise=0.25):
	from primate_amd.operators import KernelOperator

	K = KernelOperator(D["X"], name, lengthscale=D["ls"] if ls is None else ls, outputscale=s, noise=noise, dtype=dtype)
	return K, eng.DeviceOperator(K)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("idx", range(len(X.CASES)), ids=X.CASE_IDS)
def test_table_both_directions_every_profile(eng, idx, dtype):
	"""Y = C W and Y = C^T U through slq_kernel_cross_matmat within 1.0 bar of the model, after the device z* were found to be the
	model's bit for bit with zeros in the padding."""
	m, n, d, b, variant = X.CASES[idx]
	for name in X.PROFILES:
		Df, Da = X.case_data(idx, name, dtype, False), X.case_data(idx, name, dtype, True)
		rf = X.check_condition(Df["Y"], Df["bar"], name, variant, dtype)
		ra = X.check_condition(Da["Y"], Da["bar"], name, variant, dtype)
		K, op = _operator(eng, Df, name, dtype)
		cross = eng.KernelCross(op, Df["Xnew"])
		try:
			assert cross.shape == (m, n) and cross.dtype == np.dtype(dtype)
			zs, nrm = cross.scaled_points()
			assert np.array_equal(zs, Df["zs"]) and cross.padding_is_zero and zs.dtype == np.dtype(dtype)
			assert np.allclose(nrm, np.sum(Df["zs"].astype(F64) ** 2, axis=1), rtol=(d + 2) * 2 * R.eps_of(dtype), atol=0)
			got_f = cross.matmat(Df["W"])
			got_a = cross.matmat(Da["W"], trans=True)
			assert got_f.shape == (m, b) and got_a.shape == (n, b) and got_f.dtype == np.dtype(dtype)
			wf, wa = X.worst(got_f, Df["Y"], Df["bar"]), X.worst(got_a, Da["Y"], Da["bar"])
			print(f"{X.CASE_IDS[idx]} {name} {np.dtype(dtype).name}: forward {wf:.3f} adjoint {wa:.3f} of the bar (bar / max |Y| {rf:.1e}, {ra:.1e})")
			assert np.all(np.isfinite(got_f)) and np.all(np.isfinite(got_a))
			assert wf <= 1.0 and wa <= 1.0, (X.CASE_IDS[idx], name, wf, wa)
		finally:
			cross.close()
			op.close()


def test_new_points_as_a_torch_tensor(eng):
	import torch

	for dtype in (F64, F32):
		D = X.case_data(2, "rbf", dtype, False)
		K, op = _operator(eng, D, "rbf", dtype)
		Xt = torch.as_tensor(np.array(D["Xnew"]), device=f"cuda:{op.ctx.device}")
		cross, host = eng.KernelCross(op, Xt), eng.KernelCross(op, D["Xnew"])
		try:
			zs, _ = cross.scaled_points()
			assert np.array_equal(zs, D["zs"]) and cross.padding_is_zero
			assert np.array_equal(cross.matmat(D["W"]), host.matmat(D["W"]))
			## and through the host operator object
			from primate_amd.operators import KernelCrossOperator

			dev = KernelCrossOperator(K, Xt).device(op)
			assert np.array_equal(dev.scaled_points()[0], D["zs"])
			dev.close()
		finally:
			cross.close(), host.close(), op.close()


@pytest.mark.parametrize("idx,trans,slabs", [(1, True, 1), (3, False, None), (5, False, None)], ids=["one_slab", "several_slabs", "two_chunks"])
def test_identical_calls_give_identical_bits(eng, idx, trans, slabs):
	m, n, d, b, _ = X.CASES[idx]
	S = eng.kernel_cross_schedule(n if trans else m, m if trans else n, b, 256)
	assert S["slabs"] == 1 if slabs == 1 else S["slabs"] > 1, S
	for dtype in (F64, F32):
		D = X.case_data(idx, "matern52", dtype, trans)
		K, op = _operator(eng, D, "matern52", dtype)
		cross = eng.KernelCross(op, D["Xnew"])
		try:
			first = cross.matmat(D["W"], trans=trans)
			assert np.array_equal(first, cross.matmat(D["W"], trans=trans))
			other = eng.KernelCross(op, D["Xnew"])
			assert np.array_equal(first, other.matmat(D["W"], trans=trans))
			other.close()
		finally:
			cross.close(), op.close()


@pytest.mark.parametrize("idx", [2, 3], ids=[X.CASE_IDS[2], X.CASE_IDS[3]])
def test_dmat_entry_equals_the_host_entry(eng, idx):
	m, n, d, b, _ = X.CASES[idx]
	Df, Da = X.case_data(idx, "matern32", F64, False), X.case_data(idx, "matern32", F64, True)
	K, op = _operator(eng, Df, "matern32", F64)
	cross = eng.KernelCross(op, Df["Xnew"])
	Nm, Mm = eng.DeviceMatrix(n, b + 3, ctx=op.ctx), eng.DeviceMatrix(m, b + 2, ctx=op.ctx)
	try:
		Nm.set(3, Df["W"])
		cross.matmat_dmat(Nm, 3, Mm, 1, b)
		assert np.array_equal(Mm.get(1, b), cross.matmat(Df["W"]))
		assert not Mm.get(0, 1).any() and not Mm.get(b + 1, 1).any()  # (nothing outside the range)
		Mm.set(2, Da["W"])
		cross.matmat_dmat(Mm, 2, Nm, 0, b, trans=True)
		assert np.array_equal(Nm.get(0, b), cross.matmat(Da["W"], trans=True))
	finally:
		Nm.close(), Mm.close(), cross.close(), op.close()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_set_parameters_equals_a_fresh_pair(eng, dtype):
	idx = 2
	Df, Da = X.case_data(idx, "matern52", dtype, False), X.case_data(idx, "matern52", dtype, True)
	new_ls, new_s = np.array([0.35, 0.6, 0.45]), 0.9
	K, op = _operator(eng, Df, "matern52", dtype, ls=0.7, s=2.0)
	cross = eng.KernelCross(op, Df["Xnew"])
	K2, op2 = _operator(eng, Df, "matern52", dtype, ls=new_ls, s=new_s)
	fresh = eng.KernelCross(op2, Df["Xnew"])
	try:
		before = cross.matmat(Df["W"])
		K.set_parameters(lengthscale=new_ls, outputscale=new_s)  # (KernelOperator.set_parameters: no code for the cross object)
		got_f, got_a = cross.matmat(Df["W"]), cross.matmat(Da["W"], trans=True)
		assert not np.array_equal(before, got_f)
		assert np.array_equal(got_f, fresh.matmat(Df["W"])) and np.array_equal(got_a, fresh.matmat(Da["W"], trans=True))
		assert np.array_equal(cross.scaled_points()[0], X.scaled_new_points(Df["X"], Df["Xnew"], new_ls, dtype))
		## the operator's own words are its own: the fresh operator's product equals the changed one's
		assert np.array_equal(op.matmat(Df["W"]), op2.matmat(Df["W"]))
	finally:
		cross.close(), fresh.close(), op.close(), op2.close()


def test_the_operator_is_untouched_by_a_cross_object(eng):
	D = X.case_data(3, "rbf", F64, False)
	m, n, d, b, _ = X.CASES[3]
	K, op = _operator(eng, D, "rbf", F64)
	V = R.probes(n, 16, seed=5)

	def snapshot():
		plan = eng.LanczosPlan(op, 16, 12, 3)
		plan.set_probes(V)
		plan.run()
		q = plan.quadrature("log")
		plan.close()
		zt = np.empty(((d + 3) // 4 * 4, (n + 15) // 16 * 16))
		nrm, par = np.empty(zt.shape[1]), np.empty(2)
		from primate_amd import _capi

		_capi.check(_capi.lib().slq_debug_kernel_points(op._h, _capi.ptr(zt), _capi.ptr(nrm), _capi.ptr(par)))
		return op.matmat(V), q, zt, nrm, par

	try:
		before = snapshot()
		cross = eng.KernelCross(op, D["Xnew"])
		cross.matmat(D["W"])
		cross.matmat(R.probes(m, 4), trans=True)
		cross.scaled_points()
		cross.close()
		for a, c in zip(before, snapshot()):
			assert np.array_equal(a, c)
	finally:
		op.close()


def test_every_device_refusal(eng):
	from primate_amd import _capi
	from primate_amd.engine import Context, DeviceMatrix, DeviceOperator

	L = _capi.lib()
	D = X.case_data(1, "rbf", F64, False)
	m, n, d, b, _ = X.CASES[1]
	K, op = _operator(eng, D, "rbf", F64)
	K32, op32 = _operator(eng, X.case_data(1, "rbf", F32, False), "rbf", F32)
	cross, cross32 = eng.KernelCross(op, D["Xnew"]), eng.KernelCross(op32, D["Xnew"])
	Nm, Mm = DeviceMatrix(n, 4, ctx=op.ctx), DeviceMatrix(m, 4, ctx=op.ctx)
	other = Context(device=op.ctx.device)
	No = DeviceMatrix(n, 4, ctx=other)
	dense = DeviceOperator(np.eye(4))
	h = C.c_void_p()
	pts = np.ascontiguousarray(D["Xnew"], dtype=F64)

	def refused(rc, text):
		assert rc == _capi.SLQ_EINVAL and text in L.slq_last_error().decode(), (rc, L.slq_last_error())

	try:
		## create
		refused(L.slq_kernel_cross_create(op.ctx._h, dense._h, m, _capi.ptr(pts), d, C.byref(h)), "kind 'dense'")
		refused(L.slq_kernel_cross_create(other._h, op._h, m, _capi.ptr(pts), d, C.byref(h)), "another context")
		refused(L.slq_kernel_cross_create(op.ctx._h, op._h, 0, _capi.ptr(pts), d, C.byref(h)), "m = 0")
		refused(L.slq_kernel_cross_create(op.ctx._h, op._h, m, _capi.ptr(pts), d - 1, C.byref(h)), "ldp = 2")
		refused(L.slq_kernel_cross_create(op.ctx._h, op._h, m, None, d, C.byref(h)), "NULL")
		bad = pts.copy()
		bad[4, 1] = np.inf
		refused(L.slq_kernel_cross_create(op.ctx._h, op._h, m, _capi.ptr(bad), d, C.byref(h)), "new point 4, coordinate 1 is inf")
		with pytest.raises(ValueError, match="new point 4, coordinate 1"):
			eng.KernelCross(op, bad)
		import torch

		with pytest.raises(ValueError, match="new point 4, coordinate 1"):
			eng.KernelCross(op, torch.as_tensor(bad, device=f"cuda:{op.ctx.device}"))
		with pytest.raises(ValueError, match=r"\(m, 3\) array"):
			eng.KernelCross(op, np.ones((4, 2)))
		assert not h.value
		## host products
		W = np.asfortranarray(D["W"])
		Y = np.zeros((n, b), order="F")
		refused(L.slq_kernel_cross_matmat(cross._h, 2, _capi.ptr(W), n, _capi.ptr(Y), m, b), "trans = 2")
		refused(L.slq_kernel_cross_matmat(cross._h, 0, _capi.ptr(W), n, _capi.ptr(Y), m, 0), "b = 0")
		refused(L.slq_kernel_cross_matmat(cross._h, 0, _capi.ptr(W), n - 1, _capi.ptr(Y), m, b), f"ldx = {n - 1}")
		refused(L.slq_kernel_cross_matmat(cross._h, 0, _capi.ptr(W), n, _capi.ptr(Y), m - 1, b), f"ldy = {m - 1}")
		refused(L.slq_kernel_cross_matmat(cross._h, 1, _capi.ptr(W), m, _capi.ptr(Y), n - 1, b), f"ldy = {n - 1}")
		refused(L.slq_kernel_cross_matmat(cross._h, 0, None, n, _capi.ptr(Y), m, b), "NULL")
		with pytest.raises(ValueError, match="dimension mismatch"):
			cross.matmat(np.ones((m, 2)))
		with pytest.raises(ValueError, match="dimension mismatch"):
			cross.matmat(np.ones((n, 2)), trans=True)
		## device matrices
		with pytest.raises(ValueError, match="fp32"):
			cross32.matmat_dmat(Nm, 0, Mm, 0, 2)
		with pytest.raises(ValueError, match=f"IN has {m} rows.*reads {n}"):
			cross.matmat_dmat(Mm, 0, Mm, 2, 2)
		with pytest.raises(ValueError, match=f"OUT has {n} rows.*writes {m}"):
			cross.matmat_dmat(Nm, 0, Nm, 2, 2)
		with pytest.raises(ValueError, match=f"IN has {n} rows.*reads {m}"):
			cross.matmat_dmat(Nm, 0, Nm, 2, 2, trans=True)
		with pytest.raises(ValueError, match=r"\(IN\): columns \[3, 5\)"):
			cross.matmat_dmat(Nm, 3, Mm, 0, 2)
		with pytest.raises(ValueError, match=r"\(OUT\): columns \[-1, 1\)"):
			cross.matmat_dmat(Nm, 0, Mm, -1, 2)
		with pytest.raises(ValueError, match="b = 0"):
			cross.matmat_dmat(Nm, 0, Mm, 0, 0)
		with pytest.raises(ValueError, match="trans = 3"):
			_capi.check(L.slq_kernel_cross_dmat(cross._h, 3, Nm._h, 0, Mm._h, 0, 2))
		with pytest.raises(ValueError, match="another context"):
			cross.matmat_dmat(No, 0, Mm, 0, 2)
		with pytest.raises(ValueError, match="matrix is NULL"):
			_capi.check(L.slq_kernel_cross_dmat(cross._h, 0, None, 0, Mm._h, 0, 2))
		## nothing was written by any refused call
		assert not Mm.get().any() and not Nm.get().any()
	finally:
		for o in (Nm, Mm, No, cross, cross32, op, op32, dense, other):
			o.close()


def test_overlapping_columns_of_one_matrix_are_refused(eng):
	from primate_amd.operators import KernelOperator

	Xt = R.points(20, 2, seed=3)
	K = KernelOperator(Xt, "rbf", lengthscale=0.4)
	op = eng.DeviceOperator(K)
	cross = eng.KernelCross(op, R.points(20, 2, seed=4))  # (m == n: one matrix can be both operands)
	Mx = eng.DeviceMatrix(20, 6, ctx=op.ctx)
	try:
		with pytest.raises(ValueError, match="overlap"):
			cross.matmat_dmat(Mx, 0, Mx, 2, 3)
		Mx.set(0, R.probes(20, 3))
		cross.matmat_dmat(Mx, 0, Mx, 3, 3)
		assert np.array_equal(Mx.get(3, 3), cross.matmat(Mx.get(0, 3)))
	finally:
		Mx.close(), cross.close(), op.close()


def test_the_python_operator_may_go_while_the_cross_object_lives(eng):
	D = X.case_data(1, "matern12", F64, False)
	K, op = _operator(eng, D, "matern12", F64)
	cross = eng.KernelCross(op, D["Xnew"])
	want = cross.matmat(D["W"])
	del op, K
	gc.collect()
	assert np.array_equal(cross.matmat(D["W"]), want)  # (the cross object keeps the device operator alive, as a plan does)
	assert X.worst(want, D["Y"], D["bar"]) <= 1.0
	cross.close()


## ---- gp.posterior -----------------------------------------------------------------------------------------------------------------------
N_GP, M_GP, S_GP, NOISE_GP, LS_GP = 300, 40, 1.5, 0.1, 0.4
_gp_cache = {}


def gp_case(name):
	"""Points, observations and the dense float64 reference (numpy.linalg.solve on _kernelop_ref.dense_matrix and the model's C),
	once per profile, read-only."""
	if name not in _gp_cache:
		rng = np.random.default_rng(77)
		Xt = R.points(N_GP, 2, seed=21)
		Xn = R.points(M_GP, 2, seed=22) + 0.5  # [0.5, 1.5]^2: its own mean is far from the training centre
		Xn[:5] = Xt[[3, 50, 120, 200, 299]]
		y = np.stack([np.sin(6 * Xt[:, 0]) + np.sqrt(NOISE_GP) * rng.standard_normal(N_GP), np.cos(4 * Xt[:, 1]) * Xt[:, 0]], axis=1)
		z, zs = R.scaled_points(Xt, LS_GP, F64), X.scaled_new_points(Xt, Xn, LS_GP, F64)
		A = R.dense_matrix(z, name, S_GP, NOISE_GP)
		Cm = X.cross_matrix(zs, z, name, S_GP).astype(F64)
		mean = Cm @ np.linalg.solve(A, y)
		block = Cm @ np.linalg.solve(A, Cm.T)
		for a in (Xt, Xn, y, mean, block):
			a.setflags(write=False)
		_gp_cache[name] = dict(X=Xt, Xnew=Xn, y=y, mean=mean, block=block, cond=float(np.linalg.cond(A)))
	return _gp_cache[name]


@pytest.mark.parametrize("name", ["rbf", "matern32"])
def test_posterior_against_a_dense_solve(name):
	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	G = gp_case(name)
	K = KernelOperator(G["X"], name, lengthscale=LS_GP, outputscale=S_GP, noise=NOISE_GP)
	mean, var, info = gp.posterior(K, G["y"], G["Xnew"], deg=60, orth=None, batch=16)
	assert mean.shape == (M_GP, 2) and var.shape == (M_GP,)
	assert info["deg"] == 60 and info["batches"] == 3 and len(info["steps"]) == 4 and info["zero_columns"] == []
	e_mean = float(np.max(np.abs(mean - G["mean"])) / np.max(np.abs(G["mean"])))
	e_var = float(np.max(np.abs(var - (S_GP - np.diag(G["block"])))) / S_GP)
	print(f"posterior {name}: cond {G['cond']:.2e}, steps {info['steps']}, mean within {e_mean:.2e} of max |mean|, variance within {e_var:.2e} of s")
	assert e_mean <= 1e-9 and e_var <= 1e-9
	assert np.all(var > 0) and np.all(var[:5] < var[5:].max())
	## one column of y is the same solve
	mean1, none, _ = gp.posterior(K, G["y"][:, 0], G["Xnew"], deg=60, batch=16, variance=False)
	assert none is None and mean1.shape == (M_GP,)
	assert np.max(np.abs(mean1 - G["mean"][:, 0])) <= 1e-9 * np.max(np.abs(G["mean"]))


def test_posterior_covariance_and_noise():
	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	G = gp_case("matern32")
	K = KernelOperator(G["X"], "matern32", lengthscale=LS_GP, outputscale=S_GP, noise=NOISE_GP)
	Xn = G["Xnew"][:16]
	mean, var, _ = gp.posterior(K, G["y"], Xn, deg=60, batch=16)
	mean_c, cov, info = gp.posterior(K, G["y"], Xn, deg=60, batch=16, covariance=True)
	assert cov.shape == (16, 16) and info["batches"] == 1 and np.array_equal(mean, mean_c)
	assert np.max(np.abs(cov - cov.T)) <= 1e-12 and np.array_equal(np.diag(cov), var)
	zs = X.scaled_new_points(G["X"], Xn, LS_GP, F64)
	ref = X.cross_matrix(zs, zs, "matern32", S_GP).astype(F64) - G["block"][:16, :16]
	assert np.max(np.abs(cov - ref)) <= 1e-9 * S_GP
	_, var_n, _ = gp.posterior(K, G["y"], Xn, deg=60, batch=16, include_noise=True)
	assert np.array_equal(var_n, var + NOISE_GP)
	_, cov_n, _ = gp.posterior(K, G["y"], Xn, deg=60, batch=16, covariance=True, include_noise=True)
	assert np.array_equal(np.diag(cov_n), var_n) and np.array_equal(cov_n - np.diag(np.diag(cov_n)), cov - np.diag(np.diag(cov)))


@pytest.mark.parametrize("name", ["rbf", "matern32"])
def test_posterior_of_a_point_without_information(name):
	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	G = gp_case(name)
	K = KernelOperator(G["X"], name, lengthscale=LS_GP, outputscale=S_GP, noise=NOISE_GP)
	Xn = np.array(G["Xnew"][:20])
	Xn[7] = [1e3, -1e3]
	mean, var, info = gp.posterior(K, G["y"], Xn, deg=60, batch=16)
	assert info["zero_columns"] == [7] and info["batches"] == 2
	assert np.all(mean[7] == 0.0) and var[7] == S_GP
	assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
	keep = np.arange(20) != 7
	assert np.max(np.abs(mean[keep] - G["mean"][:20][keep])) <= 1e-9 * np.max(np.abs(G["mean"]))
	assert np.max(np.abs(var[keep] - (S_GP - np.diag(G["block"])[:20][keep]))) <= 1e-9 * S_GP
	## a batch of nothing but such points runs no plan
	mean0, var0, info0 = gp.posterior(K, G["y"][:, 0], np.array([[1e3, 1e3], [-1e3, 2e3]]), deg=60)
	assert np.all(mean0 == 0.0) and np.all(var0 == S_GP) and info0["zero_columns"] == [0, 1] and len(info0["steps"]) == 1
