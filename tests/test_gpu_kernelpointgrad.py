"""Gradients of the kernel operator with respect to the points on the device (k_kernel_pointgrad, slq_kernel_pointgrad_*,
slq_kernel_precond_trace_pointgrad, grad.kernel_point_grad, gp.logdet_grad / gp.mll with points=True, gp.posterior_grad,
autograd.gp_mll_fun): the raw accumulator against the long-double model of `_kernelpointgrad_ref`, elementwise within its forward bar,
in the training form at every case of `_kernelgrad_ref.GPU_CASES` and in the cross form at the issue's five shapes (some new points
bitwise copies of training points); accumulation, alpha and beta, reset, Z is W, run-to-run bits, a parameter change, every refusal,
the device bytes; the exact part against the dense inverse; the drivers. Each item prints its measured figures before it asserts
(`-s` shows them; §4.20 quotes them)."""

import ctypes as C
import gc

import numpy as np
import pytest

import _gp_mll_ref as M
import _kernelcross_ref as XR
import _kernelgrad_ref as G
import _kernelop_ref as R
import _kernelpointgrad_ref as PG
from primate_amd.operators import KernelOperator

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def device_bytes():
	from primate_amd import _capi

	v = C.c_int64()
	_capi.check(_capi.lib().slq_debug_operator_device_bytes(C.byref(v)))
	return v.value


def _device(eng, X, name, ls, s, noise):
	K = KernelOperator(X, name, lengthscale=ls, outputscale=s, noise=noise)
	return K, eng.DeviceOperator(K)


def _matrix(eng, op, A):
	Ad = eng.DeviceMatrix(A.shape[0], A.shape[1], ctx=op.ctx)
	Ad.set(0, A)
	return Ad


def _one_update(eng, target, op, Z, W, alpha=1.0):
	Zd, Wd = _matrix(eng, op, Z), _matrix(eng, op, W)
	acc = eng.KernelPointGradAccumulator(target)
	acc.update(Zd, 0, Wd, 0, Z.shape[1], alpha=alpha, beta=0.0)
	vals, cnt = acc.get()
	for x in (acc, Zd, Wd):
		x.close()
	return vals, cnt


## ---- the two forms against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.GPU_CASES, ids=[G.case_id(c) for c in G.GPU_CASES])
def test_training_form_against_the_model(eng, case):
	(X, ls, s, noise, Z, W), z, P, bar = PG.case_model(case)
	ratio = PG.check_condition(P, bar)
	K, op = _device(eng, X, case[3], ls, s, noise)
	assert np.array_equal(K.scaled_points(), z)
	vals, cnt = _one_update(eng, op, op, Z, W)
	op.close()
	w = PG.worst(vals, P, bar)
	print(f"[pointgrad-training] {G.case_id(case)}: bar / max |P| = {ratio:.2e}, worst |got - model| / bar = {w:.4f}")
	assert cnt == case[2] and vals.shape == (case[0], case[1]) and np.all(np.isfinite(vals))
	assert w <= 1.0, (case, w)


@pytest.mark.parametrize("case", PG.CROSS_CASES, ids=[PG.cross_id(c) for c in PG.CROSS_CASES])
def test_cross_form_against_the_model(eng, case):
	(X, Xn, ls, s, noise, U, W, copies), z, zn, P, bar = PG.cross_model(case)
	ratio = PG.check_condition(P, bar)
	K, op = _device(eng, X, case[4], ls, s, noise)
	cross = eng.KernelCross(op, Xn)
	assert np.array_equal(cross.scaled_points()[0], zn)
	vals, cnt = _one_update(eng, cross, op, U, W)
	cross.close()
	op.close()
	w = PG.worst(vals, P, bar)
	top = float(np.max(np.abs(P)))
	blow = float(np.max(np.abs(vals[copies])) / top) if copies.size else 0.0
	print(f"[pointgrad-cross] {PG.cross_id(case)}: bar / max |R| = {ratio:.2e}, worst |got - model| / bar = {w:.4f}; copies: max |row| / max |R| = {blow:.3f}")
	assert cnt == case[3] and vals.shape == (case[0], case[2]) and np.all(np.isfinite(vals))
	assert w <= 1.0, (case, w)
	assert blow <= 1.0 + 1e-6, "a new point that IS a training point must not blow up"


## ---- the accumulator's behaviour ---------------------------------------------------------------------------------------------------
def test_two_updates_alpha_beta_reset_and_refusals(eng):
	case = (257, 8, 65, "rbf", False, 0.0, False)
	(X, ls, s, noise, Z, W), z, P, bar = PG.case_model(case)
	cut = 30
	P1, bar1 = PG.model(z, "rbf", ls, s, Z[:, :cut], W[:, :cut])
	P2, bar2 = PG.model(z, "rbf", ls, s, Z[:, cut:], W[:, cut:])
	K, op = _device(eng, X, "rbf", ls, s, noise)
	Zd, Wd = _matrix(eng, op, Z), _matrix(eng, op, W)
	acc = eng.KernelPointGradAccumulator(op)
	acc.update(Zd, 0, Wd, 0, 65, beta=0.0)
	one, _ = acc.get()
	acc.update(Zd, 0, Wd, 0, cut, beta=0.0)
	acc.update(Zd, cut, Wd, cut, 65 - cut, beta=1.0)
	two, cnt = acc.get()
	assert cnt == 65 + 65
	w_model, w_one = PG.worst(two, P1 + P2, bar1 + bar2), PG.worst(two, one.astype(LD), bar + bar1 + bar2)
	print(f"[pointgrad-api] two updates: / (bar1 + bar2) against the model {w_model:.4f}; against one update / (bar + bar1 + bar2) {w_one:.4f}")
	assert w_model <= 1.0 and w_one <= 1.0
	## alpha and beta: 2 vals - 0.5 (the last 35 columns)
	acc.update(Zd, cut, Wd, cut, 65 - cut, alpha=-0.5, beta=2.0)
	three, _ = acc.get()
	assert PG.worst(three, 2 * (P1 + P2) - 0.5 * P2, 2 * (bar1 + bar2) + 0.5 * bar2 + 4 * G.EPS * np.abs(2 * (P1 + P2))) <= 1.0
	## reset: zeros and a count of 0; the next update gives the bits of the first
	acc.reset()
	vals, cnt = acc.get()
	assert cnt == 0 and np.array_equal(vals, np.zeros((257, 8)))
	acc.update(Zd, 0, Wd, 0, 65, beta=1.0)
	again, cnt = acc.get()
	assert cnt == 65 and np.array_equal(again, one), "two runs must give identical bits"
	## refused updates leave the values alone
	for args in ((Zd, 0, Wd, 0, 0), (Zd, 60, Wd, 0, 6), (Zd, 0, Wd, -1, 4), (Zd, 0, Wd, 0, 66)):
		with pytest.raises(ValueError, match="columns|m = 0"):
			acc.update(*args)
	short = eng.DeviceMatrix(256, 4, ctx=op.ctx)
	with pytest.raises(ValueError, match="257 points"):
		acc.update(short, 0, Wd, 0, 4)
	with pytest.raises(ValueError, match="257 points"):
		acc.update(Zd, 0, short, 0, 4)
	with pytest.raises(ValueError, match="finite"):
		acc.update(Zd, 0, Wd, 0, 4, alpha=np.nan)
	with pytest.raises(ValueError, match="finite"):
		acc.update(Zd, 0, Wd, 0, 4, beta=np.inf)
	other = eng.Context(device=0)
	foreign = eng.DeviceMatrix(257, 4, ctx=other)
	with pytest.raises(ValueError, match="another context"):
		acc.update(foreign, 0, Wd, 0, 4)
	assert np.array_equal(acc.get()[0], one)
	for x in (foreign, short, acc, Zd, Wd, op):
		x.close()


def test_z_is_w_against_distinct_equal_copies(eng):
	"""Z and W one matrix and one column range: ONE pass with twice the weight; two distinct matrices with equal values: two passes. Both
	within the bar of the model, so within twice the bar of each other; other column ranges of one matrix take the two passes."""
	case = (129, 17, 33, "matern32", False, 0.0, False)
	(X, ls, s, noise, Z, W), z, _, _ = PG.case_model(case)
	P, bar = PG.model(z, "matern32", ls, s, Z, Z)
	K, op = _device(eng, X, "matern32", ls, s, noise)
	Zd, Zc = _matrix(eng, op, Z), _matrix(eng, op, Z)
	acc = eng.KernelPointGradAccumulator(op)
	acc.update(Zd, 0, Zd, 0, 33, beta=0.0)
	same, _ = acc.get()
	acc.update(Zd, 0, Zc, 0, 33, beta=0.0)
	copies, _ = acc.get()
	w_same, w_copies = PG.worst(same, P, bar), PG.worst(copies, P, bar)
	print(f"[pointgrad-api] Z is W: one pass {w_same:.4f} bars, distinct equal copies {w_copies:.4f} bars; max |difference| / bar {PG.worst(same, copies.astype(LD), 2 * bar):.4f}")
	assert w_same <= 1.0 and w_copies <= 1.0
	## one matrix, two different ranges: the general path against the model on those columns
	Pr, barr = PG.model(z, "matern32", ls, s, Z[:, :10], Z[:, 10:20])
	acc.update(Zd, 0, Zd, 10, 10, beta=0.0)
	assert PG.worst(acc.get()[0], Pr, barr) <= 1.0
	for x in (acc, Zd, Zc, op):
		x.close()


def test_identical_bits_over_several_slabs_and_a_parameter_change(eng):
	n, d, m, mnew = 1000, 3, 8, 70
	X, Xn = R.points(n, d, seed=9), R.points(mnew, d, seed=10)
	rng = np.random.default_rng(9)
	Z, W, U = rng.standard_normal((n, m)), rng.standard_normal((n, m)), rng.standard_normal((mnew, m))
	K, op = _device(eng, X, "matern52", 0.4, 1.0, 0.0)
	cross = eng.KernelCross(op, Xn)
	a, _ = _one_update(eng, op, op, Z, W)
	b, _ = _one_update(eng, op, op, Z, W)
	ca, _ = _one_update(eng, cross, op, U, W)
	cb, _ = _one_update(eng, cross, op, U, W)
	assert np.array_equal(a, b) and np.array_equal(ca, cb), "two runs must give identical bits"
	## set_parameters, then update: the next update sees the new operator - the bits of a fresh one, in both forms
	acc, cacc = eng.KernelPointGradAccumulator(op), eng.KernelPointGradAccumulator(cross)
	Zd, Wd, Ud = _matrix(eng, op, Z), _matrix(eng, op, W), _matrix(eng, op, U)
	acc.update(Zd, 0, Wd, 0, m, beta=0.0)
	cacc.update(Ud, 0, Wd, 0, m, beta=0.0)
	K.set_parameters(lengthscale=[0.3, 0.5, 0.7], outputscale=2.5, noise=0.2)
	acc.update(Zd, 0, Wd, 0, m, beta=0.0)
	cacc.update(Ud, 0, Wd, 0, m, beta=0.0)
	changed, cchanged = acc.get()[0], cacc.get()[0]
	K2, op2 = _device(eng, X, "matern52", [0.3, 0.5, 0.7], 2.5, 0.2)
	cross2 = eng.KernelCross(op2, Xn)
	fresh, _ = _one_update(eng, op2, op2, Z, W)
	cfresh, _ = _one_update(eng, cross2, op2, U, W)
	assert np.array_equal(changed, fresh) and not np.array_equal(changed, a)
	assert np.array_equal(cchanged, cfresh) and not np.array_equal(cchanged, ca)
	for x in (acc, cacc, Zd, Wd, Ud, cross, cross2, op, op2):
		x.close()


def test_create_and_cross_refusals(eng):
	import scipy.sparse as sp

	from primate_amd import _capi

	L = _capi.lib()
	msg = lambda: L.slq_last_error().decode()  # noqa: E731
	h = C.c_void_p()
	A = eng.DeviceOperator(sp.identity(40, format="csr"))
	assert L.slq_kernel_pointgrad_create(A.ctx._h, A._h, C.byref(h)) == _capi.SLQ_EINVAL and "kind 'csr'" in msg()
	A.close()
	X = R.points(40, 2, seed=2)
	op32 = eng.DeviceOperator(KernelOperator(X.astype(np.float32), "rbf"))
	assert L.slq_kernel_pointgrad_create(op32.ctx._h, op32._h, C.byref(h)) == _capi.SLQ_EINVAL and "fp32" in msg()
	cross32 = eng.KernelCross(op32, X[:5].astype(np.float32))
	assert L.slq_kernel_pointgrad_create_cross(op32.ctx._h, cross32._h, C.byref(h)) == _capi.SLQ_EINVAL and "fp32" in msg()
	with pytest.raises(ValueError, match="fp64 only"):
		eng.KernelPointGradAccumulator(cross32)
	cross32.close()
	op32.close()
	K = KernelOperator(X, "rbf", lengthscale=0.3, noise=1e-2)
	op = eng.DeviceOperator(K)
	pre = eng.DeviceOperator(K.preconditioned(20))
	assert L.slq_kernel_pointgrad_create(pre.ctx._h, pre._h, C.byref(h)) == _capi.SLQ_EINVAL and "kernel_precond" in msg()
	other = eng.Context(device=0)
	assert L.slq_kernel_pointgrad_create(other._h, op._h, C.byref(h)) == _capi.SLQ_EINVAL and "another context" in msg()
	assert L.slq_kernel_pointgrad_create(op.ctx._h, None, C.byref(h)) == _capi.SLQ_EINVAL and "NULL" in msg()
	assert L.slq_kernel_pointgrad_create_cross(op.ctx._h, None, C.byref(h)) == _capi.SLQ_EINVAL and "NULL" in msg()
	## the cross form's row counts: U on the m new points, W on the n training points
	cross = eng.KernelCross(op, X[:7] + 0.25)
	cacc = eng.KernelPointGradAccumulator(cross)
	U, W = eng.DeviceMatrix(7, 3, ctx=op.ctx), eng.DeviceMatrix(40, 3, ctx=op.ctx)
	U.set(0, np.ones((7, 3)))
	W.set(0, np.ones((40, 3)))
	cacc.update(U, 0, W, 0, 3, beta=0.0)
	before = cacc.get()[0]
	with pytest.raises(ValueError, match="7 new points and 40 training points"):
		cacc.update(W, 0, W, 0, 3)
	with pytest.raises(ValueError, match="7 new points and 40 training points"):
		cacc.update(U, 0, U, 0, 3)
	with pytest.raises(ValueError, match="m = 0"):
		cacc.update(U, 0, W, 0, 0)
	with pytest.raises(ValueError, match="columns"):
		cacc.update(U, 2, W, 0, 2)
	assert np.array_equal(cacc.get()[0], before) and cacc.get()[1] == 3
	assert L.slq_kernel_pointgrad_get(cacc._h, before.ctypes.data_as(C.c_void_p), 1, None) == _capi.SLQ_EINVAL and "ld" in msg()
	## the exact part: a training-form accumulator on the base, a fresh factor, finite weights
	acc, foreign = eng.KernelPointGradAccumulator(pre.base), eng.KernelPointGradAccumulator(op)
	tp = lambda o, a, al=1.0, be=0.0: L.slq_kernel_precond_trace_pointgrad(o._h, a._h if a is not None else None, al, be)  # noqa: E731
	assert tp(op, acc) == _capi.SLQ_EINVAL and "'kernel'" in msg()
	assert tp(pre, foreign) == _capi.SLQ_EINVAL and "another operator" in msg()
	assert tp(pre, cacc) == _capi.SLQ_EINVAL and "cross form" in msg()
	assert tp(pre, None) == _capi.SLQ_EINVAL and "NULL" in msg()
	assert tp(pre, acc, float("nan")) == _capi.SLQ_EINVAL and "finite" in msg()
	with pytest.raises(ValueError, match="preconditioned kernel operator"):
		op.precond_trace_point_grad(foreign)
	pre.precond_trace_point_grad(acc, 1.0, 0.0)
	kept, cnt = acc.get()
	assert cnt == 0, "the exact part folds no probe in: the column count stays"
	K.set_parameters(lengthscale=0.4)
	assert tp(pre, acc) == _capi.SLQ_EINVAL and "stale" in msg()
	assert np.array_equal(acc.get()[0], kept)
	pre.refresh()
	assert tp(pre, acc) == _capi.SLQ_OK and not np.array_equal(acc.get()[0], kept)
	for x in (acc, foreign, cacc, U, W, cross, pre, op):
		x.close()


def test_device_bytes_return_and_the_accumulator_keeps_what_it_borrows(eng):
	case = (17, 4, 4, "matern32", True, 0.0, False)
	(X, ls, s, noise, Z, W), z, P, bar = PG.case_model(case)
	K, op = _device(eng, X, "matern32", ls, s, noise)
	cross = eng.KernelCross(op, X[:5] + 0.125)
	start = device_bytes()
	acc, cacc = eng.KernelPointGradAccumulator(op), eng.KernelPointGradAccumulator(cross)
	assert device_bytes() > start
	acc.close()
	cacc.close()
	assert device_bytes() == start
	## the Python objects: the accumulators outlive a del of what they borrow
	acc, cacc = eng.KernelPointGradAccumulator(op), eng.KernelPointGradAccumulator(cross)
	Zd, Wd = _matrix(eng, op, Z), _matrix(eng, op, W)
	Ud = _matrix(eng, op, Z[:5])
	Xn = cross.scaled_points()[0]
	del op, K, cross
	gc.collect()
	acc.update(Zd, 0, Wd, 0, 4, beta=0.0)
	cacc.update(Ud, 0, Wd, 0, 4, beta=0.0)
	assert PG.worst(acc.get()[0], P, bar) <= 1.0
	Pc, barc = PG.model(z, "matern32", ls, s, Z[:5], W, znew=Xn)
	assert PG.worst(cacc.get()[0], Pc, barc) <= 1.0
	for x in (acc, cacc, Zd, Wd, Ud):
		x.close()


## ---- the exact part tr(P^-1 dA/dx) ----------------------------------------------------------------------------------------------------
def _trace_inverse_points(z, name, ls, s, Xinv):
	"""tr(Xinv dA/dx_ak) for every (a, k) in long double: the model with C = Xinv (Z = Xinv, W = I)."""
	return PG.model(z, name, ls, s, Xinv, np.eye(z.shape[0]))[0]


@pytest.mark.parametrize("c", (M.CASES[1], M.CASES[2]), ids=[M.case_id(M.CASES[1]), M.case_id(M.CASES[2])])
def test_exact_part_against_the_dense_inverse(eng, c):
	"""precond_trace_point_grad against tr(P^-1 dA/dx) of the dense inverse of the device's own L, at 1.0 of the bar §4.19 constructs: this
	model's bar for Z = L H, W = L, times 1 / sigma2 (tr dA/dx = 0: no second term). alpha, beta and run-to-run bits."""
	n, d, name, ell, s, sigma2, rank, note = c
	K = M.operator(c)
	op = eng.DeviceOperator(K.preconditioned(rank))
	acc = eng.KernelPointGradAccumulator(op.base)
	try:
		f = op.factor()
		Lf, Hf = np.array(f["L"]), np.array(f["H"])
		z = R.scaled_points(M.case_points(c), np.asarray(ell, dtype=np.float64), np.float64)
		want = _trace_inverse_points(z, name, ell, s, M.inv_ld(M.dense_p(Lf, sigma2)))
		bar = PG.model(z, name, ell, s, Lf @ Hf, Lf)[1] / LD(sigma2)
		ratio = PG.check_condition(want, bar)
		op.precond_trace_point_grad(acc, 1.0, 0.0)
		got, cnt = acc.get()
		w = PG.worst(got, want, bar)
		print(f"[pointgrad-exact] {M.case_id(c)}: rank {op.info()['rank']} bar / max |g| = {ratio:.2e}, error / bar {w:.3f}")
		assert cnt == 0 and got.shape == (n, d)
		op.precond_trace_point_grad(acc, 1.0, 0.0)
		assert np.array_equal(acc.get()[0], got), "two calls must give identical bits"
		op.precond_trace_point_grad(acc, -0.5, 2.0)  # 2 g - 0.5 g
		assert np.allclose(acc.get()[0], 1.5 * got, rtol=1e-12, atol=0)
		assert w <= 1.0
	finally:
		acc.close()
		op.close()


## ---- the drivers -----------------------------------------------------------------------------------------------------------------------
def test_kernel_point_grad_within_the_bar(eng):
	from primate_amd.grad import kernel_point_grad

	case = (257, 3, 16, "matern12", False, 1e4, True)
	(X, ls, s, noise, Z, W), z, P, bar = PG.case_model(case)
	K = KernelOperator(X, "matern12", lengthscale=ls, outputscale=s, noise=noise)
	assert PG.worst(kernel_point_grad(K, Z, W), P, bar) <= 1.0
	u = Z[:, 0].copy()
	P1, bar1 = PG.model(z, "matern12", ls, s, u, u)
	got = kernel_point_grad(K, u)
	assert got.shape == (257, 3) and PG.worst(got, P1, bar1) <= 1.0
	cc = (5, 40, 3, 2, "matern12")
	(Xc, Xn, lsc, sc, nc, U, Wc, copies), zc, zn, Pc, barc = PG.cross_model(cc)
	Kc = KernelOperator(Xc, "matern12", lengthscale=lsc, outputscale=sc, noise=nc)
	got = kernel_point_grad(Kc, U, Wc, Xnew=Xn)
	assert got.shape == (5, 3) and PG.worst(got, Pc, barc) <= 1.0
	with pytest.raises(ValueError, match="V is required"):
		kernel_point_grad(Kc, U, Xnew=Xn)
	with pytest.raises(ValueError, match="U must be 5 x m and V 40 x m"):
		kernel_point_grad(Kc, Wc, U, Xnew=Xn)


N3, D3, ELL3, S23, RANK3, DEG3 = 400, 2, 0.3, 1e-4, 64, 20
_est = {}


def estimator_setup():
	"""The issue's case (n = 400, rbf, d = 2, lengthscale 0.3, sigma2 = 1e-4, rank 64): the preconditioned operator, the device's L and H,
	the dense A, M = P^{-1/2}, the d derivative matrices dA/dx_.k as n x n arrays A'[a, j] = d A_aj / d x_ak, tr(P^-1 dA/dx), its bar
	and 64 Rademacher probes. Once, read-only."""
	if not _est:
		from primate_amd.lanczos import _as_device_operator

		K = KernelOperator(R.points(N3, D3, seed=400), "rbf", lengthscale=ELL3, outputscale=1.0, noise=S23)
		B = K.preconditioned(RANK3)
		f = _as_device_operator(B, dtype=np.float64).factor()
		Lf, Hf = np.array(f["L"]), np.array(f["H"])
		z = K.scaled_points().astype(np.float64)
		A = M.dense_a(z, "rbf", 1.0, S23).astype(np.float64)
		ch = G.chi("rbf", R.r2_exact(z))
		dA = np.array([(-(LD(1.0) / LD(ELL3)) * ch * (z[:, k].astype(LD)[:, None] - z[:, k].astype(LD)[None, :])).astype(np.float64) for k in range(D3)])
		Minv, condP = M.minv_dense(Lf, S23)
		exact = _trace_inverse_points(z, "rbf", ELL3, 1.0, M.inv_ld(M.dense_p(Lf, S23))).astype(np.float64)
		exact_bar = (PG.model(z, "rbf", ELL3, 1.0, Lf @ Hf, Lf)[1] / LD(S23)).astype(np.float64)
		_est.update(K=K, B=B, A=A, dA=dA, Minv=Minv, condP=condP, exact=exact, exact_bar=exact_bar, W=M.rademacher(N3, 64, seed=17))
	return _est


def _contract(dA, U, V):
	"""[a, k] = (1 / N) sum_c sum_j (U_ac V_jc + V_ac U_jc) dA_k[a, j]: the training form's mean over the N columns, dense."""
	return np.stack([np.sum(U * (Dk @ V), axis=1) + np.sum(V * (Dk @ U), axis=1) for Dk in dA], axis=1) / U.shape[1]


def _oracle_inverse_action(oracle, deg, orth=3):
	"""B^-1 W as `deg` steps of the oracle's Lanczos give it: ||w|| Q T^-1 e_1 per probe (the model's own truncation)."""

	def act(Bd, W):
		n = Bd.shape[0]
		out = np.empty_like(W)
		Bf = np.asfortranarray(Bd)
		for c in range(W.shape[1]):
			a, b, Q = np.zeros(deg + 1), np.zeros(deg + 1), np.zeros((n, deg), order="F")
			k = oracle.lanczos(Bf, W[:, c], deg, 0.0, orth, a, b, Q)
			T = np.diag(a[:k]) + np.diag(b[1:k], 1) + np.diag(b[1:k], -1)
			out[:, c] = np.linalg.norm(W[:, c]) * (Q[:, :k] @ np.linalg.solve(T, np.eye(k)[:, 0]))
		return out

	return act


def _same_entries(a, b, skip=()):
	"""Every entry of dict a is in b with equal bits (dicts and arrays recursively)."""
	for k, v in a.items():
		if k in skip:
			continue
		assert k in b, k
		if isinstance(v, dict):
			_same_entries(v, b[k], skip)
		elif v is None:
			assert b[k] is None, k
		else:
			assert np.array_equal(np.asarray(v), np.asarray(b[k])), k


@pytest.mark.parametrize("on", (True, False), ids=["control-variate", "plain"])
def test_logdet_grad_points_on_explicit_probes(eng, oracle, on):
	"""logdet_grad(points=True) on 64 host Rademacher probes in batches of 8 against the dense evaluation of the same formula on the same
	probes and the device's L. The bar is §4.19's "estimator on explicit probes" bar, elementwise: 100 cond(P) eps S, S = (1/N) sum_c of
	the absolute terms, plus the model's own Lanczos truncation (the oracle's degree-20 inverse action on the dense B against the exact
	solve) plus, with the control variate on, the exact part's bar. Every pre-existing number keeps its bits."""
	from primate_amd import gp

	E = estimator_setup()
	value, grads, info = gp.logdet_grad(E["B"], deg=DEG3, count=64, batch=8, probes=E["W"], control_variate=on, points=True)
	v0, g0, i0 = gp.logdet_grad(E["B"], deg=DEG3, count=64, batch=8, probes=E["W"], control_variate=on)
	assert value == v0 and "points" not in g0
	_same_entries(g0, grads)
	_same_entries(i0, info)
	_, U, Vm = M.estimator_terms(E["A"], E["Minv"], [], E["W"], on)
	_, Ut, _ = M.estimator_terms(E["A"], E["Minv"], [], E["W"], on, Binv_action=_oracle_inverse_action(oracle, DEG3))
	model = _contract(E["dA"], U, Vm) + (E["exact"] if on else 0.0)
	trunc = np.abs(_contract(E["dA"], Ut, Vm) - _contract(E["dA"], U, Vm))
	S = _contract(np.abs(E["dA"]), np.abs(U), np.abs(Vm))
	bar = 100.0 * E["condP"] * EPS64 * S + trunc + (E["exact_bar"] if on else 0.0)
	err = np.abs(grads["points"] - model)
	print(f"[pointgrad-estimator] control variate {on}: max error / bar {np.max(err / bar):.2e} (median truncation share of the bar {np.median(trunc / bar):.1e}); "
		  f"max |points| {np.max(np.abs(grads['points'])):.4e}, max bar {np.max(bar):.3e}")
	assert grads["points"].shape == (N3, D3) and info["control_variate"] is on
	assert np.all(err <= bar)


def test_directional_derivative_statistics(eng):
	"""n = 200: sum P (.) V along one fixed random direction V over 8 seeds of device probes; the mean within 4 standard errors (from the
	8 values) of the exact tr(A^-1 dA/dV). rank 32 at sigma2 = 1e-2 leaves cond(B) = 1.8 (dense model): 30 steps converge, so the
	truncation is no bias, and the sampled part is real - a dense model with exact solves gives a standard error of 8 % of the value
	(rank 16: cond(B) = 43 and an error of twice the value, which would test nothing; rank 48: 0.4 %, the exact part alone)."""
	from primate_amd import gp

	n, d = 200, 2
	X = R.points(n, d, seed=200)
	K = KernelOperator(X, "rbf", lengthscale=0.3, outputscale=1.0, noise=1e-2)
	B = K.preconditioned(32)
	V = np.random.default_rng(200).standard_normal((n, d))
	z = K.scaled_points().astype(np.float64)
	exact = float(np.sum(_trace_inverse_points(z, "rbf", 0.3, 1.0, M.inv_ld(M.dense_a(z, "rbf", 1.0, 1e-2))) * V))
	vals = np.array([float(np.sum(gp.logdet_grad(B, deg=30, count=32, batch=8, seed=seed, points=True)[1]["points"] * V)) for seed in range(8)])
	se = float(np.std(vals, ddof=1) / np.sqrt(vals.size))
	print(f"[pointgrad-statistics] tr(A^-1 dA/dV) {exact:.6e}; 8 seeds: mean {vals.mean():.6e} +- {se:.2e} ({abs(vals.mean() - exact) / se:.2f} standard errors)")
	assert abs(vals.mean() - exact) <= 4 * se


def test_mll_points_by_its_parts(eng):
	"""The setting of the existing mll test (n = 300, matern52, d = 3, sigma2 = 1e-3, rank 100, solve_deg 150, y with a zero column): the
	data-fit part within 100 cond(A) eps (relative to its largest component) of the dense solve, the log-determinant part equal to
	logdet_grad(points=True)'s on the same seed bit for bit, the total assembled from the two with ==, and every pre-existing entry of
	grads and info equal, bit for bit, to the call without points."""
	from primate_amd import gp

	n, d, s, sigma2 = 300, 3, 1.2, 1e-3
	rng = np.random.default_rng(719)
	X = rng.random((n, d))
	y = np.zeros((n, 2))
	y[:, 0] = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(n)
	K = KernelOperator(X, "matern52", lengthscale=0.4, outputscale=s, noise=sigma2)
	kw = dict(rank=100, deg=20, solve_deg=150, count=32, batch=8, seed=5)
	value, grads, info = gp.mll(K, y, points=True, **kw)
	v0, g0, i0 = gp.mll(K, y, **kw)
	assert value == v0 and "points" not in g0 and "datafit_points" not in i0
	_same_entries(g0, grads)
	_same_entries(i0, info)
	z = K.scaled_points().astype(np.float64)
	A = M.dense_a(z, "matern52", s, sigma2)
	alpha = M.inv_ld(A) @ y[:, 0].astype(LD)
	want = (LD(0.5) * PG.model(z, "matern52", 0.4, s, alpha, alpha)[0]).astype(np.float64)
	cond = float(np.linalg.cond(A.astype(np.float64)))
	bar = 100.0 * cond * EPS64
	e_fit = float(np.max(np.abs(info["datafit_points"] - want)) / np.max(np.abs(want)))
	print(f"[pointgrad-mll] cond(A) {cond:.2e} bar {bar:.2e}: data-fit point gradient within {e_fit:.2e} of its largest component {np.max(np.abs(want)):.3e}")
	assert e_fit <= bar
	_, ld_grads, _ = gp.logdet_grad(K, points=True, **{k: v for k, v in kw.items() if k != "solve_deg"})
	assert np.array_equal(info["logdet_points"], ld_grads["points"])
	assert grads["points"].shape == (n, d) and np.all(grads["points"] == info["datafit_points"] - 0.5 * 2 * info["logdet_points"])
	## rank = 0: everything on A itself (for large noise); the same assembly
	K0 = KernelOperator(X, "matern52", lengthscale=0.4, outputscale=s, noise=0.5)
	_, gr, inf = gp.mll(K0, y[:, 0], rank=0, deg=30, count=16, batch=8, seed=1, points=True)
	assert np.all(gr["points"] == inf["datafit_points"] - 0.5 * inf["logdet_points"]) and np.all(np.isfinite(gr["points"]))
	_, gr0, inf0 = gp.mll(K0, y[:, 0], rank=0, deg=30, count=16, batch=8, seed=1)
	_same_entries(gr0, gr)
	_same_entries(inf0, inf)


def test_the_chebyshev_route_refuses_points(eng):
	from primate_amd.chebyshev import ChebyshevFunction
	from primate_amd.grad import kernel_trace_grad

	K = KernelOperator(R.points(50, 2, seed=1), "rbf", lengthscale=0.4, noise=0.1)
	with pytest.raises(ValueError, match="Chebyshev route"):
		kernel_trace_grad(ChebyshevFunction(K, "log", deg=10, bounds=(0.05, 60.0)), count=8, points=True)


## ---- gp.posterior_grad ------------------------------------------------------------------------------------------------------------------
N_GP, M_GP, S_GP, LS_GP = 300, 40, 1.5, 0.4
_gp_cache = {}


def gp_case(noise):
	"""Points, observations (two columns) and the dense long-double posterior as a function of the new points, with its central
	differences in X* and their own error; once per noise, read-only. 5 of the 40 new points ARE training points."""
	if noise not in _gp_cache:
		rng = np.random.default_rng(77)
		Xt = R.points(N_GP, 2, seed=21)
		Xn = R.points(M_GP, 2, seed=22) * 0.9 + 0.3  # [0.3, 1.2]^2: partly outside the data, its own mean not the training centre
		Xn[:5] = Xt[[3, 50, 120, 200, 299]]
		y = np.stack([np.sin(6 * Xt[:, 0]) + np.sqrt(0.1) * rng.standard_normal(N_GP), np.cos(4 * Xt[:, 1]) * Xt[:, 0]], axis=1)
		z = R.scaled_points(Xt, LS_GP, np.float64)
		A = M.dense_a(z, "rbf", S_GP, noise)
		Ainv = M.inv_ld(A)
		alpha = Ainv @ y.astype(LD)

		def post(Xs):
			Cm = LD(S_GP) * R.phi("rbf", XR.r2_cross(XR.scaled_new_points(Xt, Xs, LS_GP, np.float64), z))
			return Cm @ alpha, LD(S_GP) - np.sum((Cm @ Ainv) * Cm, axis=1)

		h = 1e-4
		dmean, dvar, emean, evar = np.zeros((M_GP, 2, 2), dtype=LD), np.zeros((M_GP, 2), dtype=LD), np.zeros((M_GP, 2, 2), dtype=LD), np.zeros((M_GP, 2), dtype=LD)
		m0, v0 = post(Xn)
		for k in range(2):
			def at(t, k=k):
				Xs = Xn.copy()
				Xs[:, k] += t
				return post(Xs)
			(mp, vp), (mm, vm), (mp2, vp2), (mm2, vm2) = at(h), at(-h), at(2 * h), at(-2 * h)
			for f0, fp, fm, fp2, fm2, out, err in ((m0, mp, mm, mp2, mm2, dmean[:, k], emean[:, k]), (v0, vp, vm, vp2, vm2, dvar[:, k], evar[:, k])):
				d1, d2 = (fp - fm) / (2 * h), (fp2 - fm2) / (4 * h)
				out[...] = d1
				## the difference's own error: the h^2 remainder from the step 2 h, and the rounding of z* (a staircase at eps) as eps |f| / h
				err[...] = np.abs(d1 - d2) / 3 + 4 * R.eps_of(np.float64) * (np.abs(f0) + S_GP) / h
		_gp_cache[noise] = dict(X=Xt, Xnew=Xn, y=y, dmean=dmean, dvar=dvar, emean=emean, evar=evar, cond=float(np.linalg.cond(A.astype(np.float64))))
	return _gp_cache[noise]


@pytest.mark.parametrize("noise,rank", ((0.1, 0), (1e-4, 64)), ids=["plain-noise0.1", "precond64-noise1e-4"])
def test_posterior_grad_against_central_differences(eng, noise, rank):
	"""n = 300, 40 new points of which 5 are training points, a two-column y, batches of 16: dmean and dvar against central differences of
	the dense long-double posterior in X*, within 100 cond(A) eps of the largest component plus the difference's own error (with the
	factor 4 on it that the CPU tests use). posterior itself gives the same bits before and after."""
	from primate_amd import gp

	Gc = gp_case(noise)
	K = KernelOperator(Gc["X"], "rbf", lengthscale=LS_GP, outputscale=S_GP, noise=noise)
	before = gp.posterior(K, Gc["y"], Gc["Xnew"], deg=60, batch=16, precond_rank=rank)
	dmean, dvar, info = gp.posterior_grad(K, Gc["y"], Gc["Xnew"], deg=60, batch=16, precond_rank=rank)
	after = gp.posterior(K, Gc["y"], Gc["Xnew"], deg=60, batch=16, precond_rank=rank)
	assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2] == info
	assert dmean.shape == (M_GP, 2, 2) and dvar.shape == (M_GP, 2) and info["batches"] == 3
	rel = 100.0 * Gc["cond"] * EPS64
	bar_m = rel * float(np.max(np.abs(Gc["dmean"]))) + 4 * Gc["emean"]
	bar_v = rel * float(np.max(np.abs(Gc["dvar"]))) + 4 * Gc["evar"]
	em, ev = np.abs(dmean - Gc["dmean"]), np.abs(dvar - Gc["dvar"])
	print(f"[pointgrad-posterior] noise {noise} rank {rank}: cond(A) {Gc['cond']:.2e}, 100 cond eps {rel:.2e}; dmean error / bar {float(np.max(em / bar_m)):.3f} "
		  f"(max |dmean| {float(np.max(np.abs(Gc['dmean']))):.3e}, max error {float(np.max(em)):.2e}); dvar error / bar {float(np.max(ev / bar_v)):.3f} "
		  f"(max |dvar| {float(np.max(np.abs(Gc['dvar']))):.3e}, max error {float(np.max(ev)):.2e}); steps {info['steps']}")
	assert np.all(em <= bar_m) and np.all(ev <= bar_v)
	## a vector y: m x d; variance=False: no second array
	d1, none, _ = gp.posterior_grad(K, Gc["y"][:, 0], Gc["Xnew"], deg=60, batch=16, variance=False, precond_rank=rank)
	assert none is None and d1.shape == (M_GP, 2) and np.all(np.abs(d1 - Gc["dmean"][:, :, 0]) <= bar_m[:, :, 0])


def test_posterior_grad_zero_columns_are_exactly_zero(eng):
	from primate_amd import gp

	Gc = gp_case(0.1)
	K = KernelOperator(Gc["X"], "rbf", lengthscale=LS_GP, outputscale=S_GP, noise=0.1)
	Xn = Gc["Xnew"][:6].copy()
	Xn[2] = [1e3, 1e3]  # phi underflows against every training point
	y = Gc["y"].copy()
	y[:, 1] = 0.0
	dmean, dvar, info = gp.posterior_grad(K, y, Xn, deg=60, batch=16)
	assert info["zero_columns"] == [2]
	assert np.all(dvar[2] == 0.0) and np.all(dmean[2] == 0.0) and np.all(dmean[:, :, 1] == 0.0)
	assert np.all(np.isfinite(dmean)) and np.all(np.isfinite(dvar)) and np.any(dvar[0] != 0.0)


## ---- torch ---------------------------------------------------------------------------------------------------------------------------
def test_gp_mll_fun_gives_the_points_their_gradient(eng):
	import torch

	from primate_amd import gp
	from primate_amd.autograd import gp_mll_fun

	rng = np.random.default_rng(3)
	X = rng.random((150, 2))
	y = np.cos(4.0 * X[:, 0]) + 0.05 * rng.standard_normal(150)
	ls0, s0, v0 = np.array([0.3, 0.5]), 1.1, 1e-3
	K = KernelOperator(X, "matern52", lengthscale=ls0, outputscale=s0, noise=v0)
	value, grads, _ = gp.mll(K, y, rank=40, deg=20, count=16, batch=8, seed=2, points=True)
	for scale in (1.0, 3.0):
		ls = torch.tensor(ls0, dtype=torch.float64, requires_grad=True)
		Xt = torch.tensor(X, dtype=torch.float64, requires_grad=True)
		out = gp_mll_fun(Xt, torch.from_numpy(y), "matern52", ls, s0, v0, rank=40, deg=20, count=16, seed=2, batch=8)
		assert float(out.detach()) == value
		(scale * out).backward()
		assert Xt.grad.shape == (150, 2) and np.array_equal(Xt.grad.numpy(), scale * grads["points"])
		assert np.array_equal(ls.grad.numpy(), scale * grads["lengthscale"])
	## without requires_grad the points are data: no gradient, the same value
	ls = torch.tensor(ls0, dtype=torch.float64, requires_grad=True)
	Xt = torch.tensor(X, dtype=torch.float64)
	out = gp_mll_fun(Xt, torch.from_numpy(y), "matern52", ls, s0, v0, rank=40, deg=20, count=16, seed=2, batch=8)
	out.backward()
	assert Xt.grad is None and float(out.detach()) == value and np.array_equal(ls.grad.numpy(), grads["lengthscale"])


def test_kernel_trace_fun_gives_the_points_their_gradient(eng):
	import torch

	from primate_amd.autograd import kernel_trace_fun
	from primate_amd.grad import kernel_trace_grad
	from primate_amd.operators import MatrixFunction

	X = R.points(200, 2, seed=4)
	K = KernelOperator(X, "matern52", lengthscale=0.35, outputscale=1.2, noise=0.1)
	est, grads, _ = kernel_trace_grad(MatrixFunction(K, "log", deg=20), pdf="device:rademacher", count=48, batch=32, seed=5, points=True)
	est0, grads0, _ = kernel_trace_grad(MatrixFunction(K, "log", deg=20), pdf="device:rademacher", count=48, batch=32, seed=5)
	assert est == est0 and "points" not in grads0
	_same_entries(grads0, grads)
	Xt = torch.tensor(X, dtype=torch.float64, requires_grad=True)
	ls = torch.tensor(0.35, dtype=torch.float64, requires_grad=True)
	(3 * kernel_trace_fun(Xt, "matern52", ls, 1.2, 0.1, "log", deg=20, count=48, seed=5, batch=32)).backward()
	assert np.array_equal(Xt.grad.numpy(), 3.0 * grads["points"]) and float(ls.grad) == 3.0 * float(grads["lengthscale"][0])
	with pytest.raises(ValueError, match="Chebyshev route"):
		kernel_trace_fun(Xt, "matern52", ls, 1.2, 0.1, "log", deg=20, count=8, method="chebyshev", bounds=(0.05, 300.0))
