"""The matrix-free kernel operator on the device (slq_kernelop.hpp: k_kernel_rescale, k_kernel_panel) against the
long-double model of tests/_kernelop_ref.py, elementwise within its forward bound - each case first asserts that the bound is a
small fraction of the result (check_condition) - and through everything that runs on an operator unedited: Lanczos parity with
the oracle on the dense matrix of the same rounded points, hyperparameters under graph replay, the drivers.

The shapes are the smallest that reach each piece of index logic: n at both sides of the 16-point tile and the 128-row block, one
tile (one slab, straight into T) and several (the slab sum), d at both sides of the padding to 4 and past 16 (the second register
form), P at both sides of every panel width and two panels with a nearly empty last one. Each item prints its worst ratio to the
bar before it asserts (`-s` shows them)."""

import ctypes as C

import numpy as np
import pytest

import _kernelop_ref as R

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
LD = np.longdouble

## (dtype, n, d, P, profile, lengthscale, outputscale, noise, offset): every value of every axis of the issue at least once
PER3, PER4, PER5 = (0.4, 0.6, 0.8), (0.5, 0.7, 0.9, 1.1), (0.5, 0.6, 0.7, 0.8, 0.9)
CASES = [
	(F64, 1, 1, 1, "rbf", 0.3, 1.0, 0.1, 0.0),
	(F64, 15, 3, 16, "matern12", 0.5, 1.3, 0.0, 0.0),
	(F64, 17, 4, 17, "matern32", PER4, 0.7, 0.05, 0.0),
	(F64, 63, 8, 128, "matern52", 1.0, 1.0, 0.0, 0.0),
	(F64, 65, 5, 64, "rbf", PER5, 2.0, 0.01, 0.0),
	(F64, 257, 17, 130, "matern32", 1.5, 1.0, 0.1, 0.0),
	(F64, 1000, 3, 32, "rbf", 0.5, 1.0, 0.1, 0.0),
	(F64, 257, 3, 16, "matern12", PER3, 1.0, 0.0, 1e4),
	(F32, 1, 1, 1, "rbf", 0.3, 1.0, 0.1, 0.0),
	(F32, 15, 4, 32, "matern52", 0.7, 1.3, 0.0, 0.0),
	(F32, 17, 5, 33, "matern12", PER5, 0.7, 0.05, 0.0),
	(F32, 63, 17, 128, "rbf", 1.5, 1.0, 0.0, 0.0),
	(F32, 65, 5, 260, "matern32", 0.7, 2.0, 0.01, 0.0),
	(F32, 257, 8, 256, "matern52", 1.0, 1.0, 0.1, 0.0),
	(F32, 1000, 3, 64, "rbf", 0.5, 1.0, 0.1, 0.0),
	(F32, 257, 3, 32, "rbf", PER3, 1.0, 0.0, 1e4),
]


def _id(c):
	return f"{np.dtype(c[0]).name}-n{c[1]}-d{c[2]}-P{c[3]}-{c[4]}" + ("-perdim" if isinstance(c[5], tuple) else "") + ("-offset" if c[8] else "")


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


_cache = {}


def case_data(c):
	"""Points, probes, the operator object, the rounded z, and the model's (Y, bar): computed once per case, read-only."""
	if c not in _cache:
		from primate_amd.operators import KernelOperator

		dtype, n, d, P, name, ell, s, noise, offset = c
		X = R.points(n, d, seed=n + d, offset=offset, dtype=dtype)
		W = R.probes(n, P, seed=n + P, dtype=dtype)
		z = R.scaled_points(X, ell, dtype)
		Y, bar = R.model(z, name, s, noise, W)
		for Z in (X, W, z, Y, bar):
			Z.setflags(write=False)
		_cache[c] = (X, W, z, Y, bar, KernelOperator(X, name, lengthscale=ell, outputscale=s, noise=noise, dtype=dtype))
	return _cache[c]


def device_points(op, n, d, dtype):
	"""(z, |z|^2, params) as the product kernel reads them (slq_debug_kernel_points)."""
	from primate_amd import _capi

	dpad, npad = (d + 3) // 4 * 4, (n + 15) // 16 * 16
	zt, nrm, par = np.empty((dpad, npad), dtype), np.empty(npad, dtype), np.empty(2, dtype)
	_capi.check(_capi.lib().slq_debug_kernel_points(op._h, _capi.ptr(zt), _capi.ptr(nrm), _capi.ptr(par)))
	return zt, nrm, par


@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_product_at_every_edge(eng, c):
	"""T = A W through slq_operator_matmat, elementwise within the model's bar; and through a plan: one Lanczos step, whose alpha_0 =
	v^T A v / |v|^2 is within sum_i |v_i| bar_i / |v|^2 + (2 n + 8) eps sum_i |v_i| |Y_i| / |v|^2 (the product's bar through the dot
	product, plus the roundings of the norm, the two scalings and the n-term sum) of the model's. First: the z on the device are the
	model's, bit for bit, zeros in the padding."""
	dtype, n, d, P, name, ell, s, noise, offset = c
	X, W, z, Y, bar, K = case_data(c)
	ratio = R.check_condition(Y, bar, dtype)
	op = eng.DeviceOperator(K)
	try:
		assert op.kind == "kernel" and op.nnz == n * d and op.dtype == np.dtype(dtype)
		zt, nrm, par = device_points(op, n, d, dtype)
		assert np.array_equal(zt[:d, :n].T, z) and not zt[d:].any() and not zt[:, n:].any() and not nrm[n:].any()
		assert par[0] == dtype(s) and par[1] == dtype(noise)
		got = op.matmat(W)
		w_mat = R.worst(got, Y, bar)
		deg = min(2, n)
		plan = eng.LanczosPlan(op, P, deg, 0)
		plan.set_probes(W)
		plan.run()
		a = plan.tridiag()[0][:, 0].astype(LD)
		desc = plan.describe()
		plan.close()
		Wl = W.astype(LD)
		v2 = np.sum(Wl * Wl, axis=0)
		eps = LD(R.eps_of(dtype))
		want = np.sum(Wl * Y, axis=0) / v2
		abar = (np.sum(np.abs(Wl) * bar, axis=0) + LD(2 * n + 8) * eps * np.sum(np.abs(Wl) * np.abs(Y), axis=0)) / v2
		w_plan = float(np.max(np.abs(a - want) / abar))
		print(f"[kernelop] {_id(c)} bar/max|Y| {ratio:.2e} matmat {w_mat:.3f} plan-alpha {w_plan:.3f} panels {desc['panels']}x{desc['panel_width']}")
		assert w_mat <= 1.0 and w_plan <= 1.0
	finally:
		op.close()


def test_bitwise_reproducible(eng):
	c = CASES[5]
	X, W, z, Y, bar, K = case_data(c)
	op = eng.DeviceOperator(K)
	try:
		assert np.array_equal(op.matmat(W), op.matmat(W))
		plan = eng.LanczosPlan(op, 16, 20, 3)
		q = []
		for _ in range(2):
			plan.set_probes(W[:, :16])
			plan.run()
			q.append(plan.quadrature("log"))
		plan.close()
		assert np.all(np.isfinite(q[0])) and np.array_equal(q[0], q[1])
	finally:
		op.close()


## ---- Lanczos and quadrature parity ----------------------------------------------------------------------------------------
PARITY = dict(n=500, d=3, ell=0.2, s=1.0, noise=0.1, deg=20, P=16)  # (ell: lambda_max ~ 46, so that exp stays representable in fp32 rounding terms)


def parity_case(oracle, dtype):
	key = ("parity", np.dtype(dtype).name)
	if key not in _cache:
		from primate_amd.operators import KernelOperator

		p = PARITY
		X = R.points(p["n"], p["d"], seed=77, dtype=dtype)
		z = R.scaled_points(X, p["ell"], dtype)
		A = np.asfortranarray(R.dense_matrix(z, "rbf", p["s"], p["noise"]).astype(dtype))
		rng = np.random.default_rng(5)
		V = np.asfortranarray((np.floor(rng.random((p["n"], p["P"])) * 2) * 2 - 1).astype(dtype))
		ref = {(orth, fun): oracle.quad_batch(A, V, p["deg"], orth, fun=fun, fresh_q=True) for orth in (0, 3, 20) for fun in ("log", "exp")}
		_cache[key] = (KernelOperator(X, "rbf", lengthscale=p["ell"], outputscale=p["s"], noise=p["noise"], dtype=dtype), A, V, ref)
	return _cache[key]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
def test_lanczos_and_quadrature_parity(oracle, eng, dtype):
	"""Per-probe quadrature (log, exp; orth 0, 3, 20; deg 20) against the oracle on the dense A of the same rounded points: 1e-6
	relative in fp64, 3e-4 in fp32 (the bar of the fp32 dense-operator test). The library's dense operator on that A runs
	the same probes; both deviations are printed (DESIGN.md §4.15 quotes them)."""
	K, A, V, ref = parity_case(oracle, dtype)
	limit = 1e-6 if dtype == F64 else 3e-4
	ops = {"kernel": eng.DeviceOperator(K), "dense": eng.DeviceOperator(A)}
	worst = {"kernel": 0.0, "dense": 0.0}
	try:
		for orth in (0, 3, 20):
			for which, op in ops.items():
				plan = eng.LanczosPlan(op, PARITY["P"], PARITY["deg"], orth)
				plan.set_probes(V)
				plan.run()
				for fun in ("log", "exp"):
					e = float(np.max(np.abs(plan.quadrature(fun) / ref[(orth, fun)] - 1.0)))
					print(f"[kernelop-parity] {np.dtype(dtype).name} orth={orth} {fun} {which}: max rel dev from the oracle {e:.3e}")
					worst[which] = max(worst[which], e)
				plan.close()
		print(f"[kernelop-parity] {np.dtype(dtype).name} worst: kernel {worst['kernel']:.3e} dense {worst['dense']:.3e} (limit {limit:g})")
		assert worst["kernel"] <= limit
	finally:
		for op in ops.values():
			op.close()


def test_hyperparameters_under_graph_replay(eng):
	"""quad, set_parameters, quad again on the SAME plan (its captured graph replays): bitwise what a fresh operator and plan created
	with the new values give. get_parameters round-trips."""
	from primate_amd.operators import KernelOperator

	n, d, P = 300, 3, 16
	X = R.points(n, d, seed=9)
	V = R.probes(n, P, seed=9)
	K = KernelOperator(X, "matern52", lengthscale=0.5, outputscale=1.0, noise=0.1)
	op = eng.DeviceOperator(K)
	plan = eng.LanczosPlan(op, P, 20, 3)
	new = dict(lengthscale=[0.3, 0.4, 0.6], outputscale=1.7, noise=0.02)
	try:
		def quad(pl):
			pl.set_probes(V)
			pl.run()
			return pl.quadrature("log")

		q0 = quad(plan)
		assert np.array_equal(q0, quad(plan))  # (the second run replays the graph)
		K.set_parameters(**new)
		got = op.kernel_parameters()
		assert got["d"] == d and got["kernel"] == "matern52" and np.array_equal(got["lengthscale"], new["lengthscale"])
		assert got["outputscale"] == new["outputscale"] and got["noise"] == new["noise"]
		q1 = quad(plan)
		K2 = KernelOperator(X, "matern52", **new)
		op2 = eng.DeviceOperator(K2)
		plan2 = eng.LanczosPlan(op2, P, 20, 3)
		q2 = quad(plan2)
		Y1, Y2 = op.matmat(V), op2.matmat(V)
		plan2.close()
		op2.close()
		assert not np.array_equal(q0, q1) and np.array_equal(q1, q2) and np.array_equal(Y1, Y2)
		## a scalar lengthscale broadcasts on the way back
		K.set_parameters(lengthscale=0.25)
		assert np.array_equal(op.kernel_parameters()["lengthscale"], [0.25] * d)
		with pytest.raises(ValueError, match=r"lengthscale\[1\]"):
			op.set_kernel_parameters([1.0, 0.0, 1.0], 1.0, 0.0)
		assert np.array_equal(op.kernel_parameters()["lengthscale"], [0.25] * d)  # (a refused change changes nothing)
	finally:
		plan.close()
		op.close()


def test_no_n_squared_memory(eng):
	"""n = 20000, d = 3, fp64: a materialised K would be 3.2 GB; the operator takes at most 4 n (d_padded + 2) 8 bytes + 2 MiB of the
	device, and 64 sampled rows of a 16-probe product are within the bar of the model evaluated for those rows only."""
	from primate_amd.operators import KernelOperator

	n, d, P = 20000, 3, 16
	X = R.points(n, d, seed=20)
	W = R.probes(n, P, seed=20)
	K = KernelOperator(X, "rbf", lengthscale=0.2, outputscale=1.0, noise=0.1)
	ctx = eng.default_context()
	ctx.synchronize()
	free0, _ = ctx.meminfo()
	op = eng.DeviceOperator(K, ctx=ctx)
	try:
		free1, _ = ctx.meminfo()
		limit = 4 * n * (4 + 2) * 8 + (2 << 20)
		print(f"[kernelop-memory] operator bytes on the device {free0 - free1} (limit {limit}, dense {8 * n * n})")
		assert free0 - free1 <= limit
		rows = np.sort(np.random.default_rng(3).choice(n, 64, replace=False))
		rows[0], rows[-1] = 0, n - 1
		Y, bar = R.model(R.scaled_points(X, 0.2, F64), "rbf", 1.0, 0.1, W, rows=rows)
		R.check_condition(Y, bar, F64)
		got = op.matmat(W)[rows]
		w = R.worst(got, Y, bar)
		print(f"[kernelop-memory] 64 sampled rows of n = {n}: worst error / bar {w:.2e}")
		assert w <= 1.0
	finally:
		op.close()


## ---- the drivers, unedited --------------------------------------------------------------------------------------------
def driver_case():
	key = "drivers"
	if key not in _cache:
		from primate_amd.operators import KernelOperator

		n, d = 400, 3
		X = R.points(n, d, seed=41)
		kw = dict(lengthscale=0.3, outputscale=1.0, noise=0.1)
		K = KernelOperator(X, "rbf", **kw)
		A = R.dense_matrix(R.scaled_points(X, 0.3, F64), "rbf", 1.0, 0.1)
		lam, U = np.linalg.eigh(A)
		_cache[key] = (K, A, lam, U)
	return _cache[key]


def test_hutch_logdet(oracle, eng):
	"""hutch over MatrixFunction(KernelOperator, log): the estimate within 4 standard errors of slogdet, the per-probe values within
	1e-6 of the oracle's on the dense matrix, and hutch's estimate their mean."""
	from primate_amd.operators import MatrixFunction
	from primate_amd.random import isotropic
	from primate_amd.trace import hutch

	K, A, lam, U = driver_case()
	n, P, deg = A.shape[0], 64, 50
	Z = isotropic(pdf="rademacher", seed=np.random.default_rng(7))(size=(n, P))
	M = MatrixFunction(K, fun="log", deg=deg, orth=3)
	got = M.quad(Z)
	ref = oracle.quad_batch(np.asfortranarray(A), np.asfortranarray(Z), deg, 3, fun="log", fresh_q=True)
	dev = float(np.max(np.abs(got / ref - 1.0)))
	est = hutch(M, converge="count", count=P, seed=7)
	logdet = float(np.linalg.slogdet(A)[1])
	se = float(np.std(got, ddof=1) / np.sqrt(P))
	print(f"[kernelop-drivers] hutch logdet {est:.4f} exact {logdet:.4f} ({abs(est - logdet) / se:.2f} standard errors of {se:.3f}); per-probe dev from the oracle {dev:.2e}")
	assert dev <= 1e-6
	assert est == pytest.approx(float(np.mean(got)), rel=1e-12)
	assert abs(est - logdet) <= 4.0 * se


def test_xtrace_diag_and_recompute_action(eng):
	"""xtrace and diag over MatrixFunction(KernelOperator, exp(-0.1 x)) against the same drivers, same probe stream, over the dense
	f(A) from eigh: 1e-6 relative (the project's parity bar; the deg-30 Lanczos error of exp(-0.1 A) v is below 1e-12 here); and
	MatrixFunction(..., basis="recompute") @ X against eigh."""
	from primate_amd.diagonal import diag
	from primate_amd.operators import MatrixFunction
	from primate_amd.trace import xtrace

	K, A, lam, U = driver_case()
	n = A.shape[0]
	F = (U * np.exp(-0.1 * lam)) @ U.T
	M = MatrixFunction(K, fun="exp", t=-0.1, deg=30, orth=30, basis="recompute")
	Xp = R.probes(n, 24, seed=4)
	Y = M @ Xp
	assert M.basis_used == "recompute"
	e_act = float(np.linalg.norm(Y - F @ Xp) / np.linalg.norm(F @ Xp))
	a, b = xtrace(M, batch=20, count=40, seed=3), xtrace(F, batch=20, count=40, seed=3)
	da, db = diag(M, converge="count", count=48, batch=16, seed=3), diag(F, converge="count", count=48, batch=16, seed=3)
	e_diag = float(np.linalg.norm(da - db) / np.linalg.norm(db))
	print(f"[kernelop-drivers] recompute action rel err {e_act:.2e}; xtrace {a:.6f} dense {b:.6f} exact {np.sum(np.exp(-0.1 * lam)):.6f}; diag rel dev {e_diag:.2e}")
	assert e_act <= 1e-8
	assert abs(a / b - 1.0) <= 1e-6 and abs(a / float(np.sum(np.exp(-0.1 * lam))) - 1.0) <= 3e-2
	assert e_diag <= 1e-6


def test_chebyshev_action_and_kpm_density(eng):
	"""ChebyshevFunction(KernelOperator, log, deg=200) @ X against eigh within its truncation bound: sum_{k > deg} |c_k| |x| (the tail
	from 4x as many coefficients) plus the recurrence's rounding, (k + 1)^2 products' worth of the product's own relative error (2e-13:
	ten times the model's bar for this operator) per coefficient. spectral_density(method="kpm") integrates to 1 (n over n): the
	midpoint rule over 4000 cells of a density with inverse-square-root edges carries 0.6 sqrt(cell / half-width) of the polynomial's
	edge value - 2 % when all the mass sits at an edge, which the noise eigenvalues nearly do - so 5 %."""
	from primate_amd.chebyshev import ChebyshevFunction, chebyshev_coefficients, spectral_bounds
	from primate_amd.integrate import spectral_density

	K, A, lam, U = driver_case()
	n, deg = A.shape[0], 200
	Xp = R.probes(n, 8, seed=6)
	## (the automatic bounds widen both ends by 1 % of the width, which takes the lower end below zero here: the user of a kernel
	## matrix knows lambda_min >= noise, and gives the lower end)
	M = ChebyshevFunction(K, "log", deg=deg, bounds=(0.5 * K.noise, spectral_bounds(K)[1]))
	try:
		Y = M @ Xp
		lo, hi = M.bounds
		assert lo <= lam[0] and lam[-1] <= hi and lo > 0
		truth = (U * np.log(lam)) @ (U.T @ Xp)
		c4 = chebyshev_coefficients("log", 4 * (deg + 1), M.bounds)
		coef = chebyshev_coefficients("log", deg + 1, M.bounds)
		k = np.arange(deg + 1)
		xn = np.linalg.norm(Xp, axis=0)
		bar = (np.sum(np.abs(c4[deg + 1 :])) + np.abs(coef) @ ((k + 1.0) ** 2 * 2e-13)) * xn
		err = np.linalg.norm(Y - truth, axis=0)
		print(f"[kernelop-drivers] Chebyshev log action: max err / bar {float(np.max(err / bar)):.3f} (bar {float(np.max(bar / np.linalg.norm(truth, axis=0))):.2e} relative)")
		assert np.all(err <= bar)
	finally:
		M.close()
	vals, grid = spectral_density(K, bins=4000, method="kpm", deg=100, nprobes=64, batch=64, seed=5)
	integral = float(np.sum(vals) * (grid[1] - grid[0])) / n
	print(f"[kernelop-drivers] kpm density integrates to {integral:.4f}")
	assert abs(integral - 1.0) <= 0.05


def test_torch_points_on_the_gpu(eng):
	"""The same operator from a torch tensor on the context's GPU (slq_kernel_create_device): the same bits."""
	import torch

	from primate_amd.operators import KernelOperator

	for c in (CASES[4], CASES[12]):
		dtype, n, d, P, name, ell, s, noise, offset = c
		X, W, z, Y, bar, K = case_data(c)
		ctx = eng.default_context()
		Xt = torch.as_tensor(np.array(X), device=torch.device("cuda", ctx.device))  # (a writable copy: the cached case is read-only)
		Kt = KernelOperator(Xt, name, lengthscale=ell, outputscale=s, noise=noise)
		assert Kt.dtype == np.dtype(dtype) and np.array_equal(Kt.X, X)
		a, b = eng.DeviceOperator(K), eng.DeviceOperator(Kt)
		try:
			assert np.array_equal(device_points(a, n, d, dtype)[0], device_points(b, n, d, dtype)[0])
			assert np.array_equal(a.matmat(W), b.matmat(W))
		finally:
			a.close()
			b.close()


def test_refusals_through_the_raw_abi(eng):
	from primate_amd import _capi
	from primate_amd.operators import KernelOperator, MatrixFunction

	L, ctx = _capi.lib(), eng.default_context()
	X = R.points(20, 3, seed=2)
	ls = np.array([0.5])
	h = C.c_void_p()
	create = lambda n=20, d=3, pts=X, ldp=3, prof=0, l=ls, nls=1, s=1.0, v=0.0, out=C.byref(h): L.slq_kernel_create(  # noqa: E731
		ctx._h, _capi.SLQ_F64, n, d, _capi.ptr(pts) if pts is not None else None, ldp, prof, _capi.ptr(l) if l is not None else None, nls, s, v, out)
	msg = lambda: L.slq_last_error().decode()  # noqa: E731
	assert create(pts=None) == _capi.SLQ_EINVAL and create(l=None) == _capi.SLQ_EINVAL and create(out=None) == _capi.SLQ_EINVAL
	assert create(d=0) == _capi.SLQ_EINVAL and "d = 0" in msg()
	assert create(d=65, ldp=65) == _capi.SLQ_EINVAL and "d = 65" in msg()
	assert create(n=0) == _capi.SLQ_EINVAL and create(ldp=2) == _capi.SLQ_EINVAL
	assert create(prof=4) == _capi.SLQ_EINVAL and "profile 4" in msg()
	assert create(l=np.array([1.0, 2.0]), nls=2) == _capi.SLQ_EINVAL and "2 lengthscales" in msg()
	assert create(l=np.array([1.0, -1.0, 1.0]), nls=3) == _capi.SLQ_EINVAL and "lengthscale[1]" in msg()
	assert create(s=0.0) == _capi.SLQ_EINVAL and "outputscale" in msg()
	assert create(v=-1.0) == _capi.SLQ_EINVAL and "noise" in msg()
	bad = X.copy()
	bad[7, 2], bad[9, 0] = np.nan, np.inf
	assert create(pts=bad) == _capi.SLQ_EINVAL and "point 7, coordinate 2" in msg()
	assert h.value is None
	## a live operator: the affine parameter is refused with a message that says where to go, the kernel entries refuse other kinds
	K = KernelOperator(X, noise=0.1)
	op = eng.DeviceOperator(K)
	dense = eng.DeviceOperator(np.eye(4))
	try:
		assert L.slq_operator_set_parameter(op._h, 1.0) == _capi.SLQ_EINVAL and "slq_kernel_set_parameters" in msg()
		with pytest.raises(ValueError, match="slq_kernel_set_parameters"):
			op.set_parameter(1.0)
		assert L.slq_kernel_set_parameters(dense._h, _capi.ptr(ls), 1, 1.0, 0.0) == _capi.SLQ_EINVAL
		assert L.slq_kernel_get_parameters(dense._h, None, None, None, 0, None, None) == _capi.SLQ_EINVAL
		assert L.slq_kernel_set_parameters(op._h, None, 1, 1.0, 0.0) == _capi.SLQ_EINVAL
		two = np.empty(2)
		assert L.slq_kernel_get_parameters(op._h, None, None, _capi.ptr(two), 2, None, None) == _capi.SLQ_EINVAL
		nr, nc, nnz, dt = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
		_capi.check(L.slq_operator_shape(op._h, C.byref(nr), C.byref(nc), C.byref(nnz), C.byref(dt)))
		assert (nr.value, nc.value, nnz.value, dt.value) == (20, 20, 60, _capi.SLQ_F64)
		with pytest.raises(ValueError, match="float32"):
			eng.DeviceOperator(K, dtype=np.float32)
		## the plugin cache of lanczos._as_device_operator: one device operator per KernelOperator
		M1, M2 = MatrixFunction(K, "log", deg=8), MatrixFunction(K, "exp", deg=8)
		assert M1._op is M2._op and M1._op.kind == "kernel"
	finally:
		op.close()
		dense.close()
