"""The pivoted-Cholesky preconditioner of the kernel operator on the device (slq_kernelprecond.hpp: k_precond_column,
k_precond_lt, k_precond_gz, k_precond_nn) on the issue's case table: the factor against the long-double model within the forward
bounds of tests/_kernelprecond_ref.py (the CPU emulation is held to half of them), the apply M = P^{-1/2} against eigh of the P the
device's own L defines, the product B = M A M, Lanczos parity with the oracle on the dense B, log-determinants and GP prediction at
noise 1e-4 end to end, refresh under graph replay, reproducibility, lifetime and every refusal. Each item prints its measured
fractions before it asserts (`-s` shows them; §4.18 quotes them)."""

import ctypes as C
import gc

import numpy as np
import pytest

import _kernelop_ref as R
import _kernelprecond_ref as P

pytestmark = pytest.mark.gpu
IDS = [P.case_id(c) for c in P.CASES]


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


_cache = {}


def device_case(eng, c):
	"""The case's operator on the device with its factor read back, and the dense P^{-1/2} of that factor: once per case."""
	if c not in _cache:
		K = P.operator(c)
		op = eng.DeviceOperator(K.preconditioned(c[6]))
		f = op.factor()
		Minv, cond, logdet_p, _ = P.dense_p(f["L"], c[5])
		X = R.probes(c[0], max(P.COLUMN_COUNTS), seed=c[0] + 1)
		for a in (f["L"], f["pivots"], f["G"], Minv, X):
			a.setflags(write=False)
		_cache[c] = dict(K=K, op=op, f=f, Minv=Minv, cond=cond, logdet_p=logdet_p, X=X)
	return _cache[c]


def device_bytes():
	from primate_amd import _capi

	v = C.c_int64(-1)
	_capi.check(_capi.lib().slq_debug_operator_device_bytes(C.byref(v)))
	return v.value


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_factor(eng, c):
	"""Distinct pivots, the residual, the interpolation at every pivot and the greedy choice at every step, at 1.0 of the bars; the
	early-stop case stops within 2 columns of the model's rank, with zero columns beyond."""
	D = device_case(eng, c)
	op, f = D["op"], D["f"]
	n, rank_max = c[0], min(c[6], c[0])
	assert op.kind == "kernel_precond" and op.shape == (n, n) and op.dtype == np.float64
	got = P.check_factor(c, np.array(f["L"]), np.array(f["pivots"]).astype(np.int64), 1.0, "device")
	info = op.info()
	assert info["rank_max"] == rank_max and info["rank"] == got["rank"]
	z, K0, dK = P.k0_model(c)
	model_rank = int(np.sum(P.factor(P.emulate_k0(z, c[2], c[4]), c[4], c[6])[1] >= 0))
	if c is P.EARLY_STOP:
		assert got["rank"] < rank_max and abs(got["rank"] - model_rank) <= 2
	else:
		assert got["rank"] == rank_max
	## G and the eigenvalues: G = V g(t) V^T of the device's own L^T L, against NumPy's eigh (the bar of the apply covers G's use)
	L = np.array(f["L"])
	t = np.linalg.eigvalsh(L.T @ L)
	assert np.max(np.abs(np.sort(f["eig"]) - t)) <= 64 * np.finfo(np.float64).eps * rank_max * max(t[-1], 1e-300)
	assert np.array_equal(f["G"], f["G"].T)
	assert info["t_max"] == pytest.approx(float(t[-1]), rel=1e-12)
	## sum d against the model's s n - sum L^2 (forward: the residual bars summed)
	assert info["residual_trace"] == pytest.approx(c[4] * n - float(np.sum(L * L)), abs=1e-9 * c[4] * n)


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_apply(eng, c):
	"""slq_kernel_precond_apply and _apply_dmat on 1, 16, 65, 260 columns against eigh(P)^{-1/2} X with P from the device's L, within
	16 eps cond(P) max |ref|; the two entries agree bit for bit; logdet P against slogdet at 1e-9 n."""
	D = device_case(eng, c)
	op, n = D["op"], c[0]
	worst = 0.0
	for b in P.COLUMN_COUNTS:
		X = np.asfortranarray(D["X"][:, :b])
		ref = D["Minv"] @ X
		got = op.inv_sqrt(X)
		IN, OUT = eng.DeviceMatrix(n, b + 1, ctx=op.ctx), eng.DeviceMatrix(n, b + 2, ctx=op.ctx)
		try:
			IN.set(1, X)
			op.inv_sqrt_dmat(IN, 1, OUT, 2, b)
			got2 = OUT.get(2, b)
		finally:
			IN.close()
			OUT.close()
		assert np.array_equal(got, got2), f"b = {b}: the host and the device-matrix entry differ"
		worst = max(worst, float(np.max(np.abs(got - ref))) / P.apply_bar(D["cond"], ref))
	lp = op.info()["logdet_p"]
	print(f"[kernelprecond-apply] {P.case_id(c)}: cond(P) {D['cond']:.2e} worst error / (16 eps cond max|ref|) {worst:.4f}; logdet P {lp:.6f} slogdet {D['logdet_p']:.6f}")
	assert worst <= 1.0
	assert abs(lp - D["logdet_p"]) <= 1e-9 * n


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_product(eng, c):
	"""slq_operator_matmat on the same column counts against the dense M A M X from the device's L and the long-double A, within the
	bar of _kernelprecond_ref.product_model at 1.0."""
	D = device_case(eng, c)
	op = D["op"]
	Y, bar = P.product_model(c, np.array(D["f"]["L"]), np.array(D["X"]))
	worst = 0.0
	for b in P.COLUMN_COUNTS:
		got = op.matmat(np.asfortranarray(D["X"][:, :b]))
		worst = max(worst, float(np.max(np.max(np.abs(got - Y[:, :b]), axis=0) / bar[:b])))
	print(f"[kernelprecond-product] {P.case_id(c)}: worst error / bar {worst:.2e} (bar / max|Y| {float(np.max(bar / np.max(np.abs(Y), axis=0))):.2e})")
	assert worst <= 1.0
	assert np.array_equal(op.matmat(np.asfortranarray(D["X"][:, :16])), op.matmat(np.asfortranarray(D["X"][:, :16])))


## ---- Lanczos parity -------------------------------------------------------------------------------------------------------
PARITY = dict(n=500, d=3, ell=0.2, s=1.0, noise=1e-3, rank=64, deg=20, P=16)


@pytest.mark.parametrize("name", ["rbf", "matern32"])
def test_lanczos_parity(oracle, eng, name):
	"""Per-probe quadrature of log (deg 20; orth 0, 3, 20; 16 Rademacher probes) against the oracle on the dense B = M A M built from
	the device's L: 1e-6 relative, the bar of the kernel operator's own parity test. Keep and recompute plans compute the same
	Jacobi matrices, bit for bit, as they do on a kernel operator."""
	from primate_amd.operators import KernelOperator

	p = PARITY
	X = R.points(p["n"], p["d"], seed=78)
	K = KernelOperator(X, name, lengthscale=p["ell"], outputscale=p["s"], noise=p["noise"])
	op = eng.DeviceOperator(K.preconditioned(p["rank"]))
	try:
		Minv, cond, _, _ = P.dense_p(op.factor()["L"], p["noise"])
		A = R.dense_matrix(R.scaled_points(X, p["ell"], np.float64), name, p["s"], p["noise"])
		B = Minv @ A @ Minv
		B = np.asfortranarray(0.5 * (B + B.T))
		rng = np.random.default_rng(5)
		V = np.asfortranarray(np.floor(rng.random((p["n"], p["P"])) * 2) * 2 - 1)
		worst = 0.0
		for orth in (0, 3, 20):
			ref = oracle.quad_batch(B, V, p["deg"], orth, fun="log", fresh_q=True)
			tri = {}
			for basis in (None, "keep", "recompute"):
				plan = eng.LanczosPlan(op, p["P"], p["deg"], orth, basis=basis)
				plan.set_probes(V)
				plan.run()
				q = plan.quadrature("log")
				tri[basis] = plan.tridiag()
				plan.close()
				e = float(np.max(np.abs(q - ref)) / np.max(np.abs(ref)))
				worst = max(worst, e)
				print(f"[kernelprecond-parity] {name} orth={orth} basis={basis}: max dev from the oracle {e:.3e} of max |quad| (cond B {np.linalg.cond(B):.3f}, cond A {np.linalg.cond(A):.2e})")
			assert all(np.array_equal(a, b) for a, b in zip(tri["keep"], tri["recompute"]))
		assert worst <= 1e-6
	finally:
		op.close()


def test_chebyshev_action_runs_on_it(eng):
	"""A Chebyshev action plan on the preconditioned operator of the end-to-end case (n = 400, rbf, noise 1e-4, rank 64: cond B ~ 1.2):
	log(B) X against eigh of the dense B at 1e-6 relative, the project's parity bar; the truncation of the degree-40 series on the
	bounds used is asserted below 1e-9 first (the tail of four times as many coefficients), so the bar is about the products."""
	from primate_amd.chebyshev import ChebyshevFunction, chebyshev_coefficients
	from primate_amd.operators import KernelOperator

	n, deg = 400, 40
	Xp = R.points(n, 2, seed=400)
	K = KernelOperator(Xp, "rbf", lengthscale=0.3, outputscale=1.0, noise=1e-4)
	Bop = K.preconditioned(64)
	M = ChebyshevFunction(Bop, "log", deg=deg, bounds=(0.5, 2.0))
	try:
		Minv, cond, _, _ = P.dense_p(M._op.factor()["L"], 1e-4)
		A = R.dense_matrix(K.scaled_points(), "rbf", 1.0, 1e-4)
		B = Minv @ A @ Minv
		lam, U = np.linalg.eigh(0.5 * (B + B.T))
		assert 0.5 < lam[0] and lam[-1] < 2.0 and lam[0] >= 1.0 - 1e-9  # (A - P = K0 - L L^T is positive semi-definite: B >= I)
		tail = float(np.sum(np.abs(chebyshev_coefficients("log", 4 * (deg + 1), M.bounds)[deg + 1 :])))
		assert tail <= 1e-9
		X = R.probes(n, 8, seed=6)
		Y = M @ X
		truth = (U * np.log(lam)) @ (U.T @ X)
		e = float(np.linalg.norm(Y - truth) / np.linalg.norm(truth))
		print(f"[kernelprecond-cheb] log(B) X by a Chebyshev action, deg {deg} on [0.5, 2]: rel err {e:.2e} (series tail {tail:.1e}, B in [{lam[0]:.6f}, {lam[-1]:.4f}])")
		assert e <= 1e-6
	finally:
		M.close()


## ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_logdet_end_to_end(eng):
	"""n = 400, rbf, lengthscale 0.3, noise 1e-4, rank 64: gp.logdet with 32 probes of degree 20 is within 4 of its own standard errors
	+ 1e-6 |exact| of slogdet of the dense model, and its standard error is below 1.0 (CPU model: 0.05; the plain estimator: 26)."""
	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	n = 400
	X = R.points(n, 2, seed=400)
	K = KernelOperator(X, "rbf", lengthscale=0.3, outputscale=1.0, noise=1e-4)
	exact = float(np.linalg.slogdet(R.dense_matrix(K.scaled_points(), "rbf", 1.0, 1e-4))[1])
	est, info = gp.logdet(K, rank=64, deg=20, count=32, seed=3)
	print(f"[kernelprecond-logdet] estimate {est:.4f} exact {exact:.4f}: {abs(est - exact) / info['std_error']:.2f} standard errors of {info['std_error']:.4f}; rank {info['rank']}, logdet P {info['logdet_precond']:.4f}, trace part {info['trace']:.4f}")
	assert info["rank"] == 64 and info["count"] == 32
	assert info["std_error"] < 1.0
	assert abs(est - exact) <= 4.0 * info["std_error"] + 1e-6 * abs(exact)
	plain, pinfo = gp.logdet(K, rank=0, deg=20, count=32, seed=3)
	print(f"[kernelprecond-logdet] plain estimate (rank 0) {plain:.2f}, standard error {pinfo['std_error']:.2f}")
	assert pinfo["rank"] == 0 and pinfo["logdet_precond"] == 0.0


def test_posterior_with_preconditioner():
	"""n = 300, d = 2, rbf, lengthscale 0.4, s = 1.5, noise 1e-4, 40 new points of which 5 are training points, two columns of y,
	batch 16, precond_rank 64, deg 30: mean (relative to max |mean|) and variance (relative to s) within 100 cond(A) eps of a dense
	float64 solve. precond_rank = 0 at noise 0.1 is the call without the argument, bit for bit."""
	import _kernelcross_ref as XR
	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	n, m, s, noise, ell = 300, 40, 1.5, 1e-4, 0.4
	rng = np.random.default_rng(77)
	Xt = R.points(n, 2, seed=21)
	Xn = R.points(m, 2, seed=22) + 0.5
	Xn[:5] = Xt[[3, 50, 120, 200, 299]]
	y = np.stack([np.sin(6 * Xt[:, 0]) + np.sqrt(noise) * rng.standard_normal(n), np.cos(4 * Xt[:, 1]) * Xt[:, 0]], axis=1)
	z, zs = R.scaled_points(Xt, ell, np.float64), XR.scaled_new_points(Xt, Xn, ell, np.float64)
	A = R.dense_matrix(z, "rbf", s, noise)
	Cm = XR.cross_matrix(zs, z, "rbf", s).astype(np.float64)
	ref_mean = Cm @ np.linalg.solve(A, y)
	ref_var = s - np.diag(Cm @ np.linalg.solve(A, Cm.T))
	bar = 100.0 * float(np.linalg.cond(A)) * float(np.finfo(np.float64).eps)
	K = KernelOperator(Xt, "rbf", lengthscale=ell, outputscale=s, noise=noise)
	mean, var, info = gp.posterior(K, y, Xn, deg=30, batch=16, precond_rank=64)
	e_mean = float(np.max(np.abs(mean - ref_mean)) / np.max(np.abs(ref_mean)))
	e_var = float(np.max(np.abs(var - ref_var)) / s)
	print(f"[kernelprecond-posterior] cond(A) {np.linalg.cond(A):.2e}, bar {bar:.2e}: mean within {e_mean:.2e} of max |mean|, variance within {e_var:.2e} of s; steps {info['steps']}")
	assert mean.shape == (m, 2) and var.shape == (m,) and info["batches"] == 3
	assert e_mean <= bar and e_var <= bar
	K1 = KernelOperator(Xt, "rbf", lengthscale=ell, outputscale=s, noise=0.1)
	a = gp.posterior(K1, y, Xn, deg=60, batch=16)
	b = gp.posterior(K1, y, Xn, deg=60, batch=16, precond_rank=0)
	assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


## ---- refresh, reproducibility, lifetime ---------------------------------------------------------------------------------------
def test_refresh_and_graph_replay(eng):
	"""quad on a plan; set_parameters on the base: the same plan raises "stale"; after refresh the same plan (its captured graph
	replays, the factor's addresses are the old ones) gives the bits of a fresh base + preconditioner + plan."""
	from primate_amd.operators import KernelOperator

	n, d, Pn, rank = 300, 3, 16, 40
	X = R.points(n, d, seed=9)
	V = R.probes(n, Pn, seed=9)
	K = KernelOperator(X, "matern52", lengthscale=0.5, outputscale=1.0, noise=1e-3)
	new = dict(lengthscale=[0.3, 0.4, 0.6], outputscale=1.7, noise=2e-3)
	op = eng.DeviceOperator(K.preconditioned(rank))
	plan = eng.LanczosPlan(op, Pn, 20, 3)

	def quad(pl):
		pl.set_probes(V)
		pl.run()
		return pl.quadrature("log")

	try:
		q0 = quad(plan)
		assert np.array_equal(q0, quad(plan))  # (the second run replays the graph)
		addr = op.precond_addresses()
		ws = plan.workspace_bytes
		K.set_parameters(**new)
		with pytest.raises(ValueError, match="stale"):
			quad(plan)
		with pytest.raises(ValueError, match="stale"):
			op.matmat(V)
		with pytest.raises(ValueError, match="stale"):
			op.inv_sqrt(V)
		op.refresh()
		assert op.precond_addresses() == addr
		q1 = quad(plan)
		K2 = KernelOperator(X, "matern52", **new)
		op2 = eng.DeviceOperator(K2.preconditioned(rank))
		plan2 = eng.LanczosPlan(op2, Pn, 20, 3)
		q2 = quad(plan2)
		base_plan = eng.LanczosPlan(op2.base, Pn, 20, 3)
		extra = ws - base_plan.workspace_bytes
		base_plan.close()
		plan2.close()
		f1, f2 = op.factor(), op2.factor()
		op2.close()
		assert not np.array_equal(q0, q1) and np.array_equal(q1, q2)
		assert all(np.array_equal(f1[k], f2[k]) for k in ("L", "pivots", "G", "eig"))
		## the plan's own scratch (V, the slab partials, G L^T W) is in its workspace figure
		assert extra >= n * 16 * 8, extra
		## the lazy refresh of the Python layer: the cached device operator of a host object follows its base
		from primate_amd.lanczos import _as_device_operator

		Bh = K.preconditioned(rank)
		dop = _as_device_operator(Bh)
		K.set_parameters(noise=5e-3)
		assert _as_device_operator(Bh) is dop
		dop.matmat(V)  # (refreshed: no "stale")
	finally:
		plan.close()
		op.close()


def test_reproducible_and_freed(eng):
	"""Two creations give equal L, pivots and G; two products equal bits; the bytes the operators hold return to their starting value
	after destroy; the Python base object may be dropped while the preconditioned operator lives."""
	c = P.CASES[4]
	gc.collect()
	from primate_amd.lanczos import _as_device_operator

	K = P.operator(c)
	_as_device_operator(K)  # (the base's device operator, which the preconditioned ones borrow: it is not part of the count)
	start = device_bytes()
	X = R.probes(c[0], 33, seed=3)
	ops = [eng.DeviceOperator(K.preconditioned(c[6])) for _ in range(2)]
	try:
		assert device_bytes() > start
		f = [o.factor() for o in ops]
		assert all(np.array_equal(f[0][k], f[1][k]) for k in ("L", "pivots", "G"))
		Y = [o.matmat(X) for o in ops]
		assert np.array_equal(Y[0], Y[1]) and np.array_equal(Y[0], ops[0].matmat(X))
	finally:
		for o in ops:
			o.close()
	assert device_bytes() == start
	Bh = P.operator(c).preconditioned(c[6])
	op = eng.DeviceOperator(Bh)
	del Bh
	gc.collect()
	try:
		assert np.array_equal(op.matmat(X), Y[0])
	finally:
		op.close()


def test_refusals(eng):
	from primate_amd import _capi
	from primate_amd.operators import KernelOperator

	L, ctx = _capi.lib(), eng.default_context()
	msg = lambda: L.slq_last_error().decode()  # noqa: E731
	X = R.points(40, 3, seed=2)
	K = KernelOperator(X, noise=1e-2)
	K0 = KernelOperator(X, noise=0.0)
	K32 = KernelOperator(X.astype(np.float32), noise=1e-2)
	base, base0, base32, dense = eng.DeviceOperator(K), eng.DeviceOperator(K0), eng.DeviceOperator(K32), eng.DeviceOperator(np.eye(40))
	h = C.c_void_p()
	create = lambda b, r=8, tol=0.0: L.slq_kernel_precond_create(ctx._h, b._h, r, tol, C.byref(h))  # noqa: E731
	op = None
	try:
		assert create(dense) == _capi.SLQ_EINVAL and "not a kernel operator" in msg() and "dense" in msg()
		assert create(base32) == _capi.SLQ_EINVAL and "fp32" in msg()
		assert create(base0) == _capi.SLQ_EINVAL and "sigma2 is 0" in msg()
		assert create(base, r=0) == _capi.SLQ_EINVAL and "rank_max = 0" in msg()
		assert create(base, r=257) == _capi.SLQ_EINVAL and "rank_max = 257" in msg()
		assert create(base, tol=-1.0) == _capi.SLQ_EINVAL and "tol" in msg()
		assert h.value is None
		op = eng.DeviceOperator(K.preconditioned(100))
		assert op.info()["rank_max"] == 40  # (clamped to n)
		ls = np.array([0.5])
		assert L.slq_kernel_set_parameters(op._h, _capi.ptr(ls), 1, 1.0, 0.1) == _capi.SLQ_EINVAL and "base operator" in msg()
		assert L.slq_operator_set_parameter(op._h, 1.0) == _capi.SLQ_EINVAL and "slq_kernel_precond_refresh" in msg()
		g = C.c_void_p()
		assert L.slq_kernel_cross_create(ctx._h, op._h, 3, _capi.ptr(X), 3, C.byref(g)) == _capi.SLQ_EINVAL and "kernel_precond" in msg()
		assert L.slq_kernel_grad_create(ctx._h, op._h, C.byref(g)) == _capi.SLQ_EINVAL and "kernel_precond" in msg()
		assert g.value is None
		## the entries of the preconditioner refuse every other kind
		assert L.slq_kernel_precond_refresh(base._h) == _capi.SLQ_EINVAL and "'kernel'" in msg()
		assert L.slq_kernel_precond_info(dense._h, None, None, None, None, None) == _capi.SLQ_EINVAL
		Mx = eng.DeviceMatrix(40, 8, ctx=ctx)
		My = eng.DeviceMatrix(39, 8, ctx=ctx)
		try:
			apply = lambda IN, i0, OUT, o0, b: L.slq_kernel_precond_apply_dmat(op._h, IN._h, i0, OUT._h, o0, b)  # noqa: E731
			assert apply(Mx, 0, Mx, 2, 4) == _capi.SLQ_EINVAL and "overlap" in msg()
			assert apply(Mx, 0, Mx, 0, 4) == _capi.SLQ_EINVAL and "overlap" in msg()
			assert apply(Mx, 0, Mx, 4, 4) == _capi.SLQ_OK
			assert apply(Mx, 0, Mx, 4, 0) == _capi.SLQ_EINVAL and apply(Mx, 6, Mx, 0, 4) == _capi.SLQ_EINVAL
			assert apply(Mx, 0, My, 0, 4) == _capi.SLQ_EINVAL and "rows" in msg()
		finally:
			Mx.close()
			My.close()
		buf = np.zeros((40, 2), order="F")
		assert L.slq_kernel_precond_apply(op._h, _capi.ptr(buf), 39, _capi.ptr(buf), 40, 2) == _capi.SLQ_EINVAL
		assert L.slq_kernel_precond_apply(op._h, _capi.ptr(buf), 40, _capi.ptr(buf), 40, 0) == _capi.SLQ_EINVAL
		with pytest.raises(ValueError, match="preconditioned kernel operator"):
			base.info()
	finally:
		if op is not None:
			op.close()
		for o in (base, base0, base32, dense):
			o.close()
