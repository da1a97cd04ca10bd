"""The device Toeplitz operator on the GPU: products against the long-double model of tests/_toeplitz_ref.py at every
pass structure, pair isolation, Lanczos against the dense operator, the closed-form log-determinant of the KMS matrix, the other plan
kinds through their unedited drivers, live updates under graph replay, the refusals and the device memory.

Worst device error over the product cases, as a fraction of the bar (measured on an MI355X; profiles/toeplitz_products.txt): one kernel
0.24 (fp64) / 0.20 (fp32), three kernels 0.093 / 0.11, five kernels 0.068 / 0.074."""

import ctypes as C

import numpy as np
import pytest

import _toeplitz_ref as R

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def _op(eng, c, r, dtype):
	from primate_amd.operators import ToeplitzOperator

	T = ToeplitzOperator(np.asarray(c, dtype=np.float64), None if r is None else np.asarray(r, dtype=np.float64), dtype=dtype)
	return T, eng.DeviceOperator(T)


def _live_bytes():
	from primate_amd import _capi

	v = C.c_int64(0)
	_capi.check(_capi.lib().slq_debug_operator_device_bytes(C.byref(v)))
	return int(v.value)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "general"])
@pytest.mark.parametrize("n", R.sizes())
def test_products_against_the_model(eng, n, symmetric, dtype):
	c, r = R.values(n, symmetric, dtype)
	T, op = _op(eng, c, r, dtype)
	assert op.kind == "toeplitz" and op.nnz == 2 * n - 1
	worst = 0.0
	try:
		for b in R.BS:
			_, _, X, Y, bars = R.case_data(n, b, symmetric, dtype)
			got = op.matmat(X)
			ratio = R.ratios(got, Y, bars)
			print(f"[toeplitz] n={n} b={b} levels={R.plan(n, dtype)['levels']} {np.dtype(dtype).name} symmetric={symmetric} worst={ratio.max():.4f} of the bar")
			worst = max(worst, float(ratio.max()))
			assert np.all(np.isfinite(got)) and ratio.max() <= 1.0, f"n={n} b={b}: column {int(np.argmax(ratio))} is at {ratio.max():.3g} of the bar"
	finally:
		op.close()


@pytest.mark.parametrize("case", R.two_panel_cases(), ids=lambda c: f"{c[0]}-{c[1]}-{np.dtype(c[3]).name}")
def test_products_over_two_panels(eng, case):
	"""More columns than a panel holds: the second panel's offsets, its padding mask (an odd count) and the reuse of the one workspace."""
	n, b, symmetric, dtype = case
	c, r, X, Y, bars = R.case_data(*case)
	T, op = _op(eng, c, r, dtype)
	try:
		got = op.matmat(X)
		ratio = R.ratios(got, Y, bars)
		print(f"[toeplitz] n={n} b={b} two panels {np.dtype(dtype).name} worst={ratio.max():.4f} of the bar")
		assert np.all(np.isfinite(got)) and ratio.max() <= 1.0, f"column {int(np.argmax(ratio))} is at {ratio.max():.3g} of the bar"
	finally:
		op.close()
	## the geometry is what the case is for
	Ts, ops = _op(eng, *R.values(n, True, dtype), dtype)
	plan = eng.LanczosPlan(ops, b, 2, 0)
	assert plan.describe()["panels"] == 2
	plan.close()
	ops.close()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
@pytest.mark.parametrize("n", [17, R.structure_sizes()[0] + 1])
def test_pair_isolation(eng, n, dtype):
	"""Even columns random, odd columns zero: the odd outputs stay within the bar (of their pair) and the even ones are right; and the
	roles exchanged."""
	c, r = R.values(n, False, dtype)
	T, op = _op(eng, c, r, dtype)
	try:
		for live in (0, 1):
			X = R.inputs(n, 18, dtype, seed=3 + live).copy(order="F")
			X[:, 1 - live :: 2] = 0
			Y, bars = R.model(c, r, X), R.bar(c, r, X, dtype)
			assert np.all(Y[:, 1 - live :: 2] == 0) and np.all(bars > 0)
			ratio = R.ratios(op.matmat(X), Y, bars)
			assert ratio.max() <= 1.0, f"live columns {live}::2: column {int(np.argmax(ratio))} at {ratio.max():.3g} of the bar"
	finally:
		op.close()


@pytest.mark.parametrize("dtype,tol", [(F64, None), (F32, 3e-4)], ids=["float64", "float32"])
@pytest.mark.parametrize("n", [64, R.structure_sizes()[0] + 1])
def test_lanczos_against_the_dense_operator(eng, n, dtype, tol):
	from scipy.linalg import toeplitz

	from primate_amd.lanczos import lanczos
	from primate_amd.operators import MatrixFunction, ToeplitzOperator

	c = 0.5 ** np.arange(n)
	T, Td = ToeplitzOperator(c, dtype=dtype), toeplitz(c).astype(dtype)
	v = np.random.default_rng(0).standard_normal(n).astype(dtype)
	(a1, b1), (a2, b2) = lanczos(T, v0=v, deg=20, orth=5, dtype=dtype), lanczos(Td, v0=v, deg=20, orth=5, dtype=dtype)
	rtol, atol = (1e-9, 1e-11) if tol is None else (tol, tol)
	np.testing.assert_allclose(a1, a2, rtol=rtol, atol=atol)
	np.testing.assert_allclose(b1, b2, rtol=rtol, atol=atol)
	M1, M2 = MatrixFunction(T, fun="log", deg=20, dtype=dtype), MatrixFunction(Td, fun="log", deg=20, dtype=dtype)
	X = np.random.default_rng(1).standard_normal((n, 6)).astype(dtype)
	np.testing.assert_allclose(M1.quad(X), M2.quad(X), rtol=1e-9 if tol is None else tol)


def test_kms_log_determinant_by_hutch():
	"""log det of the KMS matrix is (n - 1) log(1 - rho^2): hutch within 3 of its own standard errors."""
	from primate_amd.operators import MatrixFunction, ToeplitzOperator
	from primate_amd.trace import hutch

	n, rho = 4096, 0.5
	M = MatrixFunction(ToeplitzOperator(rho ** np.arange(n)), "log", deg=30)
	est, info = hutch(M, converge="count", count=256, seed=11, full=True, record=True)
	samples = np.ravel(info.estimator.values)
	se = float(np.std(samples, ddof=1) / np.sqrt(samples.size))
	exact = (n - 1) * np.log(1 - rho * rho)
	print(f"[toeplitz] KMS log det {est:.4f}, exact {exact:.4f}, standard error {se:.4f}")
	assert samples.size == 256 and abs(est - exact) <= 3 * se


def test_other_plan_kinds_through_their_drivers():
	"""n = 300: the recompute and the kept-basis action against eigh, the Chebyshev action within its truncation bound, a KPM density integrating to n."""
	from scipy.linalg import toeplitz

	from primate_amd.chebyshev import ChebyshevFunction, chebyshev_coefficients
	from primate_amd.integrate import spectral_density
	from primate_amd.operators import MatrixFunction, ToeplitzOperator

	n = 300
	c = 0.5 ** np.arange(n)
	T = ToeplitzOperator(c)
	lam, U = np.linalg.eigh(toeplitz(c))
	X = np.random.default_rng(5).standard_normal((n, 7))
	ref = U @ (np.exp(lam)[:, None] * (U.T @ X))
	for basis in ("recompute", "keep"):
		Y = MatrixFunction(T, "exp", deg=40, orth=40, basis=basis) @ X
		assert np.max(np.abs(Y - ref)) <= 1e-9 * np.max(np.abs(ref)), basis
	## Chebyshev action of log on [0.3, 3.1] (the KMS spectrum lies in [1/3, 3]). With per-product error delta |x| the three-term
	## recurrence gives |T_k error| <= k (k + 1) / 2 (2 delta / h + 3 eps) |x| (the U_m(A~) that propagate a step's error have norm <= m + 1),
	## delta = eps log2(L) |t|_1 sqrt2 (the pair of a column has at most sqrt2 times its norm here: compared below), h the half width.
	bounds, deg = (0.3, 3.1), 200
	M = ChebyshevFunction(T, "log", deg=deg, bounds=bounds)
	Yc = M @ X
	refc = U @ (np.log(lam)[:, None] * (U.T @ X))
	long = chebyshev_coefficients("log", 2 * deg + 1, bounds)
	k = np.arange(deg + 1)
	eps, h = 2.0**-53, 0.5 * (bounds[1] - bounds[0])
	xn = np.linalg.norm(X, axis=0)
	pair = np.sqrt(2.0) * np.max(xn)
	delta = eps * np.log2(R.plan(n, F64)["L"]) * (2 * np.sum(c) - c[0])
	bar = np.sum(np.abs(long[deg + 1 :])) * xn + np.sum(np.abs(long[: deg + 1]) * (1 + k * (k + 1) / 2)) * (2 * delta / h + 3 * eps) * pair
	err = np.linalg.norm(Yc - refc, axis=0)
	print(f"[toeplitz] Chebyshev action: error {err.max():.3g}, bound {bar.min():.3g}, result {np.linalg.norm(refc, axis=0).min():.3g}")
	assert np.all(bar <= 1e-9 * np.linalg.norm(refc, axis=0)) and np.all(err <= bar)
	vals, grid = spectral_density(T, bins=400, method="kpm", deg=200, nprobes=64, batch=64, seed=5)
	total = float(np.sum(0.5 * (vals[1:] + vals[:-1]) * np.diff(grid)))
	print(f"[toeplitz] KPM density integrates to {total:.4f} (n = {n})")
	assert abs(total - n) <= 1e-3 * n


@pytest.mark.parametrize("n", [64, R.structure_sizes()[0] + 1])
def test_live_update_under_graph_replay(eng, n, monkeypatch):
	"""A plan runs twice: array_equal (graph replay, determinism). Then set_values on the live operator: the next run is array_equal to
	a fresh operator's on the same probes. The library has no entry that reports a capture: the plan is created under the default
	SLQ_GRAPH (its runs replay captured graphs, as for every kind that is not a callback), and a plan created under SLQ_GRAPH=0, which
	launches every step eagerly, must give the same bits."""
	from primate_amd.operators import ToeplitzOperator

	T = ToeplitzOperator(0.5 ** np.arange(n))
	op = eng.DeviceOperator(T)
	X = np.asfortranarray(np.random.default_rng(2).standard_normal((n, 5)))
	monkeypatch.setenv("SLQ_GRAPH", "0")  # (read when the plan is created)
	eager = eng.LanczosPlan(op, 5, 12, 3)
	monkeypatch.delenv("SLQ_GRAPH")
	plan = eng.LanczosPlan(op, 5, 12, 3)
	eager.set_probes(X)
	eager.run()
	eager_out = (eager.quadrature("log"),) + tuple(eager.tridiag()[:2])
	eager.close()
	runs = []
	for _ in range(2):
		plan.set_probes(X)
		plan.run()
		runs.append((plan.quadrature("log"),) + tuple(plan.tridiag()[:2]))
	for u, v, w in zip(*runs, eager_out):
		assert np.array_equal(u, v) and np.array_equal(u, w)
	T.set_values(0.3 ** np.arange(n))
	assert np.array_equal(op.toeplitz_values()["c"], 0.3 ** np.arange(n)) and op.toeplitz_values()["symmetric"]
	plan.set_probes(X)
	plan.run()
	after = (plan.quadrature("log"),) + tuple(plan.tridiag()[:2])
	fresh_op = eng.DeviceOperator(ToeplitzOperator(0.3 ** np.arange(n)))
	fresh = eng.LanczosPlan(fresh_op, 5, 12, 3)
	fresh.set_probes(X)
	fresh.run()
	want = (fresh.quadrature("log"),) + tuple(fresh.tridiag()[:2])
	for u, v, w in zip(after, want, runs[0]):
		assert np.array_equal(u, v) and not np.array_equal(u, w)
	for obj in (plan, fresh, op, fresh_op):
		obj.close()


def test_symbol_on_the_device_is_the_host_symbol(eng):
	from primate_amd import _capi

	for n, dtype in ((17, F64), (R.structure_sizes()[0] + 1, F32)):
		c, r = R.values(n, False, dtype)
		T, op = _op(eng, c, r, dtype)
		L = R.plan(n, dtype)["L"]
		out = np.empty(L, dtype=np.complex128 if dtype == F64 else np.complex64)
		_capi.check(_capi.lib().slq_debug_toeplitz_symbol(op._h, _capi.ptr(out)))
		e = np.zeros(L)
		e[:n], e[L - n + 1 :] = c, r[:0:-1]
		assert np.max(np.abs(out - np.fft.fft(e))) <= 2 * R.eps_of(dtype) * np.sum(np.abs(e))
		op.close()


def test_refusals(eng):
	from primate_amd import _capi
	from primate_amd.chebyshev import ChebyshevFunction
	from primate_amd.operators import MatrixFunction, ToeplitzOperator

	n = 40
	c, r = R.values(n, False, F64)
	T, op = _op(eng, c, r, F64)
	L = _capi.lib()
	h = C.c_void_p()
	for create in (lambda: L.slq_plan_create(op.ctx._h, op._h, 4, 10, 3, 0, C.byref(h)), lambda: L.slq_plan_create(op.ctx._h, op._h, 4, 10, 3, 1, C.byref(h)),
	               lambda: L.slq_plan_create_recompute(op.ctx._h, op._h, 4, 10, 3, C.byref(h)), lambda: L.slq_plan_create_chebyshev(op.ctx._h, op._h, 4, 10, C.byref(h)),
	               lambda: L.slq_plan_create_chebyshev_action(op.ctx._h, op._h, 4, 10, C.byref(h))):  # fmt: skip
		assert create() == _capi.SLQ_EINVAL and "non-symmetric" in L.slq_last_error().decode()
	with pytest.raises(ValueError, match="non-symmetric"):
		MatrixFunction(T, "log", deg=10).quad(np.ones((n, 2)))
	with pytest.raises(ValueError, match="non-symmetric"):
		ChebyshevFunction(T, "exp", deg=10, bounds=(0.0, 4.0)) @ np.ones((n, 2))
	## a symmetry-changing set, at the library and through the host object
	c64 = np.ascontiguousarray(c, dtype=np.float64)
	assert L.slq_toeplitz_set_values(op._h, _capi.ptr(c64), None, n) == _capi.SLQ_EINVAL and "symmetry" in L.slq_last_error().decode()
	assert L.slq_toeplitz_set_values(op._h, _capi.ptr(c64), _capi.ptr(c64), n - 1) == _capi.SLQ_EINVAL
	with pytest.raises(ValueError, match="no parameter t"):
		op.set_parameter(1.0)
	## nan in c, n above the maximum, a wrong dtype: named
	bad = c64.copy()
	bad[5] = np.nan
	assert L.slq_toeplitz_create(op.ctx._h, 1, n, _capi.ptr(bad), None, C.byref(h)) == _capi.SLQ_EINVAL and "c[5]" in L.slq_last_error().decode()
	assert L.slq_toeplitz_set_values(op._h, _capi.ptr(c64), _capi.ptr(bad), n) == _capi.SLQ_EINVAL and "r[5]" in L.slq_last_error().decode()
	too_many = R.plan(1, F64)["max_n"] + 1
	assert L.slq_toeplitz_create(op.ctx._h, 1, too_many, _capi.ptr(c64), None, C.byref(h)) == _capi.SLQ_EINVAL and "maximum" in L.slq_last_error().decode()
	assert L.slq_toeplitz_create(op.ctx._h, 1, 0, _capi.ptr(c64), None, C.byref(h)) == _capi.SLQ_EINVAL
	assert L.slq_toeplitz_create(op.ctx._h, 5, n, _capi.ptr(c64), None, C.byref(h)) == _capi.SLQ_EINVAL
	## the rounded values come back, and the gp entries keep refusing what is not a kernel operator
	got = op.toeplitz_values()
	assert np.array_equal(got["c"], c) and np.array_equal(got["r"], r) and not got["symmetric"]
	op.close()
	from primate_amd import gp

	with pytest.raises((ValueError, TypeError)):
		gp.logdet(ToeplitzOperator(0.5 ** np.arange(n)))


def test_device_memory_returns(eng):
	start = _live_bytes()
	for n, dtype in ((64, F32), (R.structure_sizes()[0] + 1, F64), (R.structure_sizes()[1][-1], F64)):
		c, r = R.values(n, True, dtype)
		T, op = _op(eng, c, r, dtype)
		assert _live_bytes() > start
		op.matmat(R.inputs(n, 3, dtype))
		op.close()
		assert _live_bytes() == start
