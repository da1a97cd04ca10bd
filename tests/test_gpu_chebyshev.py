"""Chebyshev moments on the device (slq_plan_create_chebyshev, engine.ChebyshevPlan, primate_amd.chebyshev): the moments on
every path against the NumPy yardstick tests/_cheb_ref.py (validated on the CPU by tests/test_cheb_cpu.py), past the Lanczos
cap against the exact sine-basis formula, exactness against a Gauss rule, a log-determinant, the `outside` rule, the density
and the plan-kind guards. Every test needs a real MI355X (`-m gpu`).

The rounding rule of the moments (`_cheb_ref.rounding_bar`): 8x the deviation of the NumPy restatement carried in the
operator's dtype from the fp64 yardstick, maximised over k and computed here - not a stored number; the 8 is for the device's
other summation order over blocks and waves - and never below (k + 1) eps_F mu_0."""

import ctypes as C

import numpy as np
import pytest

from _action_check import dense_spd, random_spd_graph
from _cheb_ref import center_halfwidth, grid_laplacian, grid_laplacian_eig, moments_eig, moments_recurrence, rounding_bar

pytestmark = pytest.mark.gpu
NSTEPS_MAX = 9


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


_HOST, _REF = {}, {}


def host_matrix(kind, dtype):
	key = (kind, np.dtype(dtype).name)
	if key not in _HOST:
		if kind == "grid40":
			_HOST[key] = grid_laplacian(40, 37, dtype)
		elif kind == "grid70":
			_HOST[key] = grid_laplacian(70, 67, dtype)
		elif kind == "graph":
			_HOST[key] = random_spd_graph(20000, 16.0, seed=11, dtype=dtype)
		else:
			_HOST[key] = dense_spd(640, seed=5, dtype=dtype)
	return _HOST[key]


def make_operator(eng, kind, dtype):
	"""(host matrix, DeviceOperator, keep-alive): the matrices as they are, a host callback and a TorchOperator over the dense one."""
	if kind == "callback":
		from scipy.sparse.linalg import aslinearoperator

		A = host_matrix("dense", dtype)
		return A, eng.DeviceOperator(aslinearoperator(A)), None
	if kind == "torch":
		import torch

		from primate_amd.operators import TorchOperator

		A = host_matrix("dense", dtype)
		At = torch.tensor(np.ascontiguousarray(A), device="cuda")
		return A, eng.DeviceOperator(TorchOperator(lambda X: At @ X, A.shape[0], dtype=dtype)), At
	A = host_matrix(kind, dtype)
	return A, eng.DeviceOperator(A), None


def bounds_of(kind, dtype):
	from primate_amd.chebyshev import spectral_bounds

	return spectral_bounds(host_matrix("dense" if kind in ("callback", "torch") else kind, dtype), "gershgorin")


def probes_of(n, P, dtype, seed):
	return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, P)), dtype=dtype)


def reference(kind, dtype, P):
	"""(Z, mu64, bar) for the 2 * NSTEPS_MAX + 1 moments of a case, computed once and shared by its step counts: a shorter run's
	moments are the prefix (the direct recurrence has no look-ahead)."""
	key = (kind, np.dtype(dtype).name, P)
	if key not in _REF:
		A = host_matrix("dense" if kind in ("callback", "torch") else kind, dtype)
		Z = probes_of(A.shape[0], P, dtype, 1000 + P)
		b = bounds_of(kind, dtype)
		K = 2 * NSTEPS_MAX + 1
		mu64 = moments_recurrence(A, Z, K, b, np.float64)
		muF = mu64 if np.dtype(dtype) == np.float64 else moments_recurrence(A, Z, K, b, dtype)
		_REF[key] = (Z, mu64, rounding_bar(mu64, muF, float(np.finfo(dtype).eps)))
	return _REF[key]


## (operator, dtype, P, SLQ_TILES, expected describe() entries)
CASES = [
	("grid40", np.float64, 3, None, dict(sequence="fused", tiles=0, panel_width=16, panels=1)),
	("grid40", np.float64, 20, None, dict(sequence="fused", tiles=0, panel_width=32, panels=1)),
	("grid40", np.float64, 130, None, dict(sequence="fused", tiles=0, panel_width=128, panels=2)),
	("grid70", np.float64, 128, "2", dict(sequence="fused", tiles=2, panel_width=128, panels=1)),
	("grid70", np.float64, 40, "2", dict(sequence="fused", tiles=2, panel_width=64, panels=1)),
	("grid70", np.float64, 20, "2", dict(sequence="fused", tiles=2, panel_width=32, panels=1)),
	("grid70", np.float32, 130, "2", dict(sequence="fused", tiles=2, panel_width=256, panels=1)),
	("graph", np.float64, 32, None, dict(sequence="sweeps", tiles=0, dense_kernel=0)),
	("dense", np.float64, 32, None, dict(sequence="sweeps", dense_kernel=(2, 3, 4))),
	("dense", np.float32, 256, None, dict(sequence="sweeps", dense_kernel=(5,))),
	("callback", np.float64, 5, None, dict(sequence="sweeps", dense_kernel=0)),
	("torch", np.float64, 32, None, dict(sequence="sweeps", dense_kernel=0)),
]  # fmt: skip


def _case_id(c):
	return f"{c[0]}-{np.dtype(c[1]).name}-P{c[2]}-tiles{c[3]}"


@pytest.mark.parametrize("nsteps", [1, 2, NSTEPS_MAX])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_moments_on_every_path(eng, monkeypatch, case, nsteps):
	"""Steps 1 (mu_0 .. mu_2 alone), 2 and 9 (both slot parities, the no-store last step) on the generic passes, the ring-fed
	passes (k_csr_ring_pass at 128 columns, k_ring_pass on merged tiles and in fp32), the CSR sweeps and the dense product with
	k_cheb_axpy, and the unfused operators with k_cheb_3term; describe() says which path the plan took. k = 0 and 1 are the
	checks of mu_0 against |z|^2 and of mu_1 against z . A~ z."""
	kind, dtype, P, tiles, expect = case
	if tiles is not None:
		monkeypatch.setenv("SLQ_TILES", tiles)
	A, op, keep_alive = make_operator(eng, kind, dtype)
	Z, mu64, bar = reference(kind, dtype, P)
	K = 2 * nsteps + 1
	plan = eng.ChebyshevPlan(op, P, nsteps)
	try:
		d = plan.describe()
		for k, v in expect.items():
			assert (d[k] in v) if isinstance(v, tuple) else (d[k] == v), (k, d)
		assert d["ring_slots"] == 2
		plan.set_probes(Z)
		plan.run(bounds_of(kind, dtype))
		mu, out = plan.moments(return_outside=True)
		assert mu.shape == (P, K) and not out.any()
		err = np.abs(mu - mu64[:, :K])
		worst = float(np.max(err / bar[:, :K]))
		excess = float(np.max(np.abs(mu) / mu[:, :1] - 1.0))
		print(f"{_case_id(case)} steps {nsteps}: max err / bar {worst:.3f}, max |mu_k| / mu_0 - 1 = {excess:.3e}")
		assert np.all(err <= bar[:, :K]), worst
		# identical runs give identical bits
		plan.set_probes(Z)
		plan.run(bounds_of(kind, dtype))
		assert np.array_equal(plan.moments(), mu)
	finally:
		plan.close()
		op.close()


def test_past_the_lanczos_cap(eng):
	"""700 steps - 1401 moments, where a Lanczos plan stops at 512 - on the 40 x 37 grid against the sine-basis eigen-formula,
	which is exact at any k; the same rule with the fp64 restatement's own deviation from the exact moments."""
	m1, m2, P, nsteps = 40, 37, 20, 700
	A = host_matrix("grid40", np.float64)
	op = eng.DeviceOperator(A)
	Z = probes_of(A.shape[0], P, np.float64, 77)
	b = bounds_of("grid40", np.float64)
	K = 2 * nsteps + 1
	lam, UtZ = grid_laplacian_eig(m1, m2, Z)
	exact = moments_eig(lam, UtZ, K, b)
	bar = rounding_bar(exact, moments_recurrence(A, Z, K, b), float(np.finfo(np.float64).eps))
	with pytest.raises(ValueError):
		eng.LanczosPlan(op, P, nsteps, 0)
	plan = eng.ChebyshevPlan(op, P, nsteps)
	try:
		plan.set_probes(Z)
		plan.run(b)
		mu, out = plan.moments(return_outside=True)
		err = np.abs(mu - exact)
		print(f"700 steps: max err / bar {float(np.max(err / bar)):.3f}, max |mu_k| / mu_0 - 1 = {float(np.max(np.abs(mu) / mu[:, :1] - 1.0)):.3e}")
		assert not out.any() and np.all(err <= bar), float(np.max(err / bar))
	finally:
		plan.close()
		op.close()


def test_exact_for_polynomials_like_the_gauss_rule(eng):
	"""f a polynomial of degree 2M - 1 from random Chebyshev coefficients: sum_k c_k mu_k over M steps and the M-point Gauss rule
	of a fully reorthogonalised Lanczos run are both exact for it. Bar: the Chebyshev side's sum_k |c_k| bar_k (the moments'
	rule) plus the Gauss side's sum_k |c_k| (k + 1)^2 eps mu_0 - its nodes carry perturbations of eps h, and |T_k'| <= k^2."""
	from numpy.polynomial import chebyshev as npc

	M, P = 8, 20
	A = host_matrix("grid40", np.float64)
	op = eng.DeviceOperator(A)
	Z = probes_of(A.shape[0], P, np.float64, 31)
	b = bounds_of("grid40", np.float64)
	c, h = center_halfwidth(b)
	coef = np.random.default_rng(3).standard_normal(2 * M)
	eps = float(np.finfo(np.float64).eps)
	cheb, lan = eng.ChebyshevPlan(op, P, M), eng.LanczosPlan(op, P, M, M)
	try:
		cheb.set_probes(Z)
		cheb.run(b)
		got, stage = cheb.moment_sum(coef, return_stage=True)
		lan.set_probes(Z)
		lan.run()
		ref = lan.quadrature(lambda x: npc.chebval((x - c) / h, coef))
		mu = cheb.moments()
		assert np.allclose(got, mu[:, : 2 * M] @ coef, rtol=0, atol=2 * M * eps * np.max(np.abs(mu[:, : 2 * M]) @ np.abs(coef)))
		assert stage[3] == P and stage[2] == 0.0 and np.isclose(stage[0], got.sum(), rtol=1e-13) and np.isclose(stage[1], (got**2).sum(), rtol=1e-13)
		k = np.arange(2 * M)
		mu0 = np.sum(Z * Z, axis=0)
		bar = np.abs(coef) @ ((k + 1) * eps) * mu0 + np.abs(coef) @ ((k + 1) ** 2 * eps) * mu0
		print(f"exactness: max err / bar {float(np.max(np.abs(got - ref) / bar)):.3f}")
		assert np.all(np.abs(got - ref) <= bar), float(np.max(np.abs(got - ref) / bar))
	finally:
		cheb.close()
		lan.close()
		op.close()


def test_logdet_quadratic_forms_and_hutch(eng):
	"""z^T log(A) z on the shifted 24^2 Laplacian against the dense value: |error| <= sum_{k > 2M} |c_k| mu_0 (the truncated
	series; the tail from 4x as many coefficients) + sum_k |c_k| bar_k (the moments' rounding rule); and hutch() over a
	ChebyshevFunction is the mean of those forms over its host probe stream."""
	import scipy.sparse as sp

	from primate_amd.chebyshev import ChebyshevFunction, chebyshev_coefficients, spectral_bounds
	from primate_amd.random import isotropic
	from primate_amd.trace import hutch

	m, deg, P = 24, 80, 64
	A = (grid_laplacian(m, m) + sp.identity(m * m)).tocsr()
	lam, U = np.linalg.eigh(A.toarray())
	b = spectral_bounds(A)
	assert b[0] <= lam[0] and lam[-1] <= b[1] and b[0] > 0
	Z = isotropic(pdf="rademacher", seed=np.random.default_rng(7))(size=(m * m, P))
	truth = np.sum((U.T @ Z) ** 2 * np.log(lam)[:, None], axis=0)
	c4 = chebyshev_coefficients("log", 4 * (deg + 1), b)
	coef = chebyshev_coefficients("log", deg + 1, b)
	mu0 = np.sum(Z * Z, axis=0)
	k = np.arange(deg + 1)
	eps = float(np.finfo(np.float64).eps)
	bar = np.sum(np.abs(c4[deg + 1 :])) * mu0 + np.abs(coef) @ ((k + 1) * eps) * mu0
	M = ChebyshevFunction(A, "log", deg=deg)
	try:
		got = M.quad(Z)
		assert M.bounds == b
		print(f"logdet: max err / bar {float(np.max(np.abs(got - truth) / bar)):.3f}, rel err {float(np.max(np.abs(got / truth - 1))):.2e}")
		assert np.all(np.abs(got - truth) <= bar)
		est = hutch(M, converge="count", count=P, seed=7)
		assert est == pytest.approx(float(np.mean(got)), rel=1e-12)  # (the estimator's running mean against one sum)
		assert abs(est - float(np.mean(truth))) <= float(np.mean(bar))
		dev = M.quad_generated(16, "rademacher", seed=3)
		assert dev.shape == (16,) and np.all(np.abs(dev / np.mean(truth) - 1) < 0.2)
	finally:
		M.close()


def test_bounds_that_miss_the_spectrum_raise_the_flag(eng):
	"""A half-width of 0.8 of the true one: every probe's flag goes up, moment_sum refuses, the moments still come back
	finite, the plan runs again correctly with good bounds, and ChebyshevFunction turns the flag into ValueError."""
	from primate_amd.chebyshev import ChebyshevFunction

	kind, P, nsteps = "grid40", 20, NSTEPS_MAX
	A = host_matrix(kind, np.float64)
	op = eng.DeviceOperator(A)
	Z, mu64, bar = reference(kind, np.float64, P)
	a, b = bounds_of(kind, np.float64)
	c, h = center_halfwidth((a, b))
	short = (c - 0.8 * h, c + 0.8 * h)
	plan = eng.ChebyshevPlan(op, P, nsteps)
	try:
		plan.set_probes(Z)
		plan.run(short)
		mu, out = plan.moments(return_outside=True)
		assert out.all() and np.all(np.isfinite(mu))
		with pytest.raises(ValueError, match="bounds"):
			plan.moment_sum(np.ones(3))
		acc = eng.DensityAccumulator("chebyshev", np.linspace(short[0], short[1], 9)[1:-1], ctx=op.ctx)
		with pytest.raises(ValueError, match="bounds"):
			acc.update(plan)
		acc.close()
		plan.set_probes(Z)
		plan.run((a, b))
		mu, out = plan.moments(return_outside=True)
		assert not out.any() and np.all(np.abs(mu - mu64) <= bar)
		assert np.allclose(plan.moment_sum(np.ones(3)), mu[:, :3].sum(axis=1), rtol=1e-14)
		M = ChebyshevFunction(A, "exp", deg=2 * nsteps, bounds=short)
		with pytest.raises(ValueError, match="not inside bounds"):
			M.quad(Z)
		M.close()
	finally:
		plan.close()
		op.close()


def test_spectral_bounds_contain_the_spectrum_of_every_test_operator(eng):
	from scipy.sparse.linalg import aslinearoperator, eigsh

	from primate_amd.chebyshev import spectral_bounds

	for kind in ("grid40", "grid70"):
		m1, m2 = (40, 37) if kind == "grid40" else (70, 67)
		lam, _ = grid_laplacian_eig(m1, m2, np.zeros((m1 * m2, 1)))
		a, b = spectral_bounds(host_matrix(kind, np.float64))
		assert a <= lam.min() and lam.max() <= b
	G = host_matrix("graph", np.float64)
	a, b = spectral_bounds(G)
	top = float(eigsh(G, k=1, which="LA", return_eigenvectors=False)[0])
	assert a <= 1.0 and top <= b  # (a graph Laplacian + I: nothing below 1)
	D = host_matrix("dense", np.float64)
	ev = np.linalg.eigvalsh(D)
	a, b = spectral_bounds(D)
	assert a <= ev[0] and ev[-1] <= b
	# operators known by their product only: the Lanczos estimate (extreme Ritz values -/+ residuals, widened)
	a, b = spectral_bounds(aslinearoperator(D), seed=1)
	assert a <= ev[0] and ev[-1] <= b, (a, b, ev[0], ev[-1])
	with pytest.raises(ValueError):
		spectral_bounds(aslinearoperator(D), method="gershgorin")


def _trapezoid(y, x):
	return float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(x)))


def _density_numpy(mu, g, grid, bounds):
	"""rho[p, x] by the cos(k arccos x~) form and by the forward recurrence, and the floor 4 K eps sum |g_k mu_k| / (pi h sqrt(1 - x~^2))."""
	c, h = center_halfwidth(bounds)
	x = (grid - c) / h
	K = mu.shape[1]
	gm = mu * g[None, :]
	gm[:, 1:] *= 2.0
	den = np.pi * h * np.sqrt(1.0 - x * x)
	cosf = (gm @ np.cos(np.outer(np.arange(K), np.arccos(x)))) / den
	T = np.zeros((K, x.size))
	T[0] = 1.0
	if K > 1:
		T[1] = x
	for k in range(2, K):
		T[k] = 2.0 * x * T[k - 1] - T[k - 2]
	rec = (gm @ T) / den
	floor = 4.0 * K * np.finfo(float).eps * np.sum(np.abs(gm), axis=1)[:, None] / den[None, :]
	return cosf, rec, floor


def test_density_from_moments(eng):
	"""P = 20, 41 moments, G = 65 on the 40 x 37 grid. Undamped: mean and M2 equal NumPy's evaluation of the returned moments by
	the cos(k arccos x~) form, at 8x NumPy's own spread between that form and the recurrence form, floored at
	4 K eps sum |g_k mu_k| / (pi h sqrt(1 - x~^2)). Jackson: every per-probe value >= -(that floor) - the kernel is positive -
	and the trapezoid integral over a grid spanning the bounds is mu_0 up to the grid's own quadrature error, which the same
	formula gives on the CPU. spectral_density(method="kpm") returns the accumulator's mean on its grid."""
	from primate_amd.chebyshev import damping_factors, density_grid
	from primate_amd.integrate import spectral_density
	from primate_amd.random import isotropic

	P, nsteps, G = 20, 20, 65
	K = 2 * nsteps + 1
	A = host_matrix("grid40", np.float64)
	n = A.shape[0]
	op = eng.DeviceOperator(A)
	b = bounds_of("grid40", np.float64)
	grid = density_grid(G, *b)
	Z = isotropic(pdf="rademacher", seed=np.random.default_rng(5))(size=(n, P))
	plan, one = eng.ChebyshevPlan(op, P, nsteps), eng.ChebyshevPlan(op, 1, nsteps)
	try:
		plan.set_probes(Z)
		plan.run(b)
		mu = plan.moments()
		# undamped
		acc = eng.DensityAccumulator("chebyshev", grid, ctx=op.ctx)
		acc.update(plan, damping=None)
		mean, m2, outside, cnt = acc.get()
		acc.close()
		cosf, rec, floor = _density_numpy(mu, np.ones(K), grid, b)
		e = np.maximum(8.0 * np.abs(cosf - rec), floor)  # per probe and grid point
		assert cnt == P and np.all(outside == 0)
		me = e.mean(axis=0)
		assert np.all(np.abs(mean - cosf.mean(axis=0)) <= me), float(np.max(np.abs(mean - cosf.mean(axis=0)) / me))
		dlt = np.abs(cosf - cosf.mean(axis=0))
		ep = e + me
		m2_bar = np.sum(2.0 * dlt * ep + ep * ep, axis=0)
		m2_np = np.sum((cosf - cosf.mean(axis=0)) ** 2, axis=0)
		assert np.all(np.abs(m2 - m2_np) <= m2_bar), float(np.max(np.abs(m2 - m2_np) / m2_bar))
		# Jackson: positivity per probe (one-probe plans: the accumulator's mean after one update IS the probe's value)
		g = damping_factors("jackson", K)
		cosj, recj, floorj = _density_numpy(mu, g, grid, b)
		for p in range(P):
			one.set_probes(Z[:, p])
			one.run(b)
			acc = eng.DensityAccumulator("chebyshev", grid, ctx=op.ctx)
			acc.update(one, damping=g)
			val = acc.get()[0]
			acc.close()
			assert np.all(val >= -floorj[p]), (p, float(val.min()))
			assert np.all(np.abs(val - cosj[p]) <= np.maximum(8.0 * np.abs(cosj[p] - recj[p]), floorj[p]))
		# normalisation: integral over the bounds = mu_0 (= n for Rademacher probes)
		acc = eng.DensityAccumulator("chebyshev", grid, ctx=op.ctx)
		acc.update(plan, damping=g)
		meanj = acc.get()[0]
		acc.close()
		quad_err = abs(_trapezoid(cosj.mean(axis=0), grid) - n)  # the grid's own error, from the same formula
		w = np.gradient(grid)
		assert abs(_trapezoid(meanj, grid) - n) <= quad_err + float(np.sum(w * np.maximum(8.0 * np.abs(cosj - recj), floorj).mean(axis=0)))
		print(f"density: trapezoid integral {_trapezoid(meanj, grid):.6f} of {n}, grid error {quad_err:.3e}")
		# the driver
		vals, dgrid, info = spectral_density(A, bins=G, method="kpm", deg=2 * nsteps, damping="jackson", nprobes=P, batch=P, seed=5, full=True)
		assert np.array_equal(dgrid, grid) and info["interval"] == b and info["nprobes"] == P
		assert np.array_equal(vals, meanj)
		# a grid point on the boundary is refused, and so is the Lanczos update on this kind
		edge = eng.DensityAccumulator("chebyshev", np.array([b[0], 0.5 * (b[0] + b[1])]), ctx=op.ctx)
		with pytest.raises(ValueError, match="strictly inside"):
			edge.update(plan)
		edge.close()
	finally:
		plan.close()
		one.close()
		op.close()


def test_plan_kinds_refuse_each_others_entries(eng):
	"""Every Lanczos accessor on a Chebyshev plan and every Chebyshev entry on a Lanczos plan is SLQ_EINVAL; both plans stay usable."""
	from primate_amd import _capi

	L = _capi.lib()
	A = host_matrix("grid40", np.float64)
	n, P = A.shape[0], 4
	op = eng.DeviceOperator(A)
	Z = probes_of(n, P, np.float64, 9)
	b = bounds_of("grid40", np.float64)
	cheb, lan, keep = eng.ChebyshevPlan(op, P, 3), eng.LanczosPlan(op, P, 6, 3), eng.LanczosPlan(op, P, 6, 3, basis="keep")
	diag = eng.DiagAccumulator(n, ctx=op.ctx)
	dens_l = eng.DensityAccumulator("gaussian", np.linspace(0.5, 7.5, 8), bw=0.3, ctx=op.ctx)
	dens_c = eng.DensityAccumulator("chebyshev", np.linspace(0.5, 7.5, 8), ctx=op.ctx)
	try:
		for pl in (cheb, lan, keep):
			pl.set_probes(Z)
		cheb.run(b)
		lan.run()
		keep.run()
		mu = cheb.moments()
		q = lan.quadrature("exp", t=-0.1)
		buf, ibuf = np.zeros((P, 8)), np.zeros(P, dtype=np.int32)
		Y = np.zeros((n, P), order="F")
		h = cheb._h
		lanczos_entries = [
			lambda: L.slq_plan_run(h, 1e-8),
			lambda: L.slq_plan_run_steps(h, 1e-8, 2),
			lambda: L.slq_plan_get_tridiag(h, buf.ctypes.data, buf.ctypes.data, ibuf.ctypes.data),
			lambda: L.slq_plan_quadrature(h, 0, None, buf.ctypes.data, None, None),
			lambda: L.slq_plan_quadrature_at(h, 1, 0, 0.0, 0, None, buf.ctypes.data, None, None, None),
			lambda: L.slq_plan_get_basis(h, 0, Y.ctypes.data, n),
			lambda: L.slq_plan_fun_action(h, 0, None, Y.ctypes.data, n),
			lambda: L.slq_diag_update(diag._h, h, 0, None),
			lambda: L.slq_density_update(dens_l._h, h),
			lambda: L.slq_density_update(dens_c._h, h),
			lambda: L.slq_density_update(dens_c._h, lan._h),
		]
		for i, call in enumerate(lanczos_entries):
			assert call() == _capi.SLQ_EINVAL, i
		with pytest.raises(ValueError):
			cheb.quadrature("exp")
		one = np.ones(3)
		for pl in (lan, keep):
			cheb_entries = [
				lambda: L.slq_plan_run_chebyshev(pl._h, 4.0, 4.0, 0.0),
				lambda: L.slq_plan_get_moments(pl._h, buf.ctypes.data, ibuf.ctypes.data),
				lambda: L.slq_plan_moment_sum(pl._h, 3, one.ctypes.data, buf.ctypes.data, None),
				lambda: L.slq_density_update_moments(dens_c._h, pl._h, 3, None),
			]
			for i, call in enumerate(cheb_entries):
				assert call() == _capi.SLQ_EINVAL, i
		assert L.slq_density_update_moments(dens_l._h, cheb._h, 3, None) == _capi.SLQ_EINVAL
		# nothing was disturbed
		assert np.array_equal(cheb.moments(), mu) and np.array_equal(lan.quadrature("exp", t=-0.1), q)
		assert dens_c.get()[3] == 0 and dens_l.get()[3] == 0
		dens_c.update(cheb)
		dens_l.update(lan)
		assert dens_c.get()[3] == P and dens_l.get()[3] == P
		cheb.set_probes(Z)
		cheb.run(b)
		assert np.array_equal(cheb.moments(), mu)
		assert keep.fun_action("exp", t=-0.1).shape == (n, P)
		# creation: the step count has its own bound
		for bad in (0, 16385):
			with pytest.raises(ValueError):
				eng.ChebyshevPlan(op, P, bad)
		big = eng.ChebyshevPlan(op, 1, 16384)
		assert big.describe()["ring_slots"] == 2 and big.workspace_bytes < 64 << 20
		big.close()
	finally:
		for x in (cheb, lan, keep, diag, dens_l, dens_c):
			x.close()
		op.close()
