"""The Chebyshev action Y = sum_k c_k T_k(A~) X on the device (slq_plan_create_chebyshev_action, engine.ChebyshevPlan(action=True),
ChebyshevFunction @ X) against the NumPy yardstick tests/_cheb_action_ref.py (validated on the CPU by
tests/test_cheb_action_cpu.py). Every test needs a real MI355X (`-m gpu`).

The rule, per column i: err_i = ||Y_dev - Y_ld||_2 <= bar_i = max(8 D_i, B_i), with Y_ld the long-double restatement,
D_i = ||Y_F - Y_ld||_2 the deviation of the restatement carried in the operator's dtype F (computed here, not a stored number;
the 8 is for the device's other summation order) and B_i = eps_F sum_k (k + 1) |c_k| ||z_i||_2."""

import ctypes as C

import numpy as np
import pytest

from _action_check import dense_spd, random_spd_graph
from _cheb_action_ref import action_bar, action_eig, action_recurrence, action_recurrence_ld, coefficient_weight, col_norms, jackson_step_coefficients
from _cheb_ref import center_halfwidth, grid_laplacian

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def acc_cols():
	from primate_amd import _capi

	n, S, K = C.c_int(), C.c_int(), C.c_int()
	assert _capi.lib().slq_debug_cheb_action_schedule(1, None, None, 0, C.byref(n), C.byref(S), C.byref(K)) == _capi.SLQ_OK
	return K.value


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


def exp_coefficients(nsteps, bounds):
	from primate_amd.chebyshev import chebyshev_coefficients

	return chebyshev_coefficients("exp", nsteps + 1, bounds, t=-1.0)


def yardstick(A, Z, coefs, bounds, dtype):
	"""[(Y_ld, bar)] for a list of coefficient vectors: the long-double restatement and the rule's bar, one pass per dtype."""
	lds = action_recurrence_ld(A, Z, list(coefs), bounds)
	Fs = action_recurrence(A, Z, list(coefs), bounds, dtype)
	eps = float(np.finfo(dtype).eps)
	return [(yl, action_bar(yl, yf, Z, cf, eps)[0]) for yl, yf, cf in zip(lds, Fs, coefs)]


def check(Y, Yld, bar, what):
	err = col_norms(np.asarray(Y, dtype=np.longdouble) - Yld)
	worst = float(np.max(err / bar))
	print(f"{what}: max err / bar {worst:.3f}")
	assert np.all(np.isfinite(Y)) and np.all(err <= bar), (what, worst)


## (operator, dtype, P, SLQ_TILES, expected describe() entries): the cases of tests/test_gpu_chebyshev.py
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
## the cases that take every step count around a piece's edge
FULL = {("grid40", "float64", 130), ("grid70", "float64", 128), ("graph", "float64", 32), ("dense", "float32", 256)}


def _case_id(c):
	return f"{c[0]}-{np.dtype(c[1]).name}-P{c[2]}-tiles{c[3]}"


def steps_of(case, K):
	full = (case[0], np.dtype(case[1]).name, case[2]) in FULL
	return [1, 2, K - 1, K, K + 1, 2 * K + 1] if full else [1, K + 1]


def reference(case, K):
	"""{nsteps: (coef, Y_ld, bar)} of a case and its probes, computed once for all its step counts (one pass over the w_k)."""
	kind, dtype, P = case[0], case[1], case[2]
	key = (kind, np.dtype(dtype).name, P)
	if key not in _REF:
		A = host_matrix("dense" if kind in ("callback", "torch") else kind, dtype)
		Z = probes_of(A.shape[0], P, dtype, 2000 + P)
		b = bounds_of(kind, dtype)
		steps = steps_of(case, K)
		coefs = [exp_coefficients(s, b) for s in steps]
		_REF[key] = (Z, {s: (cf, yl, bar) for s, cf, (yl, bar) in zip(steps, coefs, yardstick(A, Z, coefs, b, dtype))})
	return _REF[key]


## ---- A. every path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_action_on_every_path(eng, monkeypatch, case):
	"""exp(-x) on the Gershgorin bounds at 1 and K + 1 steps on every path of the moments' tests - the generic passes, the ring-fed
	passes, the CSR sweeps, the dense product, the unfused operators - and at 1, 2, K - 1, K, K + 1, 2 K + 1 (one piece short,
	exactly one, one and a column, two and the last column alone ...) on four of them, panels of 2 included. Per step count:
	the plan describes itself as the moments' plan does but for its ring, every column is within bar, a second identical call
	gives identical bits, and the moments of the action's run equal, bit for bit, those of a plain plan on the same probes."""
	kind, dtype, P, tiles, expect = case
	if tiles is not None:
		monkeypatch.setenv("SLQ_TILES", tiles)
	K = acc_cols()
	A, op, keep_alive = make_operator(eng, kind, dtype)
	Z, ref = reference(case, K)
	b = bounds_of(kind, dtype)
	try:
		for nsteps in steps_of(case, K):
			coef, Yld, bar = ref[nsteps]
			plan, plain = eng.ChebyshevPlan(op, P, nsteps, action=True), eng.ChebyshevPlan(op, P, nsteps)
			try:
				d = plan.describe()
				for k, v in expect.items():
					assert (d[k] in v) if isinstance(v, tuple) else (d[k] == v), (k, d)
				assert d["ring_slots"] == max(2, min(K, nsteps + 1)) and d["acc_cols"] == K
				assert plain.describe()["ring_slots"] == 2 and plain.describe()["acc_cols"] == 0
				plan.set_probes(Z)
				Y = plan.action(b, coef)
				assert Y.shape == (A.shape[0], P) and Y.dtype == np.dtype(dtype) and Y.flags.f_contiguous
				mu, out = plan.moments(return_outside=True)
				assert not out.any()
				check(Y, Yld, bar, f"{_case_id(case)} steps {nsteps}")
				plan.set_probes(Z)
				assert np.array_equal(plan.action(b, coef), Y)
				plain.set_probes(Z)
				plain.run(b)
				assert np.array_equal(plain.moments(), mu)
			finally:
				plan.close()
				plain.close()
	finally:
		op.close()


## ---- B. unit coefficients ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=_case_id)
def test_unit_coefficients(eng, monkeypatch, case):
	"""coef = e_k picks w_k = T_k(A~) Z: e_0 returns Z bit for bit, e_1 is A~ Z, e_K the last column of the first piece and
	e_{K+1} the first of the next."""
	kind, dtype, P, tiles, _ = case
	if tiles is not None:
		monkeypatch.setenv("SLQ_TILES", tiles)
	K = acc_cols()
	nsteps = K + 2
	A, op, _ = make_operator(eng, kind, dtype)
	Z = probes_of(A.shape[0], P, dtype, 7)
	b = bounds_of(kind, dtype)
	units = [0, 1, K, K + 1]
	coefs = [np.eye(nsteps + 1)[k] for k in units]
	plan = eng.ChebyshevPlan(op, P, nsteps, action=True)
	try:
		for k, cf, (Yld, bar) in zip(units, coefs, yardstick(A, Z, coefs, b, dtype)):
			plan.set_probes(Z)
			Y = plan.action(b, cf)
			if k == 0:
				assert np.array_equal(Y, Z)
			check(Y, Yld, bar, f"{_case_id(case)} e_{k}")
	finally:
		plan.close()
		op.close()


## ---- C. zero columns ---------------------------------------------------------------------------------------------------
def test_columns_with_a_zero_coefficient_are_not_read(eng, monkeypatch):
	"""An even polynomial at 2 K + 1 steps: the odd columns are not read - the same bits as with SLQ_ACC_SKIP=0, which reads them
	all - and slq_plan_action_columns counts what was read against what was offered."""
	K = acc_cols()
	nsteps, P = 2 * K + 1, 20
	A = host_matrix("grid40", np.float64)
	Z = probes_of(A.shape[0], P, np.float64, 8)
	b = bounds_of("grid40", np.float64)
	coef = np.random.default_rng(4).standard_normal(nsteps + 1) / (1.0 + np.arange(nsteps + 1))
	coef[1::2] = 0.0
	nonzero = int(np.count_nonzero(coef))
	assert nonzero == K + 1
	op = eng.DeviceOperator(A)
	got = {}
	try:
		for skip in ("1", "0"):
			monkeypatch.setenv("SLQ_ACC_SKIP", skip)
			plan = eng.ChebyshevPlan(op, P, nsteps, action=True)
			try:
				plan.set_probes(Z)
				got[skip] = plan.action(b, coef)
				assert plan.action_columns(reset=True) == ((nonzero if skip == "1" else nsteps + 1), nsteps + 1)
				assert plan.action_columns() == (0, 0)
			finally:
				plan.close()
		assert np.array_equal(got["1"], got["0"])
		(Yld, bar), = yardstick(A, Z, [coef], b, np.float64)
		check(got["1"], Yld, bar, "even polynomial")
	finally:
		op.close()


## ---- D. the action against the moments of the same run ---------------------------------------------------------------
def test_action_agrees_with_the_moments_of_its_run(eng):
	"""z_i . Y_i = sum_k c_k z_i . w_k = sum_{k <= nsteps} c_k mu_ik: the vectors and the moments of ONE run, the moments through
	the doubling identities. Bar: 8 eps mu_i0 sum_k (k + 1) |c_k|."""
	K = acc_cols()
	nsteps, P = K + 1, 20
	A = host_matrix("grid40", np.float64)
	Z = probes_of(A.shape[0], P, np.float64, 12)
	b = bounds_of("grid40", np.float64)
	coef = exp_coefficients(nsteps, b)
	op = eng.DeviceOperator(A)
	plan = eng.ChebyshevPlan(op, P, nsteps, action=True)
	try:
		plan.set_probes(Z)
		Y = plan.action(b, coef)
		mu = plan.moments()
		lhs = np.sum(Z.astype(np.longdouble) * Y.astype(np.longdouble), axis=0)
		rhs = mu[:, : nsteps + 1].astype(np.longdouble) @ coef.astype(np.longdouble)
		bar = 8.0 * np.finfo(np.float64).eps * mu[:, 0] * coefficient_weight(coef)
		err = np.abs((lhs - rhs).astype(np.float64))
		print(f"action against moments: max err / bar {float(np.max(err / bar)):.3f}")
		assert np.all(err <= bar), float(np.max(err / bar))
		# the device's own sum of the same moments
		assert np.allclose(plan.moment_sum(coef), rhs.astype(np.float64), rtol=0, atol=float(np.max(bar)))
	finally:
		plan.close()
		op.close()


## ---- E. outside --------------------------------------------------------------------------------------------------------
def test_bounds_that_miss_the_spectrum_are_refused(eng):
	"""A half-width of 0.8 of the true one: SLQ_EINVAL / ValueError naming the bounds, the caller's array untouched, the flags
	readable, and the plan serves a correct action afterwards."""
	from primate_amd import _capi
	from primate_amd.chebyshev import ChebyshevFunction

	K = acc_cols()
	nsteps, P = K + 1, 20
	A = host_matrix("grid40", np.float64)
	n = A.shape[0]
	Z = probes_of(n, P, np.float64, 13)
	a, b = bounds_of("grid40", np.float64)
	c, h = center_halfwidth((a, b))
	coef = exp_coefficients(nsteps, (a, b))
	op = eng.DeviceOperator(A)
	plan = eng.ChebyshevPlan(op, P, nsteps, action=True)
	try:
		plan.set_probes(Z)
		Y = np.full((n, P), -7.25, order="F")
		rc = _capi.lib().slq_plan_chebyshev_action(plan._h, c, 0.8 * h, 0.0, nsteps + 1, coef.ctypes.data, Y.ctypes.data, n)
		assert rc == _capi.SLQ_EINVAL and b"bounds" in _capi.lib().slq_last_error()
		assert np.all(Y == -7.25)
		plan.set_probes(Z)
		with pytest.raises(ValueError, match="bounds"):
			plan.action((c - 0.8 * h, c + 0.8 * h), coef)
		mu, out = plan.moments(return_outside=True)
		assert out.all() and np.all(np.isfinite(mu))
		D = eng.DeviceMatrix(n, P, ctx=op.ctx)
		D.set(0, Y)
		plan.set_probes(Z)
		with pytest.raises(ValueError, match="bounds"):
			plan.action_into((c - 0.8 * h, c + 0.8 * h), coef, D, 0)
		assert np.all(D.get() == -7.25)
		(Yld, bar), = yardstick(A, Z, [coef], (a, b), np.float64)
		plan.set_probes(Z)
		got = plan.action((a, b), coef)
		check(got, Yld, bar, "after a refused run")
		plan.set_probes(Z)
		plan.action_into((a, b), coef, D, 0)
		assert np.array_equal(D.get(), got)
		D.close()
		M = ChebyshevFunction(A, "exp", deg=nsteps, bounds=(c - 0.8 * h, c + 0.8 * h), t=-1.0)
		with pytest.raises(ValueError, match="not inside bounds"):
			M @ Z
		M.close()
	finally:
		plan.close()
		op.close()


def test_automatic_bounds_are_widened(eng, monkeypatch):
	"""bounds_method="lanczos" - an estimate - with a small margin: where the estimate misses the spectrum the margin doubles and
	the action runs again. The estimate is made to miss here (a Lanczos estimate from a random start misses only by chance): it
	answers 0.9 of the true half-width, so that the second widening (0.04, then 0.08 of the width per side) contains the
	spectrum. The result is within bar of the restatement on the FINAL bounds."""
	from primate_amd import chebyshev

	A = host_matrix("grid40", np.float64)
	Z = probes_of(A.shape[0], 6, np.float64, 14)
	c, h = center_halfwidth(bounds_of("grid40", np.float64))
	asked = []

	def estimate(A_, method="auto", margin=0.01, seed=None):
		asked.append((method, margin))
		return (c - 0.9 * h, c + 0.9 * h)

	monkeypatch.setattr(chebyshev, "spectral_bounds", estimate)
	M = chebyshev.ChebyshevFunction(A, "exp", deg=24, bounds_method="lanczos", margin=0.02, t=-1.0)
	try:
		Y = M @ Z
		assert asked == [("lanczos", 0.02)]
		assert M.bounds == pytest.approx((c - 0.9 * h - 0.08 * 1.8 * h, c + 0.9 * h + 0.08 * 1.8 * h))
		coef = chebyshev.chebyshev_coefficients("exp", 25, M.bounds, t=-1.0)
		(Yld, bar), = yardstick(A, Z, [coef], M.bounds, np.float64)
		check(Y, Yld, bar, "widened bounds")
	finally:
		M.close()


## ---- F. guards -----------------------------------------------------------------------------------------------------------
def test_guards_of_the_c_abi(eng):
	"""Every SLQ_EINVAL of the action entries through the raw ABI, the message naming the cause and the output untouched; the
	Lanczos entries on an action plan; and the Chebyshev entries working on it."""
	from primate_amd import _capi

	L = _capi.lib()
	A = host_matrix("grid40", np.float64)
	n, P, nsteps = A.shape[0], 4, 5
	Z = probes_of(n, P, np.float64, 15)
	a, b = bounds_of("grid40", np.float64)
	c, h = center_halfwidth((a, b))
	coef = exp_coefficients(nsteps, (a, b))
	op = eng.DeviceOperator(A)
	act, plain, lan = eng.ChebyshevPlan(op, P, nsteps, action=True), eng.ChebyshevPlan(op, P, nsteps), eng.LanczosPlan(op, P, 6, 3)
	D = eng.DeviceMatrix(n, P, ctx=op.ctx)
	Y = np.full((n, P), 3.5, order="F")
	D.set(0, Y)
	bad = coef.copy()
	bad[2] = np.nan
	inf = coef.copy()
	inf[0] = np.inf

	def host(plan, cf=coef, ncoef=nsteps + 1, ldy=n):
		return L.slq_plan_chebyshev_action(plan._h, c, h, 0.0, ncoef, cf.ctypes.data, Y.ctypes.data, ldy)

	def dev(plan, cf=coef, ncoef=nsteps + 1, o0=0):
		return L.slq_plan_chebyshev_action_dmat(plan._h, c, h, 0.0, ncoef, cf.ctypes.data, D._h, o0)

	def refused(rc, word):
		msg = L.slq_last_error().decode()
		assert rc == _capi.SLQ_EINVAL and word in msg, (rc, word, msg)
		assert np.all(Y == 3.5) and np.all(D.get() == 3.5)

	try:
		refused(host(act), "probes")  # no probes yet
		refused(dev(act), "probes")
		for pl in (act, plain, lan):
			pl.set_probes(Z)
		for call in (host, dev):
			refused(call(plain), "action plan")
			refused(call(lan), "Chebyshev plan")
			refused(call(act, ncoef=nsteps), "ncoef")
			refused(call(act, ncoef=nsteps + 2), "ncoef")
			refused(call(act, cf=bad), "finite")
			refused(call(act, cf=inf), "finite")
		refused(host(act, ldy=n - 1), "ldy")
		refused(dev(act, o0=1), "slq_plan_chebyshev_action_dmat")  # columns [1, 1 + P) of a P-column matrix
		refused(L.slq_plan_chebyshev_action(act._h, c, 0.0, 0.0, nsteps + 1, coef.ctypes.data, Y.ctypes.data, n), "halfwidth")
		# sphere probes drawn on the device: the panel holds the normal draw, not the probe
		act.generate_probes("sphere", seed=5)
		refused(host(act), "sphere")
		refused(dev(act), "sphere")
		# ... while the quadratic forms of such probes are served as on a plain plan
		act.run((a, b))
		plain.generate_probes("sphere", seed=5)
		plain.run((a, b))
		assert np.array_equal(act.moments(), plain.moments())
		assert np.array_equal(act.moment_sum(coef), plain.moment_sum(coef))
		dens = eng.DensityAccumulator("chebyshev", np.linspace(a, b, 9)[1:-1], ctx=op.ctx)
		dens.update(act)
		assert dens.get()[3] == P
		dens.close()
		# Lanczos entries on an action plan: as on any Chebyshev plan
		buf, ibuf = np.zeros((P, 8)), np.zeros(P, dtype=np.int32)
		hnd = act._h
		for i, call in enumerate([
			lambda: L.slq_plan_run(hnd, 1e-8),
			lambda: L.slq_plan_run_steps(hnd, 1e-8, 2),
			lambda: L.slq_plan_get_tridiag(hnd, buf.ctypes.data, buf.ctypes.data, ibuf.ctypes.data),
			lambda: L.slq_plan_quadrature(hnd, 0, None, buf.ctypes.data, None, None),
			lambda: L.slq_plan_get_basis(hnd, 0, Y.ctypes.data, n),
			lambda: L.slq_plan_fun_action(hnd, 0, None, Y.ctypes.data, n),
			lambda: L.slq_plan_fun_action_dmat(hnd, 0, None, D._h, 0),
		]):  # fmt: skip
			assert call() == _capi.SLQ_EINVAL, i
		assert np.all(Y == 3.5) and np.all(D.get() == 3.5)
		# nothing was disturbed: host probes, and both entries give the same bits
		act.set_probes(Z)
		assert host(act) == _capi.SLQ_OK
		act.set_probes(Z)
		assert dev(act) == _capi.SLQ_OK
		assert np.array_equal(D.get(), Y) and not np.any(Y == 3.5)
		(Yld, bar), = yardstick(A, Z, [coef], (a, b), np.float64)
		check(Y, Yld, bar, "after the guards")
		for badsteps in (0, 16385):
			with pytest.raises(ValueError):
				eng.ChebyshevPlan(op, P, badsteps, action=True)
	finally:
		for x in (act, plain, lan, D):
			x.close()
		op.close()


## ---- G. beyond the Lanczos cap -------------------------------------------------------------------------------------------
def test_beyond_the_lanczos_cap(eng):
	"""Degree 1400 - a Lanczos plan stops at 512 - on the 40 x 37 grid: a Jackson-damped step at mid-spectrum (a spectral
	projector) within bar of the long-double restatement, on a ring of K slots; and exp(-0.1 x) at degree 40 against the exact
	U f(L) U^T Z: within bar + ||z|| sum_{k > 40} |c_k|, the tail from a 200-coefficient expansion."""
	from primate_amd.chebyshev import chebyshev_coefficients

	K = acc_cols()
	m1, m2, P = 40, 37, 4
	A = host_matrix("grid40", np.float64)
	Z = probes_of(A.shape[0], P, np.float64, 16)
	b = bounds_of("grid40", np.float64)
	c, h = center_halfwidth(b)
	op = eng.DeviceOperator(A)
	try:
		deg = 1400
		with pytest.raises(ValueError):
			eng.LanczosPlan(op, P, deg, 0)
		coef = jackson_step_coefficients(deg, b, c)
		plan = eng.ChebyshevPlan(op, P, deg, action=True)
		try:
			assert plan.describe()["ring_slots"] == K and plan.workspace_bytes < 64 << 20
			plan.set_probes(Z)
			Y = plan.action(b, coef)
		finally:
			plan.close()
		(Yld, bar), = yardstick(A, Z, [coef], b, np.float64)
		check(Y, Yld, bar, "Jackson step, degree 1400")
		# it is the projector it approximates, away from the cut: U 1[lam <= c] U^T Z in the mean
		proj = action_eig(m1, m2, Z, lambda lam: (lam <= c).astype(np.float64))
		assert float(np.max(col_norms(Y - proj) / col_norms(Z))) < 0.2
		deg = 40
		coef = chebyshev_coefficients("exp", deg + 1, b, t=-0.1)
		tail = float(np.sum(np.abs(chebyshev_coefficients("exp", 200, b, t=-0.1)[deg + 1 :])))
		plan = eng.ChebyshevPlan(op, P, deg, action=True)
		try:
			plan.set_probes(Z)
			Y = plan.action(b, coef)
		finally:
			plan.close()
		(Yld, bar), = yardstick(A, Z, [coef], b, np.float64)
		exact = action_eig(m1, m2, Z, lambda lam: np.exp(-0.1 * lam))
		err = col_norms(Y - exact)
		full = bar + col_norms(Z) * tail
		print(f"exp(-0.1 A) Z, degree 40, against U f(L) U^T Z: max err / bar {float(np.max(err / full)):.3f} (tail {tail:.2e})")
		assert np.all(err <= full), float(np.max(err / full))
	finally:
		op.close()


## ---- H. the public interface ---------------------------------------------------------------------------------------------
class HostPolynomial:
	"""p(A) as a host LinearOperator: the restatement in `dtype`, its result rounded to fp64."""

	def __init__(self, A, coef, bounds, dtype):
		from scipy.sparse.linalg import LinearOperator

		self.A, self.coef, self.bounds, self.dt = A, coef, bounds, dtype
		n = A.shape[0]

		def mm(X):
			X = np.asarray(X, dtype=np.float64)
			X2 = X.reshape(n, -1)
			return np.asarray(action_recurrence(A, X2, coef, bounds, dtype), dtype=np.float64).reshape(X.shape)

		self.op = LinearOperator((n, n), matvec=mm, matmat=mm, rmatvec=mm, rmatmat=mm, dtype=np.float64)


def test_public_interface(eng):
	"""ChebyshevFunction @ x and @ X (130 columns in batches of 64) equal the engine-level action bit for bit; hutchpp, xtrace
	and diag over it agree with the same drivers over a host LinearOperator whose product is the fp64 restatement of the same
	polynomial - same probe stream - within 10x the difference those drivers themselves show between the fp64 restatement and
	the long-double restatement rounded to fp64 (the reference's own sensitivity to rounding-level inputs; floor 1e-12
	relative); diag in batches of 16 is the loop's estimate."""
	from primate_amd.chebyshev import ChebyshevFunction, chebyshev_coefficients
	from primate_amd.diagonal import diag
	from primate_amd.trace import hutchpp, xtrace

	A = host_matrix("grid40", np.float64)
	n, deg = A.shape[0], 40
	X = probes_of(n, 130, np.float64, 17)
	M = ChebyshevFunction(A, "exp", deg=deg, t=-0.1, batch=64)
	try:
		Y = M @ X
		y = M @ X[:, 5]
		b = M.bounds
		assert b == bounds_of("grid40", np.float64) and M._adjoint() is M
		coef = chebyshev_coefficients("exp", deg + 1, b, t=-0.1)
		op = eng.DeviceOperator(A)
		want = np.empty_like(Y)
		for c0, m in ((0, 64), (64, 64), (128, 2), (5, 1)):
			plan = eng.ChebyshevPlan(op, m, deg, action=True)
			plan.set_probes(X[:, c0 : c0 + m])
			got = plan.action(b, coef)
			plan.close()
			if m == 1:
				assert y.shape == (n,) and np.array_equal(y, got[:, 0])
			else:
				want[:, c0 : c0 + m] = got
		op.close()
		assert Y.shape == (n, 130) and np.array_equal(Y, want)
		(Yld, bar), = yardstick(A, X, [coef], b, np.float64)
		check(Y, Yld, bar, "ChebyshevFunction @ X")
		# linear and symmetric: one polynomial for every column
		lin = M @ (X[:, :2] @ np.array([[2.0], [-3.0]]))
		assert np.all(col_norms(lin - (2.0 * Y[:, :1] - 3.0 * Y[:, 1:2])) <= 5.0 * bar[:1] + 5.0 * bar[1:2])
		H64, Hld = HostPolynomial(A, coef, b, np.float64).op, HostPolynomial(A, coef, b, np.longdouble).op

		def agree(name, driver):
			got, r64, rld = (np.asarray(driver(o), dtype=np.float64) for o in (M, H64, Hld))
			scale = float(np.linalg.norm(r64))
			tol = max(10.0 * float(np.linalg.norm(r64 - rld)), 1e-12 * scale)
			dev = float(np.linalg.norm(got - r64))
			print(f"{name}: |device - host| / tol = {dev / tol:.3f} (tol {tol / scale:.2e} relative)")
			assert dev <= tol, (name, dev, tol)

		agree("hutchpp", lambda o: hutchpp(o, m=60, seed=3))
		agree("xtrace", lambda o: xtrace(o, batch=20, count=40, seed=3))
		agree("diag", lambda o: diag(o, converge="count", count=48, batch=16, seed=3))
		# the batched fold is the loop's: 48 samples, the loop's estimate and sample count
		est, info = diag(M, converge="count", count=48, batch=16, seed=3, full=True)
		assert info.nit == 48 and est.shape == (n,) and np.array_equal(est, diag(M, converge="count", count=48, batch=16, seed=3))
		# ... and a crude sanity check of what it estimates: diag exp(-0.1 A) through the sine basis, 48 Rademacher samples
		true = action_eig(40, 37, np.eye(n), lambda lam: np.exp(-0.1 * lam)).diagonal()
		assert float(np.linalg.norm(est - true) / np.linalg.norm(true)) < 0.2
	finally:
		M.close()
