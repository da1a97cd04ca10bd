"""Resumable Lanczos runs, the Gauss-Radau rule and the adaptive degree on the device.

1. a staged run IS the one-shot run (array_equal: the launches are the same);
2. every prefix of a run is the oracle's run of that degree (the tolerances of test_gpu_parity's golden tests);
3. the Radau rule against an independent construction (NumPy and 50 digits), bar max(1e-13, 10 d) with d the
   distance between those two - the reference side's own indeterminacy;
4. Gauss and Gauss-Radau values bracket the truth;
5. the adaptive driver stops where the oracle's statistics say it must;
6. errors leave the plan usable.
"""

import ctypes as C

import numpy as np
import pytest

from _radau_check import expected_stop, gauss_np, radau_mp, radau_np, rule_distance, stage_statistics
from conftest import laplacian_2d

pytestmark = pytest.mark.gpu

NINE = {"identity": {}, "abs": {}, "sqrt": {}, "log": {}, "inv": {}, "exp": {}, "smoothstep": {"a": 0.5, "b": 6.0}, "numrank": {}, "softsign": {}}
RULE_ABS = 1e-13  # the absolute bar test_standalone_quadrature_entry holds the Gauss rule to


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def rademacher(n, p, seed=1234):
	rng = np.random.default_rng(seed)
	return np.asfortranarray(np.floor(rng.random((n, p)) * 2) * 2 - 1)


@pytest.fixture(scope="module")
def lap24(eng):
	A = laplacian_2d(24)
	lam = np.linalg.eigvalsh(A.toarray())
	return A, eng.DeviceOperator(A), lam


def oracle_prefix(O, A, v, m, orth):
	"""alpha (m), beta (m + 1, beta[m] = the residual norm) of the oracle's run with deg = m, orth = min(orth, m)."""
	o = min(orth, m)
	al, be = np.zeros(m + 1), np.zeros(m + 1)
	Q = np.zeros((A.shape[0], max(2, o)), order="F")
	O.lanczos(A, v, m, 1e-8, o, al, be, Q)
	return al[:m], be


## ---- 1. staged = one-shot, exactly ----------------------------------------------------------------------------------
def _shape(name, golden):
	"""(A, probes, deg, orth, keep_basis, fun, fun_kwargs) of a plan shape."""
	rng = np.random.default_rng(7)
	if name == "ring_gram":  # the bench's path: ring-fed tiles, projections from Gram rows
		A = laplacian_2d(256)
		return A, rademacher(A.shape[0], 256, 1), 30, 3, False, "log", {}
	if name == "narrow_panel":  # generic passes
		A = laplacian_2d(64)
		return A, rademacher(A.shape[0], 8, 2), 30, 3, False, "log", {}
	if name == "sweeps":
		A = laplacian_2d(64)
		return A, rademacher(A.shape[0], 16, 3), 30, 12, False, "log", {}
	if name == "full_reorth_basis":
		A = laplacian_2d(32)
		return A, rademacher(A.shape[0], 8, 4), 24, 24, True, "log", {}
	if name == "dense_f64":
		B = rng.standard_normal((200, 200))
		return B @ B.T / 200 + np.eye(200), rademacher(200, 8, 5), 30, 3, False, "log", {}
	if name == "csr_f32":
		A = laplacian_2d(64, dtype=np.float32)
		return A, rademacher(A.shape[0], 8, 6).astype(np.float32), 30, 3, False, "log", {}
	if name == "early_stop":
		return np.asarray(golden["stop_A"]), np.asarray(golden["stop_v"]).reshape(-1, 1), 30, 30, False, "exp", {"t": -0.1}
	raise KeyError(name)


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("name", ["ring_gram", "narrow_panel", "sweeps", "full_reorth_basis", "dense_f64", "csr_f32", "early_stop"])
def test_staged_run_equals_the_one_shot_run(eng, golden, monkeypatch, name, graph):
	monkeypatch.setenv("SLQ_GRAPH", graph)  # (read when the plan is created)
	A, X, deg, orth, keep, fun, kw = _shape(name, golden)
	op = eng.DeviceOperator(A)
	plan = eng.LanczosPlan(op, X.shape[1], deg, orth, keep_basis=keep)
	if name == "ring_gram":
		d = plan.describe()
		assert d["tiles"] == 2 and d["sequence"] == "fused_gram", d
	grid = np.linspace(-1.0, 9.0, 64)
	## the one-shot run
	plan.set_probes(X)
	plan.run()
	a1, b1, s1 = plan.tridiag()
	q1, n1, w1 = plan.quadrature(fun, return_rule=True, **kw)
	y1 = plan.fun_action(fun, **kw) if keep else None
	acc = eng.DensityAccumulator("gaussian", grid, 0.3, ctx=op.ctx)
	acc.update(plan)
	dens1 = acc.get()
	acc.close()
	if name == "early_stop":
		assert np.all(s1 == 5)
	## the same plan, staged
	plan.set_probes(X)
	assert plan.steps_done == 0
	for m in (7, 20, 21, deg):
		plan.run(upto=m)
		assert plan.steps_done == m
		a, b, s = plan.tridiag()
		assert np.array_equal(a[:, :m], a1[:, :m]) and np.array_equal(b[:, : m + 1], b1[:, : m + 1]), (name, m)
		assert np.all(a[:, m:] == 0) and np.all(b[:, m + 1 :] == 0), (name, m)
		assert np.array_equal(s, np.minimum(s1, m)), (name, m, s)
	assert np.array_equal(a, a1) and np.array_equal(b, b1) and np.array_equal(s, s1)
	qa, na, wa = plan.quadrature_at(deg, fun, return_rule=True, **kw)
	assert np.array_equal(qa, q1) and np.array_equal(na, n1) and np.array_equal(wa, w1)
	## after the last stage the entries of the finished run work, and return the one-shot run's values
	q2, n2, w2 = plan.quadrature(fun, return_rule=True, **kw)
	assert np.array_equal(q2, q1) and np.array_equal(n2, n1) and np.array_equal(w2, w1)
	if keep:
		assert np.array_equal(plan.fun_action(fun, **kw), y1)
	acc = eng.DensityAccumulator("gaussian", grid, 0.3, ctx=op.ctx)
	acc.update(plan)
	dens2 = acc.get()
	acc.close()
	for u, v in zip(dens1, dens2):
		assert np.array_equal(u, v)
	## run_steps(deg) on fresh probes is slq_plan_run
	plan.set_probes(X)
	plan.run(upto=deg)
	a, b, s = plan.tridiag()
	assert np.array_equal(a, a1) and np.array_equal(b, b1) and np.array_equal(s, s1)
	assert np.array_equal(plan.quadrature(fun, **kw), q1)
	plan.close()
	op.close()


## ---- 2. every prefix meets the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("orth", [0, 3, 10, 12, 20])
def test_every_prefix_is_the_oracles_run_of_that_degree(eng, golden, oracle, lap24, orth):
	"""The operator, probes and degree of test_golden_laplacian_tridiag_and_rule / _all_functions, whose tolerances these are."""
	A, op, _ = lap24
	V = np.asfortranarray(golden["lap_probes"])
	P, deg = V.shape[1], 20
	plan = eng.LanczosPlan(op, P, deg, orth)
	plan.set_probes(V)
	for m in (1, 2, 3, 5, 8, 11, 12, 13, 17, 20):  # (also m < orth)
		plan.run(upto=m)
		a, b, s = plan.tridiag()
		assert np.array_equal(s, np.full(P, m))
		for i in range(P):
			al, be = oracle_prefix(oracle, A, V[:, i], m, orth)
			np.testing.assert_allclose(a[i, :m], al, rtol=0, atol=1e-12, err_msg=f"alpha m={m} probe {i}")
			np.testing.assert_allclose(b[i, : m + 1], be, rtol=0, atol=1e-12, err_msg=f"beta m={m} probe {i}")
		for fun, kw in NINE.items():
			ref = oracle.quad_batch(A, V, m, min(orth, m), fun=fun, fresh_q=True, **kw)
			np.testing.assert_allclose(plan.quadrature_at(m, fun, **kw), ref, rtol=1e-11, err_msg=f"{fun} m={m}")
	## an earlier prefix of a longer run: still that degree's run
	for m in (5, 13):
		ref = oracle.quad_batch(A, V, m, min(orth, m), fun="log", fresh_q=True)
		np.testing.assert_allclose(plan.quadrature_at(m, "log"), ref, rtol=1e-11)
	plan.close()


## ---- 3. the Radau rule against an independent construction ----------------------------------------------------------
def _record(line):
	print("YARDSTICK R " + line)


def _check_rule(name, got, alpha, beta, m, a):
	ref64, ref50 = radau_np(alpha, beta, m, a), radau_mp(alpha, beta, m, a)
	d = rule_distance(ref64, ref50)
	bar = max(RULE_ABS, 10.0 * d)
	err = rule_distance(got, ref50)
	_record(f"{name}: m={m} d(fp64 host, 50 digits)={d:.2e} bar={bar:.2e} device={err:.2e}")
	assert err <= bar, (name, err, bar)
	assert abs(got[0][0] - a) <= bar, (name, got[0][0], a)
	assert abs(np.sum(got[1]) - 1.0) <= RULE_ABS, name


@pytest.mark.parametrize("m", [1, 5, 20, 40])
def test_radau_rule_of_a_run_against_numpy_and_50_digits(eng, lap24, m):
	A, op, lam = lap24
	a = lam[0] / 2
	V = rademacher(A.shape[0], 6, 21)
	plan = eng.LanczosPlan(op, 6, 40, 3)
	plan.set_probes(V)
	plan.run(upto=m)
	al, be, _ = plan.tridiag()
	q, nodes, weights = plan.quadrature_at(m, "log", rule="radau", endpoint=a, return_rule=True)
	assert nodes.shape == (6, m + 1)
	for i in range(6):
		_check_rule(f"lap24 probe {i}", (nodes[i], weights[i]), al[i], be[i], m, a)
		ref = np.sum(np.log(nodes[i]) * weights[i]) * A.shape[0]
		assert abs(q[i] - ref) <= 1e-12 * abs(ref)
	## the stand-alone entry on the same Jacobi matrices: the same rule, bit for bit
	from primate_amd.integrate import quadrature

	n2, w2 = eng.quadrature_radau_batch(al[:, :m], be[:, :m], be[:, m], a)
	assert np.array_equal(n2, nodes) and np.array_equal(w2, weights)
	n3, w3 = quadrature(al[0, :m], be[0, :m], quad="radau", endpoint=a, residual=be[0, m])
	assert np.array_equal(n3, nodes[0]) and np.array_equal(w3, weights[0])
	## an endpoint above the smallest Ritz value is an error, not a number; the plan stays usable
	theta = gauss_np(al[0], be[0], m)[0]
	with pytest.raises(ValueError, match="Ritz"):
		plan.quadrature_at(m, "log", rule="radau", endpoint=float(theta[0]) + 0.25)
	with pytest.raises(ValueError):
		eng.quadrature_radau_batch(al[:, :m], be[:, :m], be[:, m], float(theta[0]) + 0.25)
	assert np.array_equal(plan.quadrature_at(m, "log", rule="radau", endpoint=a), q)
	plan.close()


def _edge_jacobi():
	"""(name, alpha (m), beta (m + 1), endpoint): positive definite Jacobi matrices of norm O(1) at the edges of the rule."""
	out = []
	d = 10.0 ** np.linspace(-3.0, 0.0, 12)  # graded: D^(1/2) tridiag(1/2, 1, 1/2) D^(1/2), positive definite
	e = np.r_[0.0, 0.5 * np.sqrt(d[1:] * d[:-1]), 0.3]
	out.append(("graded 1e-3..1", d, e, 0.0))
	out.append(("graded 1..1e-3", d[::-1].copy(), np.r_[0.0, e[1:12][::-1], 1e-4], 0.0))
	k = 12
	dl, el = np.full(k, 2.0), np.r_[0.0, np.full(k - 1, -1.0), -1.0]
	t = el.copy()
	t[5] = 1e-9  # tiny interior coupling
	out.append(("Laplacian, interior coupling 1e-9", dl, t, 0.01))
	t = el.copy()
	t[k] = 1e-10  # tiny coupling to the border: the prescribed node carries almost no weight
	out.append(("Laplacian, border coupling 1e-10", dl, t, 0.01))
	t = el.copy()
	t[1] = 1e-9  # the first vector almost decoupled
	out.append(("Laplacian, first coupling 1e-9", dl, t, 0.01))
	out.append(("m = 1", np.array([2.5]), np.array([0.0, 0.7]), 0.1))
	out.append(("m = 1, endpoint far below", np.array([2.5]), np.array([0.0, 0.7]), -100.0))
	out.append(("m = 2", np.array([1.0, 3.0]), np.array([0.0, 0.5, 2.0]), 0.25))
	return out


def test_radau_rule_at_its_edges_through_the_standalone_entry(eng):
	for name, al, be, a in _edge_jacobi():
		m = len(al)
		nodes, weights = eng.quadrature_radau_batch(al[None, :], be[None, :m], [be[m]], a)
		_check_rule(name, (nodes[0], weights[0]), al, be, m, a)
		q, _, _ = eng.quadrature_radau_batch(al[None, :], be[None, :m], [be[m]], a, fun="exp", t=-1.0)
		ref = np.sum(np.exp(-nodes[0]) * weights[0])
		assert abs(q[0] - ref) <= 1e-13 * abs(ref)
	## a batch wider than a wavefront, every lane its own matrix
	rng = np.random.default_rng(5)
	nb, m = 70, 9
	al = rng.uniform(2.0, 3.0, (nb, m))
	be = np.c_[np.zeros(nb), rng.uniform(0.1, 0.9, (nb, m))]
	nodes, weights = eng.quadrature_radau_batch(al, be[:, :m], be[:, m], 0.05)
	for i in (0, 63, 64, 69):
		_check_rule(f"random batch lane {i}", (nodes[i], weights[i]), al[i], be[i], m, 0.05)
	## beta_m = 0: the Gauss rule is exact; it comes back behind a zero-weight node at the endpoint
	nodes, weights = eng.quadrature_radau_batch(al[:3], be[:3, :m], np.zeros(3), 0.05)
	gn, gw = eng.quadrature_batch(al[:3], be[:3, :m])
	assert np.array_equal(nodes[:, 1:], gn) and np.array_equal(weights[:, 1:], gw)
	assert np.all(nodes[:, 0] == 0.05) and np.all(weights[:, 0] == 0.0)


def test_a_probe_that_stopped_early_returns_its_gauss_value(eng, golden):
	A, v = np.asarray(golden["stop_A"]), np.asarray(golden["stop_v"]).reshape(-1, 1)
	op = eng.DeviceOperator(A)
	plan = eng.LanczosPlan(op, 1, 20, 20)
	plan.set_probes(v)
	for m in (5, 7, 20):
		plan.run(upto=m)
		assert plan.tridiag()[2][0] == 5
		g, gn, gw = plan.quadrature_at(m, "exp", return_rule=True, t=-0.1)
		r, rn, rw, st = plan.quadrature_at(m, "exp", rule="radau", endpoint=-1e3, return_rule=True, return_stage=True, t=-0.1)
		assert np.array_equal(r, g) and np.array_equal(rn[:, 1:], gn) and np.array_equal(rw[:, 1:], gw) and rw[0, 0] == 0.0
		assert st[2] == 0.0 and st[3] == 1.0 and st[0] == g[0]
	plan.close()
	op.close()


## ---- 4. the bracket holds --------------------------------------------------------------------------------------------
def test_gauss_and_radau_values_bracket_the_truth(eng, lap24):
	A, op, lam = lap24
	n = A.shape[0]
	_, U = np.linalg.eigh(A.toarray())
	a = lam[0] / 2
	funs = {"log": ({}, np.log), "inv": ({}, lambda x: 1.0 / x), "exp": ({"t": -1.0}, lambda x: np.exp(-x))}
	ncase, worst = 0, 0.0
	for orth in (0, 3, 10, 60):
		V = rademacher(n, 8, 100 + orth)
		C2 = (U.T @ V) ** 2
		plan = eng.LanczosPlan(op, 8, 60, orth)
		plan.set_probes(V)
		for m in (5, 10, 20, 40):
			plan.run(upto=m)
			for fun, (kw, f) in funs.items():
				truth = f(lam) @ C2
				g = plan.quadrature_at(m, fun, **kw)
				r = plan.quadrature_at(m, fun, rule="radau", endpoint=a, **kw)
				## slack: 1e-12 of the truth (where the CPU oracle and a NumPy Radau rule miss no case) plus the device's parity bar
				## against the oracle, rtol 1e-11 of the value
				slack = 1e-12 * np.abs(truth) + 1e-11 * np.maximum(np.abs(g), np.abs(r))
				lo, hi = np.minimum(g, r), np.maximum(g, r)
				miss = np.maximum(lo - slack - truth, truth - hi - slack)
				worst = max(worst, float(np.max(miss / np.abs(truth))))
				assert np.all(miss <= 0), (orth, m, fun, miss)
				ncase += 8
		plan.close()
	print(f"bracket: {ncase} cases, largest (miss - slack) / |truth| = {worst:.2e}")
	assert ncase == 384


## ---- 5. the driver stops where the oracle says ------------------------------------------------------------------------
STAGES = [5, 10, 15, 20, 30, 40, 60]


def probes32(n):
	return np.asfortranarray(np.random.default_rng(1234).choice([-1.0, 1.0], size=(n, 32)))


@pytest.fixture(scope="module")
def oracle_stages(oracle, lap24):
	"""S_k and the bracket widths of the stages from the oracle alone: Lanczos of degree m, orth min(3, m), NumPy rules."""
	A, _, lam = lap24
	n = A.shape[0]
	V = probes32(n)
	S, W = [], []
	for m in STAGES:
		g, r = np.zeros(32), np.zeros(32)
		for i in range(32):
			al, be = oracle_prefix(oracle, A, V[:, i], m, 3)
			th, ta = gauss_np(al, be, m)
			g[i] = np.sum(np.log(th) * ta) * n
			th, ta = radau_np(al, be, m, lam[0] / 2)
			r[i] = np.sum(np.log(th) * ta) * n
		s, w = stage_statistics(g, r)
		S.append(s)
		W.append(w)
	return V, np.array(S), np.array(W)


@pytest.mark.parametrize("with_endpoint, deg_rtol", [(False, 1e-5), (True, 3e-4)])
def test_adaptive_driver_stops_where_the_oracle_says(eng, lap24, oracle_stages, with_endpoint, deg_rtol):
	"""The oracle's statistics here: relative change of the batch sum per stage 5.9e-3, 7.9e-4, 1.4e-4, 3.3e-5, 1.16e-6,
	9.6e-9 (stages 10 .. 60); relative bracket width 2.7e-2, 3.2e-3, 6.3e-4, 1.4e-4, 7.7e-6, 1.5e-7 (stages 5 .. 40).
	deg_rtol = 3e-4 with the endpoint stops at 20 (6.3e-4 > 3e-4 > 1.4e-4). deg_rtol = 1e-5 without it stops at 40: by the
	rule |S_k - S_{k-1}| <= deg_rtol |S_k|, stage 30 (change 3.3e-5) does not meet 1e-5, stage 40 (1.16e-6) is the first that
	does. Both thresholds lie a factor >= 2 from the statistics on either side, which the test asserts from the oracle
	(recomputed here, not taken from this list) before it asserts the device."""
	A, op, lam = lap24
	V, S, W = oracle_stages
	endpoint = lam[0] / 2 if with_endpoint else None
	stat = W / np.abs(S) if with_endpoint else np.r_[np.inf, np.abs(np.diff(S)) / np.abs(S[1:])]
	print("oracle statistic per stage:", dict(zip(STAGES, stat)))
	want = expected_stop(STAGES, S, W, deg_rtol, with_endpoint)
	k = STAGES.index(want)
	assert 0 < k < len(STAGES) - 1
	assert np.all(stat[:k] >= 2 * deg_rtol) and stat[k] <= deg_rtol / 2, (stat, deg_rtol)  # the margin: against a device-oracle distance of 1e-11
	assert want == (20 if with_endpoint else 40)
	q, used, hist = eng.quad_adaptive(op, V, 60, 3, "log", stages=STAGES, deg_rtol=deg_rtol, endpoint=endpoint)
	assert used == want
	assert [m for m, _ in hist] == STAGES[: k + 1]
	for (m, st), s_ref, w_ref in zip(hist, S, W):
		st = np.atleast_2d(st)
		assert abs(st[0, 0] - s_ref) <= 1e-11 * abs(s_ref) and st[0, 3] == 32 and st[0, 2] == 0.0
		if with_endpoint:
			assert abs(st[1, 2] - w_ref) <= 2e-11 * abs(s_ref)  # (a sum of 32 differences of values held to 1e-11 each)
	## the values are those of a fixed deg = deg_used run on the same plan, bit for bit
	plan = eng.LanczosPlan(op, 32, 60, 3)
	plan.set_probes(V)
	plan.run(upto=used)
	g = plan.quadrature_at(used, "log")
	if with_endpoint:
		r = plan.quadrature_at(used, "log", rule="radau", endpoint=endpoint)
		assert q.shape == (32, 2) and np.array_equal(q[:, 0], g) and np.array_equal(q[:, 1], r)
	else:
		assert np.array_equal(q, g)
	plan.close()
	## ... and what a plan of that degree returns, at the parity bar
	np.testing.assert_allclose(g, eng.quad_batch(op, V, used, 3, fun="log"), rtol=1e-11)


def test_matrix_function_and_hutch_agree_on_the_degree(eng, lap24):
	from primate_amd.operators import MatrixFunction
	from primate_amd.trace import hutch

	A, op, lam = lap24
	V = probes32(A.shape[0])
	M = MatrixFunction(A, "log", deg=5, orth=3, deg_max=60, deg_rtol=1e-5, deg_step=5)
	y = M.quad(V)
	used = M.deg_used
	## the same stages through the engine: the same stop, the same values
	q, used2, hist = eng.quad_adaptive(op, V, 60, 3, "log", stages=list(range(5, 61, 5)), deg_rtol=1e-5)
	assert used == used2 and np.array_equal(y, q) and 5 < used < 60
	assert [m for m, _ in M.deg_history] == [m for m, _ in hist]
	assert M.quad_bounds is None
	## hutch goes through the same adaptive quad: on the probes it draws, the mean of M.quad and the same degree
	from primate_amd.random import isotropic

	est = hutch(M, batch=32, converge="count", count=32, seed=3)
	used_h = M.deg_used
	W = isotropic(pdf="rademacher", seed=np.random.default_rng(3))(size=(A.shape[0], 32))
	yw = M.quad(W)
	assert M.deg_used == used_h and 5 < used_h <= 60
	assert abs(est - np.mean(yw)) <= 1e-12 * abs(est)
	truth = float(np.sum(np.log(lam)))
	assert abs(est - truth) < 0.05 * abs(truth)
	## with the endpoint: the bracket of every probe, around the truth
	Mb = MatrixFunction(A, "log", deg=5, orth=3, deg_max=60, deg_rtol=3e-4, deg_step=5, endpoint=lam[0] / 2)
	yb = Mb.quad(V)
	lo, hi = Mb.quad_bounds
	plan = eng.LanczosPlan(op, 32, 60, 3)
	plan.set_probes(V)
	plan.run(upto=Mb.deg_used)
	g = plan.quadrature_at(Mb.deg_used, "log")
	r = plan.quadrature_at(Mb.deg_used, "log", rule="radau", endpoint=lam[0] / 2)
	plan.close()
	assert np.array_equal(yb, g) and np.array_equal(lo, np.minimum(g, r)) and np.array_equal(hi, np.maximum(g, r))
	truth_p = np.log(lam) @ ((np.linalg.eigh(A.toarray())[1].T @ V) ** 2)
	assert np.all(lo - 1e-11 * np.abs(lo) <= truth_p) and np.all(truth_p <= hi + 1e-11 * np.abs(hi))
	## device-drawn probes
	y = M.quad_generated(32, "rademacher", seed=9)
	assert y.shape == (32,) and 5 < M.deg_used <= 60
	## a deg_rtol nothing meets ends at deg_max with the history complete
	q, used, hist = eng.quad_adaptive(op, V, 60, 3, "log", stages=STAGES, deg_rtol=1e-300)
	assert used == 60 and [m for m, _ in hist] == STAGES
	np.testing.assert_allclose(q, eng.quad_batch(op, V, 60, 3, fun="log"), rtol=1e-11)
	q, used, hist = eng.quad_adaptive(op, V, 60, 3, "log", stages=STAGES, deg_rtol=1e-300, endpoint=lam[0] / 2)
	assert used == 60 and [m for m, _ in hist] == STAGES and q.shape == (32, 2)


## ---- 6. errors and state ---------------------------------------------------------------------------------------------
def test_errors_leave_the_plan_usable(eng, lap24):
	from primate_amd import _capi

	A, op, lam = lap24
	V = rademacher(A.shape[0], 4, 8)
	plan = eng.LanczosPlan(op, 4, 20, 3, keep_basis=True)
	L = _capi.lib()
	with pytest.raises(ValueError):  # no probes yet
		plan.run(upto=5)
	plan.set_probes(V)
	plan.run()
	a1, b1, _ = plan.tridiag()
	q1 = plan.quadrature("log")
	plan.set_probes(V)
	assert plan.steps_done == 0
	for bad in (0, -1, 21):
		assert L.slq_plan_run_steps(plan._h, 1e-8, bad) == _capi.SLQ_EINVAL
	plan.run(upto=8)
	for bad in (8, 3, 21):  # upto <= cur, upto > deg
		assert L.slq_plan_run_steps(plan._h, 1e-8, bad) == _capi.SLQ_EINVAL
	assert L.slq_plan_run_steps(plan._h, 1e-6, 12) == _capi.SLQ_EINVAL  # another rtol mid-run
	assert L.slq_plan_run(plan._h, 1e-8) == _capi.SLQ_EINVAL  # the one-shot entry needs fresh probes
	## the entries of the finished run, mid-run: an error that names the way out
	acc = eng.DensityAccumulator("gaussian", np.linspace(0, 8, 16), 0.3, ctx=op.ctx)
	dg = eng.DiagAccumulator(A.shape[0], ctx=op.ctx)
	for call in (lambda: plan.quadrature("log"), lambda: plan.fun_action("log"), lambda: plan.basis(0), lambda: acc.update(plan), lambda: dg.update(plan, "log")):
		with pytest.raises(ValueError, match="slq_plan_quadrature_at"):
			call()
	for bad_m in (0, 9, -2):
		with pytest.raises(ValueError):
			plan.quadrature_at(bad_m, "log")
	assert L.slq_plan_quadrature_at(plan._h, 8, 2, 0.0, 3, None, None, None, None, None) == _capi.SLQ_EINVAL
	assert L.slq_plan_quadrature_at(plan._h, 8, 1, C.c_double(float("nan")), 3, None, None, None, None, None) == _capi.SLQ_EINVAL
	## a plan with stale ring columns (the drop-in entry's) is not resumable
	assert L.slq_debug_plan_mark_stale(plan._h, 2) == 0
	assert L.slq_plan_run_steps(plan._h, 1e-8, 12) == _capi.SLQ_EINVAL
	assert b"stale" in L.slq_last_error()
	assert L.slq_debug_plan_mark_stale(plan._h, 0) == 0
	## after all of that the run goes on as if nothing had happened
	assert plan.steps_done == 8
	a, b, _ = plan.tridiag()
	assert np.array_equal(a[:, :8], a1[:, :8]) and np.array_equal(b[:, :9], b1[:, :9])
	plan.run(upto=20)
	assert np.array_equal(plan.quadrature("log"), q1)
	with pytest.raises(ValueError):  # finished: nothing left to run
		plan.run(upto=20)
	## new probes reset the count, set or generated
	plan.set_probes(V)
	assert plan.steps_done == 0
	plan.run(upto=4)
	plan.generate_probes("rademacher", seed=1)
	assert plan.steps_done == 0
	plan.run(upto=20)
	assert plan.steps_done == 20 and np.all(np.isfinite(plan.quadrature("log")))
	acc.close()
	dg.close()
	plan.close()
