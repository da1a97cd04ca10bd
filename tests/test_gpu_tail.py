"""The serial tail of a run: the rescue of an offered step as ONE launch whose last workgroup
finishes the panel, what a plan's second run starts from, the two storage forms of the first-row QL, and the profiling
events without a system-scope fence. Needs a real MI355X (`-m gpu`).

Bars. Rescue: the tridiagonal within 1e-10 (fp32: 3e-4) of the run that reads every column, as tests/test_gpu_omega.py holds
it; runs of one plan np.array_equal to each other. Second run of a plan: np.array_equal to a fresh plan. QL: the bars of
tests/test_ql_edges.py (check_rule: nodes C_NODE k eps ||T||, clustered weights 1e-13, sums 1e-12) with the oracle's C QL as
the reference - the same textbook algorithm in another storage -, and np.array_equal between any two places a matrix takes in
a batch."""

import time

import numpy as np
import pytest

import _omega_cases as oc
import test_ql_edges as tq
from conftest import laplacian_2d

pytestmark = pytest.mark.gpu

DEG = 12


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


@pytest.fixture(scope="module")
def grid():
	"""The 200^2 5-point grid (40,000 rows: the smallest size where the device skips and offers its windows), fp64 and fp32
	operators made on first use, and the SLQ_OMEGA=0 runs the rescue cases are held to (one per shape)."""
	state = {"A": laplacian_2d(200), "ops": {}, "off": {}}
	yield state
	for op in state["ops"].values():
		op.close()


def _op(eng, grid, dtype):
	key = np.dtype(dtype).name
	if key not in grid["ops"]:
		grid["ops"][key] = eng.DeviceOperator(grid["A"].astype(dtype))
	return grid["ops"][key]


def _plan_outputs(plan):
	a, b, s = plan.tridiag()
	return {"alpha": a, "beta": b, "steps": s, "log": plan.quadrature("log"), "exp": plan.quadrature("exp", t=-0.1)}


def _same(x, y):
	return all(np.array_equal(x[k], y[k]) for k in ("alpha", "beta", "steps", "log", "exp"))


def _tridiag_dist(a, b):
	return max(np.max(np.abs(a[k] - b[k])) / np.max(np.abs(b[k])) for k in ("alpha", "beta"))


def _rescue_case(eng, monkeypatch, grid, dtype, P, j, bar):
	monkeypatch.setenv("SLQ_TILES", "2")
	op = _op(eng, grid, dtype)
	X = oc.rademacher(grid["A"].shape[0], P, 11 + P, dtype)
	key = (np.dtype(dtype).name, P)
	if key not in grid["off"]:
		grid["off"][key] = oc.run(eng, monkeypatch, op, X, DEG, 3, {"SLQ_OMEGA": 0})
	off = grid["off"][key]
	for k in oc.OFF_KEYS:
		monkeypatch.delenv(k, raising=False)
	monkeypatch.setenv("SLQ_OMEGA_RESCUE", str(j))
	plan = eng.LanczosPlan(op, P, DEG, 3)
	monkeypatch.delenv("SLQ_OMEGA_RESCUE")
	info = plan.describe()
	NP = info["panels"]
	assert info["omega"] == 1 and info["sequence"] == "fused_gram", info
	first = None
	for prof in (False, True):  # graph replay, then the launches one by one between events
		plan.profile_enable(prof)
		for rep in range(3):  # the SAME plan: the tickets are back at zero, and whichever workgroup finishes gives the same bits
			plan.window_columns(reset=True)
			plan.set_probes(X)
			plan.run()
			got = _plan_outputs(plan)
			cols, resc = plan.window_columns(), plan.window_flags()[1]
			assert np.all(resc[j] == 1), (j, resc.T)  # every panel rescued at j
			assert cols["rescues"] >= NP, cols
			ab = _tridiag_dist(got, off)
			print(f"TAIL-RESCUE {np.dtype(dtype).name} P={P} panels={NP} j={j} profiled={prof} run {rep}: {cols}, tridiagonal {ab:.2e} from SLQ_OMEGA=0")
			assert ab <= bar, ab
			if first is None:
				first = got
			assert _same(got, first), f"run {rep} (profiled={prof}) differs from the plan's first run"
	plan.profile_enable(False)
	plan.close()


@pytest.mark.parametrize("j", [3, 7, DEG - 1])
@pytest.mark.parametrize("P", [130, 32])  # two panels with a ragged second one; one narrow panel
def test_rescue_in_one_launch(eng, monkeypatch, grid, P, j):
	_rescue_case(eng, monkeypatch, grid, np.float64, P, j, 1e-10)


def test_rescue_in_one_launch_fp32(eng, monkeypatch, grid):
	_rescue_case(eng, monkeypatch, grid, np.float32, 260, 7, 3e-4)


@pytest.mark.parametrize("orth", [3, 6])  # with the edge recurrence (its state and flags are cleared too) and without
def test_second_run_starts_from_zero(eng, monkeypatch, grid, orth):
	"""A plan that ran to deg, got new probes and ran again equals a fresh plan on those probes bit for bit."""
	monkeypatch.setenv("SLQ_TILES", "2")
	for k in oc.OFF_KEYS:
		monkeypatch.delenv(k, raising=False)
	op = _op(eng, grid, np.float64)
	n, P = grid["A"].shape[0], 130
	X1, X2 = oc.rademacher(n, P, 1), oc.rademacher(n, P, 2)
	used = eng.LanczosPlan(op, P, DEG, orth)
	assert used.describe()["omega"] == (1 if orth == 3 else 0)
	used.set_probes(X1)
	used.run()
	used.quadrature("log")
	used.set_probes(X2)
	used.run()
	again = _plan_outputs(used)
	flags_again = used.window_flags() if orth == 3 else None
	used.close()
	fresh = eng.LanczosPlan(op, P, DEG, orth)
	fresh.set_probes(X2)
	fresh.run()
	ref = _plan_outputs(fresh)
	if orth == 3:
		assert all(np.array_equal(a, b) for a, b in zip(flags_again, fresh.window_flags()))
	fresh.close()
	assert _same(again, ref)


def test_second_run_starts_from_zero_behind_an_early_stop(golden, eng):
	"""The operator of tests/test_gpu_parity.py::test_golden_early_stop (five distinct eigenvalues: every run stops after 5 of
	20 steps): the rows of alpha and nu behind the stop are zero on the plan's second run too, and that run equals a fresh
	plan's."""
	A, v = golden["stop_A"], np.asarray(golden["stop_v"], dtype=np.float64)
	op = eng.DeviceOperator(A)
	rng = np.random.default_rng(5)
	w = np.floor(rng.random(len(v)) * 2) * 2 - 1
	used = eng.LanczosPlan(op, 1, 20, 20)
	used.set_probes(w)
	used.run()
	a0, b0, s0 = used.tridiag()
	assert s0[0] == 5 and np.all(b0[0, 6:] == 0) and np.all(a0[0, 5:] == 0) and np.all(a0[0, :5] != 0), (s0, a0, b0)
	used.set_probes(v)
	used.run()
	a, b, s = used.tridiag()
	q = used.quadrature("identity")
	used.close()
	fresh = eng.LanczosPlan(op, 1, 20, 20)
	fresh.set_probes(v)
	fresh.run()
	fa, fb, fs = fresh.tridiag()
	fq = fresh.quadrature("identity")
	fresh.close()
	op.close()
	assert s[0] == 5 and np.all(b[0, 6:] == 0) and np.all(a[0, 5:] == 0), (s, a, b)
	assert np.array_equal(a, fa) and np.array_equal(b, fb) and np.array_equal(s, fs) and np.array_equal(q, fq)


def _oracle_reference(oracle):
	"""tests/test_ql_edges.py::reference with the oracle's first-row QL in the place of the 50-digit one (same fields)."""

	def ref(d, e):
		w, z, rc = oracle.tridiag_ql(np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64), first_row_only=True)
		assert rc == 0
		o = np.argsort(w, kind="stable")
		nodes, weights = w[o], z[0, o] ** 2
		norm = float(np.max(np.abs(nodes)))
		fun = {"identity": (float(np.sum(nodes * weights)), float(np.sum(np.abs(nodes) * weights)))}
		if 1e-100 < norm < 1e100:
			with np.errstate(over="ignore"):
				ex = np.exp(nodes)
			if np.all(np.isfinite(ex)) and np.sum(ex * weights) < 1e300:
				fun["exp"] = (float(np.sum(ex * weights)), float(np.sum(ex * weights)))
		return {"nodes": nodes, "weights": weights, "norm": norm, "fun": fun, "action": {}}

	return ref


def _random_jacobi(k, nb, seed):
	"""Entries of size 1e-3 .. 1 (||T|| <= 3, as the random cases of the edge set): sum exp(theta) tau is then as well
	conditioned as its bar assumes. With ||T|| ~ 100 the sum hangs on the top node's weight, which is far below eps and has
	no relative accuracy in any QL."""
	rng = np.random.default_rng(seed)
	D = rng.uniform(-1.0, 1.0, (nb, k)) * 10.0 ** rng.integers(-3, 1, (nb, 1))
	E = rng.uniform(0.1, 1.0, (nb, k)) * np.abs(D).max(axis=1, keepdims=True)
	E[:, 0] = 0.0
	## a zero tail (an early stop) and an interior split in some of them: lanes of very different sweep counts
	for i in range(0, nb, 7):
		if k > 2:
			D[i, k // 2 :], E[i, k // 2 :] = 0.0, 0.0
	for i in range(3, nb, 11):
		if k > 3:
			E[i, k // 3] = 0.0
	return D, E


def _check_batch(eng, monkeypatch, oracle, names, D, E):
	monkeypatch.setattr(tq, "reference", _oracle_reference(oracle))
	worst = {"node": 0.0, "fun": 0.0, "orth": 0.0, "resid": 0.0}
	nodes, weights = eng.quadrature_batch(D, E)
	quad = {f: eng.quadrature_batch(D, E, fun=f)[0] for f in ("identity", "exp")}
	for i, name in enumerate(names):
		tq.check_rule(name, D[i], E[i], nodes[i], weights[i], {f: quad[f][i] for f in quad}, worst)
	return nodes, weights, quad, worst


@pytest.mark.parametrize("k", [1, 2, 3, 32, 64])
def test_ql_forms_on_the_edge_set(eng, monkeypatch, oracle, k):
	"""The edge set of tests/test_ql_edges.py at the sizes the lane form serves (k <= 64: one probe per wave)."""
	cases = tq.edge_cases()[k]
	D, E = np.array([d for _, d, _ in cases]), np.array([e for _, _, e in cases])
	*_, worst = _check_batch(eng, monkeypatch, oracle, [c[0] for c in cases], D, E)
	print(f"TAIL-QL edge set k={k} ({len(cases)} matrices): node {worst['node']:.3f} k eps ||T|| (bar {tq.C_NODE}), sum f tau {worst['fun']:.2e} (bar {tq.F_TOL})")


@pytest.mark.parametrize("k", [1, 2, 3, 30, 63, 64, 65])  # 65: the LDS form
def test_ql_forms_on_random_jacobi_matrices(eng, monkeypatch, oracle, k):
	"""70 random Jacobi matrices against the oracle QL, and every matrix bit for bit the same wherever it stands in a batch
	and whatever the batch size (1, 63, 65, 70, and the batch reversed)."""
	D, E = _random_jacobi(k, 70, 100 + k)
	nodes, weights, quad, worst = _check_batch(eng, monkeypatch, oracle, [f"random {k} #{i}" for i in range(70)], D, E)
	print(f"TAIL-QL random k={k}: node {worst['node']:.3f} k eps ||T|| (bar {tq.C_NODE}), sum f tau {worst['fun']:.2e} (bar {tq.F_TOL})")
	for nb in (1, 63, 65):
		q, nd, w = eng.quadrature_batch(D[:nb], E[:nb], fun="exp")
		assert np.array_equal(nd, nodes[:nb]) and np.array_equal(w, weights[:nb]) and np.array_equal(q, quad["exp"][:nb]), nb
	q, nd, w = eng.quadrature_batch(D[::-1], E[::-1], fun="exp")
	assert np.array_equal(nd[::-1], nodes) and np.array_equal(w[::-1], weights) and np.array_equal(q[::-1], quad["exp"])
	q, nd, w = eng.quadrature_batch(D[69:], E[69:], fun="exp")  # the last one alone
	assert np.array_equal(nd, nodes[69:]) and np.array_equal(w, weights[69:]) and np.array_equal(q, quad["exp"][69:])


@pytest.mark.parametrize("k", [30, 65])
def test_ql_forms_keep_the_nan_and_the_flag(eng, k):
	"""An all-zero probe is NaN (0/0 in the reference) and the others are not; a matrix whose QL cannot converge (NaN entries:
	no deflation test ever holds) still raises the flag, in both forms."""
	from primate_amd import _capi

	A = laplacian_2d(20)
	X = oc.rademacher(A.shape[0], 8, 3)
	X[:, 5] = 0.0
	op = eng.DeviceOperator(A)
	q = eng.quad_batch(op, X, k, 3, fun="exp")
	op.close()
	assert np.isnan(q[5]) and np.all(np.isfinite(np.delete(q, 5))), q
	D, E = _random_jacobi(k, 5, 9)
	eng.quadrature_batch(D, E)
	D[3, k // 2] = np.nan
	with pytest.raises(_capi.SlqError) as ei:
		eng.quadrature_batch(D, E)
	assert ei.value.code == _capi.SLQ_ENOTCONV


def test_profiling_events(eng, monkeypatch, grid):
	"""With profiling on, over 3 runs: every class with launches has time, the classes sum to no more than the wall time, an
	offered step from the second on has three launches of class finalize (one more than the same step of a plan that offers
	nothing), and a quadrature call has one launch."""
	monkeypatch.setenv("SLQ_TILES", "2")
	op = _op(eng, grid, np.float64)
	P, runs = 130, 3
	X = oc.rademacher(grid["A"].shape[0], P, 4)
	prof = {}
	for omega in (1, 0):
		for k in oc.OFF_KEYS:
			monkeypatch.delenv(k, raising=False)
		monkeypatch.setenv("SLQ_OMEGA", str(omega))
		plan = eng.LanczosPlan(op, P, DEG, 3)
		monkeypatch.delenv("SLQ_OMEGA")
		assert plan.describe()["omega"] == omega
		plan.set_probes(X)
		plan.run()  # (untimed: first launches)
		plan.quadrature("log")
		plan.profile_enable(True)
		plan.profile_read(reset=True)
		eng.default_context().synchronize()
		t0 = time.perf_counter()
		for _ in range(runs):
			plan.set_probes(X)
			plan.run()
			plan.quadrature("log")
		pr = plan.profile_read(reset=True)
		wall_ms = (time.perf_counter() - t0) * 1e3
		plan.close()
		total = sum(v["ms"] for v in pr.values())
		print(f"TAIL-EVENTS omega={omega}: wall {wall_ms:.3f} ms, classes {total:.3f} ms, {pr}")
		for name, v in pr.items():
			assert (v["ms"] > 0.0) == (v["launches"] > 0), (name, v)
		assert 0.0 < total <= wall_ms, (total, wall_ms)
		assert pr["quadrature"]["launches"] == runs, pr["quadrature"]
		prof[omega] = pr
	## offered steps: 2 .. deg - 1; from the second on each has k_fin_gram, the rescue launch and k_fin_beta_gram
	assert prof[1]["finalize"]["launches"] - prof[0]["finalize"]["launches"] == runs * (DEG - 3), (prof[1]["finalize"], prof[0]["finalize"])
	assert prof[0]["finalize"]["launches"] >= runs * 2 * (DEG - 3)
