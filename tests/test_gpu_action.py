"""Two-pass f(A)v on the device (recompute plans: slq_plan_create_recompute, LanczosPlan(basis="recompute"),
MatrixFunction(basis="recompute" | "auto"), slq_fAv_batch_mode).

A - the replay is exact (no tolerance); B - against the kept basis, at a bar derived from the two summation orders; C - against
the truth at the bars of the project's own tests of the kept-basis action; D - the full-size shape the feature is for; E - the
automatic choice. Every test needs a real MI355X (`-m gpu`)."""

from pathlib import Path

import numpy as np
import pytest

from _action_check import action_coeffs, dense_spd, order_bound, random_spd_graph
from conftest import laplacian_2d, laplacian_3d

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GB = 1e9


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def f_exp(x):
	return np.exp(-0.1 * x)


_HOST = {}


def host_matrix(kind, dtype):
	"""The test matrices, built once per module: 2-D Laplacian 200^2, 3-D 40^3, a random graph (scattered neighbours: the
	store-and-revisit sweeps), a dense SPD matrix."""
	key = (kind, np.dtype(dtype).name)
	if key not in _HOST:
		if kind == "lap2d":
			_HOST[key] = laplacian_2d(200, dtype)
		elif kind == "lap3d":
			_HOST[key] = laplacian_3d(40, dtype)
		elif kind == "graph":
			_HOST[key] = random_spd_graph(20000, 16.0, seed=11, dtype=dtype)
		else:
			_HOST[key] = dense_spd(640, seed=5, dtype=dtype)
	return _HOST[key]


def make_operator(eng, kind, dtype):
	"""(host matrix, DeviceOperator, keep-alive) for an operator kind: the four matrices as they are, a host callback and a
	TorchOperator around the dense one."""
	if kind == "callback":
		from scipy.sparse.linalg import aslinearoperator

		A = host_matrix("dense", dtype)
		return A, eng.DeviceOperator(aslinearoperator(A)), None
	if kind == "torch":
		import torch

		from primate_amd.operators import TorchOperator

		A = host_matrix("dense", dtype)
		At = torch.tensor(np.ascontiguousarray(A), device="cuda")
		T = TorchOperator(lambda X: At @ X, A.shape[0], dtype=dtype) if dtype != np.float64 else TorchOperator(lambda X: At @ X, A.shape[0])
		return A, eng.DeviceOperator(T), At
	A = host_matrix(kind, dtype)
	return A, eng.DeviceOperator(A), None


## (operator, dtype, probes, deg, orth, SLQ_TILES): every operator kind, every panel width, both dtypes and every (deg, orth)
## pair at least once; 40^3 fp64 at every pair; the grids with the ring-fed passes forced (SLQ_TILES=2) and without
CASES = [
	("lap3d", np.float64, 256, 30, 0, "2"),
	("lap3d", np.float64, 130, 30, 3, "2"),
	("lap3d", np.float64, 32, 50, 10, None),
	("lap3d", np.float64, 5, 120, 3, None),
	("lap3d", np.float64, 32, 40, 40, "2"),
	("lap3d", np.float64, 32, 200, 3, "2"),
	("lap3d", np.float32, 130, 50, 10, "2"),
	("lap2d", np.float32, 256, 30, 3, "2"),
	("lap2d", np.float64, 130, 50, 10, None),
	("lap2d", np.float32, 5, 120, 3, None),
	("graph", np.float64, 32, 30, 3, None),
	("graph", np.float32, 130, 40, 40, None),
	("dense", np.float64, 32, 50, 10, None),
	("dense", np.float32, 256, 30, 0, None),
	("callback", np.float64, 5, 30, 3, None),
	("torch", np.float64, 32, 30, 3, None),
]  # fmt: skip


def _case_id(c):
	return f"{c[0]}-{np.dtype(c[1]).name}-P{c[2]}-k{c[3]}-o{c[4]}-tiles{c[5]}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_replay_is_exact_and_meets_the_kept_basis_at_the_derived_bound(eng, monkeypatch, case):
	"""A: on a recompute plan the Jacobi matrix after run() and after fun_action() is the same array, two actions give the
	same array, quadrature() before and after an action is the same array, and SLQ_ACC_SKIP=0 changes no bit - the replay's
	sums are taken in the fixed order of the run.
	B: premise - the recompute plan's Jacobi matrix is array_equal to that of a keep_basis plan with the same arguments and
	probes (the slot count moves where a vector is stored, not what is computed). Then both outputs are the same sum of the same
	deg terms taken in opposite orders, each partial sum rounded once: |Y_rec - Y_keep| <= deg eps_F sum_t |g_t| |W_t[row]|
	elementwise; the right-hand side is evaluated in fp64 from the kept plan, and twice it is allowed for the one rounding of
	each g_t to F. Nothing here is measured."""
	kind, dtype, P, deg, orth, tiles = case
	if tiles is not None:
		monkeypatch.setenv("SLQ_TILES", tiles)
	A, op, keep_alive = make_operator(eng, kind, dtype)
	n = A.shape[0]
	rng = np.random.default_rng(100 + P + deg)
	X = np.asfortranarray(rng.standard_normal((n, P)), dtype=dtype)
	eps = float(np.finfo(dtype).eps)
	fun, kw = "exp", {"t": -0.1}

	rec = eng.LanczosPlan(op, P, deg, orth, basis="recompute")
	info = rec.basis_info()
	ring_only = 2 if rec.orth == 0 else max(rec.orth + 1, 3)
	assert info["mode"] == 2 and info["acc_cols"] == min(8, rec.deg), info
	assert ring_only <= info["ring_slots"] <= ring_only + 8 and info["ring_slots"] >= info["acc_cols"] + 1, info
	if tiles == "2" and kind in ("lap2d", "lap3d"):
		assert rec.describe()["tiles"] == 2, rec.describe()
	rec.set_probes(X)
	rec.run()
	t_run = rec.tridiag()
	q_before = rec.quadrature(fun, **kw)
	Y1 = rec.fun_action(fun, **kw)
	t_act = rec.tridiag()
	q_after = rec.quadrature(fun, **kw)
	Y2 = rec.fun_action(fun, **kw)
	assert all(np.array_equal(a, b) for a, b in zip(t_run, t_act)), "the replay changed the Jacobi matrix"
	assert np.array_equal(q_before, q_after)
	assert np.array_equal(Y1, Y2)
	assert np.all(np.isfinite(Y1))
	with pytest.raises(ValueError):
		rec.basis(0)
	with pytest.raises(ValueError):
		rec.run(upto=1)
	rec.close()

	monkeypatch.setenv("SLQ_ACC_SKIP", "0")
	rec0 = eng.LanczosPlan(op, P, deg, orth, basis="recompute")
	monkeypatch.delenv("SLQ_ACC_SKIP")
	rec0.set_probes(X)
	rec0.run()
	Y0 = rec0.fun_action(fun, **kw)
	rec0.close()
	assert np.array_equal(Y0, Y1), "SLQ_ACC_SKIP=0 changed bits"

	keep = eng.LanczosPlan(op, P, deg, orth, keep_basis=True)
	keep.set_probes(X)
	keep.run()
	t_keep = keep.tridiag()
	assert all(np.array_equal(a, b) for a, b in zip(t_run, t_keep)), "premise of B: the two plan kinds compute different Jacobi matrices"
	Yk = keep.fun_action(fun, **kw)
	a, b, steps = t_keep
	worst = 0.0
	## every 8th column, the last one, and the columns either side of a panel boundary (P = 130: the padded tail panel)
	for i in sorted(set(range(0, P, 8)) | {P - 1} | {c for c in (63, 64, 127, 128) if c < P}):
		Q = keep.basis(i)
		c = action_coeffs(a[i], b[i], rec.deg, f_exp)
		bound = 2.0 * order_bound(Q, c, np.linalg.norm(X[:, i].astype(np.float64)), rec.deg, eps)
		diff = np.abs(Y1[:, i].astype(np.float64) - Yk[:, i].astype(np.float64))
		worst = max(worst, float(np.max(diff / np.maximum(bound, 1e-300))))
		assert np.all(diff <= bound), (i, float(np.max(diff)), float(np.max(diff / np.maximum(bound, 1e-300))))
	print(f"{_case_id(case)}: max |Y_rec - Y_keep| / bound over the columns checked = {worst:.3e}")
	keep.close()
	op.close()


def test_accumulation_skips_columns_past_an_early_stop(eng, monkeypatch):
	"""An operator with five distinct eigenvalues: every Krylov space has dimension <= 5, so every probe of every panel stops
	after 5 of the 20 steps and the coefficients of the later columns are zero for whole panels. The accumulation launches do
	not read those columns - the first launch holds dead columns beside live ones, the later launches are dead altogether -
	which slq_plan_action_columns counts; SLQ_ACC_SKIP=0 reads every column offered and gives the same bits (the columns past
	the stop are finite, 0 * x adds nothing); both equal f(A) X, which the 5-step Krylov space holds exactly (the
	tolerances of the dense-eigendecomposition check), and the kept basis at rel 1e-9."""
	import scipy.sparse as sp

	n, P, deg = 6000, 130, 20
	rng = np.random.default_rng(21)
	d = rng.integers(1, 6, n).astype(np.float64)
	A = sp.diags(d).tocsr()
	X = np.asfortranarray(rng.standard_normal((n, P)))
	op = eng.DeviceOperator(A)
	res = {}
	for skip in ("1", "0"):
		monkeypatch.setenv("SLQ_ACC_SKIP", skip)
		plan = eng.LanczosPlan(op, P, deg, 3, basis="recompute")
		panels = plan.describe()["panels"]
		plan.set_probes(X)
		plan.run()
		steps = plan.tridiag()[2]
		plan.action_columns()
		Y = plan.fun_action("exp", t=-0.1)
		cols = plan.action_columns()
		res[skip] = (Y, cols, plan.tridiag())
		plan.close()
		assert np.all(steps <= 6) and np.all(steps >= 5), steps
	monkeypatch.delenv("SLQ_ACC_SKIP")
	(Y1, (rd1, off1), t1), (Y0, (rd0, off0), t0) = res["1"], res["0"]
	print(f"accumulation columns read / offered: skipping {rd1} / {off1}, SLQ_ACC_SKIP=0 {rd0} / {off0} ({panels} panels)")
	assert off1 == off0 == deg * panels and rd0 == off0
	assert 0 < rd1 <= 7 * panels < off1, (rd1, off1)  # (the columns up to the stop, and the residual column of the stopping step)
	assert np.array_equal(Y1, Y0) and all(np.array_equal(a, b) for a, b in zip(t1, t0))
	assert np.all(np.isfinite(Y1))
	np.testing.assert_allclose(Y1, np.exp(-0.1 * d)[:, None] * X, rtol=1e-8, atol=1e-9)
	keep = eng.LanczosPlan(op, P, deg, 3, keep_basis=True)
	keep.set_probes(X)
	keep.run()
	np.testing.assert_allclose(Y1, keep.fun_action("exp", t=-0.1), rtol=1e-9, atol=1e-12)
	keep.close()
	op.close()


def test_recompute_action_against_dense_eigendecomposition(eng, golden):
	"""test_fun_action_against_dense_eigendecomposition over recompute plans, at that test's tolerances: M @ v == U f(L) U^T v for
	deg = n (rtol 1e-8, atol 1e-9), and the reference's MatrixFunction._matvec on the Laplacian (golden, rtol 1e-9, atol 1e-10)."""
	rng = np.random.default_rng(1234)
	n = 60
	B = rng.standard_normal((n, n))
	A = B @ B.T / n + 0.5 * np.eye(n)
	ew, ev = np.linalg.eigh(A)
	X = np.asfortranarray(rng.uniform(-1, 1, (n, 4)))
	op = eng.DeviceOperator(A)
	plan = eng.LanczosPlan(op, 4, n, n, basis="recompute")
	assert plan.basis_mode == 2
	for fun, kw, f in [("identity", {}, lambda x: x), ("log", {}, np.log), ("exp", {"t": -0.3}, lambda x: np.exp(-0.3 * x)), ("inv", {}, lambda x: 1 / x), ("sqrt", {}, np.sqrt)]:
		plan.set_probes(X)
		plan.run()
		Y = plan.fun_action(fun, **kw)
		np.testing.assert_allclose(Y, (ev * f(ew)) @ ev.T @ X, rtol=1e-8, atol=1e-9, err_msg=fun)
	## several functions off ONE run: every action replays from the stash
	for fun, kw, f in [("inv", {}, lambda x: 1 / x), ("identity", {}, lambda x: x)]:
		np.testing.assert_allclose(plan.fun_action(fun, **kw), (ev * f(ew)) @ ev.T @ X, rtol=1e-8, atol=1e-9, err_msg=fun)
	L = laplacian_2d(int(golden["lap_m"]))
	V = golden["lap_probes"][:, :4]
	plan = eng.LanczosPlan(eng.DeviceOperator(L), 4, 20, 20, basis="recompute")
	plan.set_probes(V)
	plan.run()
	np.testing.assert_allclose(plan.fun_action("exp", t=-0.1), golden["mf_matvec_exp_t"], rtol=1e-9, atol=1e-10)
	np.testing.assert_allclose(plan.fun_action("identity"), L @ V, rtol=1e-9, atol=1e-9)  # A v is in the Krylov space: exact


def test_one_call_fun_action_batch_recompute(eng):
	"""test_one_call_fun_action_batch with basis="recompute", at that test's tolerances: against the dense eigendecomposition
	at deg = n (rtol 1e-7, atol 1e-8 there), against the plan-based route it wraps (rtol 1e-12, atol 1e-13), and deg = 200 > 141 -
	the eigenvectors in global scratch - at that check's rtol 1e-8, atol 1e-9."""
	L = random_spd_graph(90, 5.0, seed=4)
	n = L.shape[0]
	rng = np.random.default_rng(2)
	X = np.asfortranarray(rng.standard_normal((n, 11)))
	w, U = np.linalg.eigh(L.toarray())
	op = eng.DeviceOperator(L)
	for fun, kw, f in [("exp", {"t": -0.2}, lambda x: np.exp(-0.2 * x)), ("inv", {}, lambda x: 1 / x), ("identity", {}, lambda x: x)]:
		Y, used = eng.fun_action_batch(op, X, deg=n, orth=n, fun=fun, basis="recompute", return_basis=True, **kw)
		assert used == "recompute"
		np.testing.assert_allclose(Y, (U * f(w)) @ (U.T @ X), rtol=1e-7, atol=1e-8)
	plan = eng.LanczosPlan(op, 11, 25, 5, basis="recompute")
	plan.set_probes(X)
	plan.run()
	np.testing.assert_allclose(eng.fun_action_batch(op, X, deg=25, orth=5, fun="exp", t=-0.2, basis="recompute"), plan.fun_action("exp", t=-0.2), rtol=1e-12, atol=1e-13)
	with pytest.raises(ValueError):
		eng.fun_action_batch(op, X[:5], deg=10, basis="recompute")
	A2 = random_spd_graph(400, 6.0, seed=8)
	w2, U2 = np.linalg.eigh(A2.toarray())
	X2 = np.asfortranarray(rng.standard_normal((400, 5)))
	Y2 = eng.fun_action_batch(eng.DeviceOperator(A2), X2, deg=200, orth=200, fun="exp", t=-0.3, basis="recompute")
	ref2 = (U2 * np.exp(-0.3 * w2)) @ (U2.T @ X2)
	print(f"deg 200 on recompute plans: max |Y - ref| = {float(np.max(np.abs(Y2 - ref2))):.3e}, max rel = {float(np.max(np.abs(Y2 - ref2) / np.abs(ref2))):.3e}")
	np.testing.assert_allclose(Y2, ref2, rtol=1e-8, atol=1e-9)


def test_drivers_over_a_recompute_matrix_function(golden):
	"""The golden checks of test_drivers_over_matrix_function over MatrixFunction(..., basis="recompute") at that test's
	tolerances (rtol 1e-8 for diag and hutchpp, 1e-7 for xtrace), and every driver with basis="recompute" against the same call
	with basis="keep", same seed, at rel 1e-9 - the bar test_hutchpp_device_path_matches_host_algebra sets for the same algebra
	by another route."""
	from scipy.linalg import expm

	from primate_amd.diagonal import diag, xdiag
	from primate_amd.operators import MatrixFunction
	from primate_amd.trace import hutchpp, xtrace

	gd = np.load(ROOT / "tests" / "golden" / "slq_golden_drivers.npz")
	L = laplacian_2d(int(gd["lap_m"]))
	M = MatrixFunction(L, fun="exp", deg=20, orth=20, t=-0.1, basis="recompute")
	K = MatrixFunction(L, fun="exp", deg=20, orth=20, t=-0.1, basis="keep")
	d_dev = diag(M, converge="count", count=30, seed=1234, batch=8)
	assert M.basis_used == "recompute"
	np.testing.assert_allclose(d_dev, gd["mf_diag_c30"], rtol=1e-8)
	d_host = diag(M, converge="count", count=30, seed=1234, record=True)
	np.testing.assert_allclose(d_host, gd["mf_diag_c30"], rtol=1e-8)
	assert hutchpp(M, m=24, seed=1234, mode="full") == pytest.approx(float(gd["mf_hutchpp_m24_full"]), rel=1e-8)
	M0 = MatrixFunction(L, fun="exp", deg=20, orth=0, t=-0.1, basis="recompute")
	K0 = MatrixFunction(L, fun="exp", deg=20, orth=0, t=-0.1)
	assert hutchpp(M0, m=24, seed=1234) == pytest.approx(float(gd["mf0_hutchpp_m24"]), rel=1e-8)
	assert xtrace(M, batch=12, seed=1234) == pytest.approx(float(gd["mf_xtrace_b12"]), rel=1e-7)
	F = expm(-0.1 * L.toarray())
	np.testing.assert_allclose(xdiag(M, m=40, seed=11), xdiag(F, m=40, seed=11), rtol=1e-7, atol=1e-9)
	## the same call on the two plan kinds
	np.testing.assert_allclose(d_dev, diag(K, converge="count", count=30, seed=1234, batch=8), rtol=1e-9)
	assert K.basis_used == "keep"
	for mode in ("full", "reduced"):
		assert hutchpp(M, m=24, seed=1234, mode=mode) == pytest.approx(hutchpp(K, m=24, seed=1234, mode=mode), rel=1e-9)
	assert hutchpp(M0, m=24, seed=1234) == pytest.approx(hutchpp(K0, m=24, seed=1234), rel=1e-9)
	assert xtrace(M, batch=12, seed=1234) == pytest.approx(xtrace(K, batch=12, seed=1234), rel=1e-9)
	np.testing.assert_allclose(xdiag(M, m=40, seed=11), xdiag(K, m=40, seed=11), rtol=1e-9)
	v = np.random.default_rng(3).standard_normal(L.shape[0])
	np.testing.assert_allclose(M @ v, K @ v, rtol=1e-9, atol=1e-12)
	with pytest.raises(ValueError, match="callable"):
		MatrixFunction(L, fun=np.exp, deg=20, basis="recompute")


def test_sharded_diag_device_on_recompute_plans(eng):
	"""sharded_diag_device(basis="recompute") in a world of one: the pooled numer / denom of the kept-basis call, same probes."""
	from primate_amd.distributed import sharded_diag_device

	L = laplacian_2d(40)
	op = eng.DeviceOperator(L)
	keep = sharded_diag_device(op, 48, 20, 3, fun="exp", seed=7, batch=32, t=-0.1)
	rec = sharded_diag_device(op, 48, 20, 3, fun="exp", seed=7, batch=32, basis="recompute", t=-0.1)
	assert rec[3] == keep[3] == 48
	assert np.array_equal(rec[2], keep[2])  # denom: v * v of the same probes
	np.testing.assert_allclose(rec[1], keep[1], rtol=1e-9, atol=1e-12)
	with pytest.raises(ValueError, match="auto"):
		sharded_diag_device(op, 48, 20, 3, basis="auto")


def test_auto_picks_the_kept_basis_when_it_fits_and_recompute_otherwise(eng, monkeypatch):
	"""E: with the free memory reported to Python patched, MatrixFunction(basis="auto") takes the kept basis when its plan
	(+ 1 GiB) fits and a recompute plan for the whole column count when only that fits; M.basis_used says which.
	slq_fAv_batch_mode(0) on a small operator equals, bit for bit, the mode it reports having taken."""
	from primate_amd.operators import MatrixFunction

	L = laplacian_2d(60)
	n = L.shape[0]
	rng = np.random.default_rng(9)
	X = np.asfortranarray(rng.standard_normal((n, 24)))
	M = MatrixFunction(L, fun="exp", deg=30, orth=3, t=-0.1, basis="auto")
	keep_bytes = eng.plan_query_bytes(np.float64, n, 24, 30, 3, "keep")
	rec_bytes = eng.plan_query_bytes(np.float64, n, 24, 30, 3, "recompute")
	assert rec_bytes < keep_bytes
	total = M._op.ctx.meminfo()[1]
	monkeypatch.setattr(eng.Context, "meminfo", lambda self: (keep_bytes + (1 << 30), total))
	Yk = M @ X
	assert M.basis_used == "keep"
	assert M._plan(24, True).basis_mode == 1
	monkeypatch.setattr(eng.Context, "meminfo", lambda self: (keep_bytes + (1 << 30) - 1, total))
	M2 = MatrixFunction(L, fun="exp", deg=30, orth=3, t=-0.1, basis="auto")
	Yr = M2 @ X
	assert M2.basis_used == "recompute"
	plan = M2._plan(24, True)
	assert plan.basis_mode == 2 and plan.nprobes == 24  # the whole column count on one recompute plan
	monkeypatch.undo()
	ref_k = MatrixFunction(L, fun="exp", deg=30, orth=3, t=-0.1, basis="keep") @ X
	ref_r = MatrixFunction(L, fun="exp", deg=30, orth=3, t=-0.1, basis="recompute") @ X
	assert np.array_equal(Yk, ref_k) and np.array_equal(Yr, ref_r)
	np.testing.assert_allclose(Yr, Yk, rtol=1e-9, atol=1e-12)
	## a callable needs the basis on the host: "auto" means "keep" for it
	Mc = MatrixFunction(L, fun=lambda x: np.exp(-0.1 * x), deg=30, orth=3, basis="auto")
	np.testing.assert_allclose(Mc @ X[:, :2], Yk[:, :2], rtol=1e-8, atol=1e-10)
	assert Mc.basis_used == "keep"
	op = eng.DeviceOperator(L)
	Y0, used = eng.fun_action_batch(op, X, 30, 3, fun="exp", t=-0.1, basis="auto", return_basis=True)
	Y1 = eng.fun_action_batch(op, X, 30, 3, fun="exp", t=-0.1, basis="keep")
	Y2 = eng.fun_action_batch(op, X, 30, 3, fun="exp", t=-0.1, basis="recompute")
	assert used == "keep"  # (14 MB of basis: it fits whatever else runs on the device)
	assert np.array_equal(Y0, {"keep": Y1, "recompute": Y2}[used])
	assert np.array_equal(Y1, eng.fun_action_batch(op, X, 30, 3, fun="exp", t=-0.1))  # the default stays the kept basis
	np.testing.assert_allclose(Y2, Y1, rtol=1e-9, atol=1e-12)


def _full_size_checks(eng, oracle, m, P):
	"""D at grid size m^3 with P device-drawn Rademacher probes, k = 50, orth 3, exp(-0.1 x)."""
	k, orth = 50, 3
	n = m**3
	rec_bytes = eng.plan_query_bytes(np.float64, n, P, k, orth, "recompute")
	keep16 = eng.plan_query_bytes(np.float64, n, 16, k, orth, "keep")
	A = laplacian_3d(m)
	op = eng.DeviceOperator(A)
	free, total = op.ctx.meminfo()
	need = rec_bytes + keep16 + (4 << 30)
	if need > free:
		op.close()
		pytest.skip(f"needs {need / GB:.1f} GB of device memory, {free / GB:.1f} GB of {total / GB:.1f} GB free")
	quad = eng.LanczosPlan(op, P, k, orth)
	dq = quad.describe()
	quad.close()
	plan = eng.LanczosPlan(op, P, k, orth, basis="recompute")
	d = plan.describe()
	assert plan.basis_mode == 2
	assert (d["tiles"], d["sequence"], d["panel_width"]) == (dq["tiles"], dq["sequence"], dq["panel_width"]), (d, dq)
	assert d["tiles"] == 2, d  # the ring-fed default path of this operator
	print(f"workspace: {plan.workspace_bytes / GB:.2f} GB recompute; a kept basis would hold {eng.plan_query_bytes(np.float64, n, P, k, orth, 'keep') / GB:.1f} GB")
	assert plan.workspace_bytes <= 58 * GB
	assert 200 * GB < eng.plan_query_bytes(np.float64, n, P, k, orth, "keep") < 215 * GB
	plan.generate_probes("rademacher", seed=1234)
	V = plan.get_probes()
	plan.run()
	q = plan.quadrature("exp", t=-0.1)
	a, b, steps = plan.tridiag()
	assert np.all(steps == k)
	Y = plan.fun_action("exp", t=-0.1)
	np.testing.assert_allclose(np.einsum("ij,ij->j", V, Y), q, rtol=1e-8)  # v^T (f(A) v) == the plan's own quadrature

	def oracle_action(v):
		al, be, Q = np.zeros(k + 1), np.zeros(k + 1), np.zeros((n, k), order="F")
		assert oracle.lanczos(A, v.copy(), k, 1e-8, orth, al, be, Q) == k
		th, Yv = np.linalg.eigh(np.diag(al[:k]) + np.diag(be[1:k], 1) + np.diag(be[1:k], -1))
		return np.linalg.norm(v) * (Q @ (Yv @ (np.exp(-0.1 * th) * Yv[0, :])))

	refs = {c: oracle_action(np.ascontiguousarray(V[:, c])) for c in (0, P - 1)}
	## the parent's route beside it: a 16-probe kept-basis plan on the same operator and seed must meet the same bar on column 0
	kp = eng.LanczosPlan(op, 16, k, orth, keep_basis=True)
	kp.generate_probes("rademacher", seed=1234)
	assert np.array_equal(kp.get_probes()[:, 0], V[:, 0])
	kp.run()
	Yk = kp.fun_action("exp", t=-0.1)
	kp.close()
	err_keep = float(np.max(np.abs(Yk[:, 0] - refs[0])) / np.abs(refs[0]).max())
	errs = {c: float(np.max(np.abs(Y[:, c] - refs[c])) / np.abs(refs[c]).max()) for c in refs}
	print(f"max |Y - oracle| / max|oracle|: recompute {errs}, kept basis (16 probes) column 0 {err_keep:.3e}")
	np.testing.assert_allclose(Yk[:, 0], refs[0], rtol=0, atol=1e-9 * np.abs(refs[0]).max())
	for c in refs:
		np.testing.assert_allclose(Y[:, c], refs[c], rtol=0, atol=1e-9 * np.abs(refs[c]).max())
	del refs, Yk
	acc = eng.DiagAccumulator(n, ctx=op.ctx)
	acc.update(plan, "exp", t=-0.1)
	numer, denom, _, cnt = acc.get()
	acc.close()
	assert cnt == P and np.all(denom == P)
	np.testing.assert_allclose(numer.sum() / P, q.mean(), rtol=1e-8)
	assert all(np.array_equal(x, y) for x, y in zip((a, b, steps), plan.tridiag()))
	plan.close()
	del Y, V
	## k = 120: no kept basis of it exists on this device (computed, never allocated); the recompute plan is the same size
	k2 = 120
	assert eng.plan_query_bytes(np.float64, n, P, k2, orth, "keep") > 288 * GB
	assert 490 * GB < eng.plan_query_bytes(np.float64, n, P, k2, orth, "keep") < 500 * GB
	assert eng.plan_query_bytes(np.float64, n, P, k2, orth, "recompute") == rec_bytes
	plan = eng.LanczosPlan(op, P, k2, orth, basis="recompute")
	assert plan.workspace_bytes <= 58 * GB
	plan.generate_probes("rademacher", seed=1234)
	plan.run()
	t_run = plan.tridiag()
	assert np.all(t_run[2] == k2)
	q1 = plan.quadrature("exp", t=-0.1)
	Y1 = plan.fun_action("exp", t=-0.1)
	t_act = plan.tridiag()
	q2 = plan.quadrature("exp", t=-0.1)
	Y2 = plan.fun_action("exp", t=-0.1)
	assert all(np.array_equal(x, y) for x, y in zip(t_run, t_act))
	assert np.array_equal(q1, q2) and np.array_equal(Y1, Y2) and np.all(np.isfinite(Y1))
	plan.close()
	op.close()


def test_full_size_126_cubed_on_one_recompute_plan(eng, oracle):
	"""D - the point of the feature: the 126^3 7-point Laplacian, fp64, 256 device-drawn Rademacher probes, k = 50, orth 3,
	exp(-0.1 x) on ONE plan of <= 58 GB (a kept basis: 209 GB) that runs the ring-fed default path of a quadrature plan;
	columns 0 and 255 against the oracle's kept-basis recurrence at the bar of test_config3_estrada_index_full_size
	(atol = 1e-9 max|ref|), with a 16-probe keep_basis plan beside it at the same bar; v^T Y equals the plan's quadrature to
	rtol 1e-8; the diagonal accumulator on the plan; then k = 120 - 496 GB kept, the same bytes recomputed - where only the
	replay's exactness and steps == 120 are checked (at that depth with orth 3 an oracle comparison measures lost
	orthogonality, which the lost-orthogonality tests own). Skips, with the numbers, when the device does not have the memory
	free."""
	_full_size_checks(eng, oracle, 126, 256)
