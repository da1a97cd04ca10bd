"""The closing tail of a run ("the closing tail"): the update pass of step deg - 1 and the scalar kernel behind it
are left out of a run that reaches deg, on plans where that pass stores nothing, and launched by the first entry that reads
what they write. Needs a real MI355X (`-m gpu`).

Every comparison is between the same plan created under the default switches and under SLQ_LAST_STORE=2 (the launch sequence
of the run with nothing left out: the switch table keeps one line for the last update pass, and the closing tail is a value of
that switch) and is np.array_equal: the tail is the same two launches with the same arguments on the same stream, only later,
so there is no tolerance to state. Launch counts are read from the plan's per-kernel events.

Shapes: laplacian_2d(100) and laplacian_3d(22) under SLQ_TILES=2 (ring-fed Gram plans, the smallest the tiles accept) and the
24^2 grid of the golden vectors on the generic passes; 130 probes (two panels, the second ragged), 64 and 32 (merged tiles);
deg 6-12; orth 0, 3, 6 and orth = deg; fp64 and fp32; with the per-kernel events on and off (graph replay)."""

import numpy as np
import pytest
import scipy.sparse as sp

import _omega_cases as oc
from conftest import laplacian_2d, laplacian_3d

pytestmark = pytest.mark.gpu

KEYS = ("SLQ_LAST_STORE", "SLQ_GRAM", "SLQ_OMEGA", "SLQ_OMEGA_TRIP", "SLQ_OMEGA_RESCUE")


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


@pytest.fixture(scope="module")
def ops(golden):
	"""Operators by (name, dtype), made on first use: "lap2d" / "lap3d" under SLQ_TILES=2, "grid24" and the diagonal ones as the
	default switches make them (no tiles: the generic passes)."""
	import os

	made = {}

	def get(eng, name, dtype=np.float64):
		key = (name, np.dtype(dtype).name)
		if key not in made:
			had = os.environ.get("SLQ_TILES")
			if name in ("lap2d", "lap3d"):
				os.environ["SLQ_TILES"] = "2"
			else:
				os.environ.pop("SLQ_TILES", None)
			try:
				A = {"lap2d": lambda: laplacian_2d(100), "lap3d": lambda: laplacian_3d(22), "grid24": lambda: laplacian_2d(int(golden["lap_m"])),
				     "diag5": lambda: distinct_diagonal(5), "diag8": lambda: distinct_diagonal(8)}[name]()  # fmt: skip
				made[key] = (A, eng.DeviceOperator(A.astype(dtype)))
			finally:
				if had is None:
					os.environ.pop("SLQ_TILES", None)
				else:
					os.environ["SLQ_TILES"] = had
		return made[key]

	yield get
	for _, op in made.values():
		op.close()


def distinct_diagonal(m, n=600):
	"""A diagonal operator with exactly m distinct eigenvalues 1 .. m: a Krylov space of dimension m for any probe that meets
	every eigenspace, so the Lanczos run breaks down after exactly m steps."""
	A = sp.diags(1.0 + (np.arange(n) % m).astype(np.float64)).tocsr()
	A.sort_indices()
	return A


def make_plan(eng, monkeypatch, name, op, P, deg, orth, lazy, env=None, **kw):
	"""A plan created with the closing tail left to its first request (lazy = 1: the default) or kept in the run (lazy = 0:
	SLQ_LAST_STORE=2), under `env` (the other switches of KEYS unset); SLQ_TILES as the operator was made."""
	for k in KEYS:
		monkeypatch.delenv(k, raising=False)
	if name in ("lap2d", "lap3d"):
		monkeypatch.setenv("SLQ_TILES", "2")
	else:
		monkeypatch.delenv("SLQ_TILES", raising=False)
	if not lazy:
		monkeypatch.setenv("SLQ_LAST_STORE", "2")
	for k, v in (env or {}).items():
		monkeypatch.setenv(k, str(v))
	plan = eng.LanczosPlan(op, P, deg, orth, **kw)
	for k in KEYS:
		monkeypatch.delenv(k, raising=False)
	return plan


def update_class(orth):
	return "axpy_norm" if orth == 0 else "reorth_update"


def launches(plan):
	return {k: v["launches"] for k, v in plan.profile_read(reset=True).items()}


## (operator, dtype, probes, deg, orth, switches, the sequence describe() names, the plan has a lazy tail)
CASES = [
	("lap2d", np.float64, 130, 12, 3, {}, "fused_gram", True),  # ring-fed Gram with the edge recurrence, two panels
	("lap2d", np.float64, 64, 7, 3, {}, "fused_gram", True),  # merged tiles, 32 lanes per row
	("lap2d", np.float32, 32, 6, 6, {}, "fused_gram", True),  # orth = deg on the deep form, fp32
	("lap2d", np.float64, 130, 12, 12, {}, "fused_gram", False),  # orth = deg > 8: the closing step is on the sweeps
	("lap2d", np.float64, 130, 9, 3, {"SLQ_GRAM": 0}, "fused", True),  # the merged sequence on k_ring_pass
	("lap3d", np.float64, 130, 9, 6, {}, "fused_gram", True),  # deep window
	("lap3d", np.float32, 32, 8, 0, {}, "fused", True),  # orth 0: alpha pass, update pass
	("lap3d", np.float64, 64, 10, 3, {"SLQ_OMEGA": 0}, "fused_gram", True),
	("grid24", np.float64, 130, 12, 3, {}, "fused_gram", True),  # the Gram sequence on the generic passes
	("grid24", np.float64, 64, 10, 6, {}, "fused_gram", True),
	("grid24", np.float32, 32, 8, 0, {}, "fused", True),
	("grid24", np.float64, 32, 10, 3, {"SLQ_GRAM": 0}, "fused", True),  # merged alpha+dots pass, update pass
	("grid24", np.float32, 130, 6, 6, {}, "fused_gram", True),
	("grid24", np.float64, 32, 7, 3, {"SLQ_LAST_STORE": 1}, "fused_gram", False),  # the closing pass stores: nothing is left out
]


@pytest.mark.parametrize("prof", [False, True], ids=["graph", "events"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{np.dtype(c[1]).name}-P{c[2]}-k{c[3]}-o{c[4]}" + "".join(f"-{k[4:].lower()}{v}" for k, v in c[5].items()))
def test_lazy_equals_eager(eng, monkeypatch, ops, case, prof):
	"""quadrature after run, then tridiag (beta_deg and steps included), then another quadrature: np.array_equal between the two
	switch values. closing() says pending until tridiag() and not after; the quadrature does not launch the tail, tridiag()
	launches exactly the update pass and one finalize kernel, a second tridiag() launches nothing."""
	name, dtype, P, deg, orth, env, sequence, has_tail = case
	A, op = ops(eng, name, dtype)
	X = oc.rademacher(A.shape[0], P, 7 + P + deg, dtype)
	upd = update_class(orth)
	res = {}
	for lazy in (1, 0):
		plan = make_plan(eng, monkeypatch, name, op, P, deg, orth, lazy, env)
		assert plan.describe()["sequence"] == sequence, plan.describe()
		expect = bool(lazy) and has_tail
		assert plan.closing() == {"lazy": expect, "pending": False}
		plan.profile_enable(prof)
		plan.set_probes(X)
		launches(plan)  # (the norm sweep of the probes is of class axpy_norm too)
		plan.run()
		assert plan.closing() == {"lazy": expect, "pending": expect}
		q = plan.quadrature("log")
		assert plan.closing()["pending"] == expect  # the quadrature reads alpha[0 .. deg) and beta[1 .. deg) only
		plan.describe()
		n_run = launches(plan)
		assert plan.closing()["pending"] == expect  # ... and neither describe() nor profile_read() asks for the tail
		a, b, s = plan.tridiag()
		assert plan.closing() == {"lazy": expect, "pending": False}
		n_tri = launches(plan)
		a2, b2, s2 = plan.tridiag()
		n_tri2 = launches(plan)
		q2 = plan.quadrature("exp", t=-0.1)
		plan.profile_enable(False)
		plan.close()
		assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(s, s2)
		assert np.all(s == deg) and np.all(b[:, deg] > 0), (s, b[:, deg])  # (a grid Laplacian does not break down in 12 steps)
		if prof:
			if has_tail:  # (the other two: one launch per step with SLQ_LAST_STORE=1, several per step on the sweeps)
				assert n_run[upd] == (deg - 1 if expect else deg), n_run
			assert n_tri[upd] == (1 if expect else 0) and n_tri["finalize"] == (1 if expect else 0), n_tri
			assert sum(n_tri.values()) == (2 if expect else 0) and sum(n_tri2.values()) == 0, (n_tri, n_tri2)
		res[lazy] = (q, a, b, s, q2, n_run)
	for x, y in zip(res[1][:5], res[0][:5]):
		assert np.array_equal(x, y)
	if prof:  # everything in front of the closing update pass is launched as before
		one, zero = res[1][5], res[0][5]
		gone = 1 if has_tail else 0
		assert one["finalize"] == zero["finalize"] - gone and one[upd] == zero[upd] - gone
		assert all(one[k] == zero[k] for k in one if k not in ("finalize", upd)), (one, zero)


@pytest.mark.parametrize("orth,omega", [(3, 1), (3, 0), (0, 0)])
def test_launch_accounting(eng, monkeypatch, ops, orth, omega):
	"""Over R runs of set_probes -> run -> quadrature the update class has R (deg - 1) launches (R deg with the switch off) and
	finalize one less per run than with the switch off, with the edge recurrence and without it; one tridiag() at the end adds
	exactly one update launch and one finalize launch."""
	A, op = ops(eng, "lap2d")
	P, deg, R = 130, 10, 3
	X = oc.rademacher(A.shape[0], P, 5)
	upd = update_class(orth)
	got = {}
	for lazy in (1, 0):
		plan = make_plan(eng, monkeypatch, "lap2d", op, P, deg, orth, lazy, {"SLQ_OMEGA": omega})
		assert plan.describe()["omega"] == (omega if orth == 3 else 0)
		plan.profile_enable(True)
		plan.profile_read(reset=True)
		for _ in range(R):
			plan.set_probes(X)
			plan.run()
			plan.quadrature("log")
		runs = launches(plan)
		plan.tridiag()
		tri = launches(plan)
		plan.profile_enable(False)
		plan.close()
		got[lazy] = (runs, tri)
	norm = R if orth == 0 else 0  # (set_probes takes the probes' norms by a sweep of class axpy_norm)
	assert got[1][0][upd] == R * (deg - 1) + norm and got[0][0][upd] == R * deg + norm, got
	assert got[1][0]["finalize"] == got[0][0]["finalize"] - R, got
	assert got[1][1][upd] == 1 and got[1][1]["finalize"] == 1 and sum(got[1][1].values()) == 2, got[1][1]
	assert sum(got[0][1].values()) == 0, got[0][1]


@pytest.mark.parametrize("how", ["generate", "set", "close"])
def test_new_probes_drop_the_tail(eng, monkeypatch, ops, how):
	"""run; new probes: nothing is pending, no update pass is launched, and tridiag() raises as it does for a plan that has not
	run. run; close() is clean."""
	A, op = ops(eng, "lap2d")
	P, deg = 130, 8
	X = oc.rademacher(A.shape[0], P, 6)
	plan = make_plan(eng, monkeypatch, "lap2d", op, P, deg, 3, 1)
	plan.profile_enable(True)
	plan.set_probes(X)
	plan.run()
	assert plan.closing() == {"lazy": True, "pending": True}
	launches(plan)
	if how == "close":
		plan.close()
		eng.default_context().synchronize()
		return
	if how == "generate":
		plan.generate_probes("rademacher", seed=3)
	else:
		plan.set_probes(X)
	assert plan.closing() == {"lazy": True, "pending": False}
	n = launches(plan)
	assert n["reorth_update"] == 0 and n["spmm_3term"] == 0 and n["reorth_dot"] == 0, n
	with pytest.raises(ValueError, match="no completed run"):
		plan.tridiag()
	## ... and the plan runs again as a fresh one does
	plan.set_probes(X)
	plan.run()
	again = plan.tridiag()
	plan.profile_enable(False)
	plan.close()
	fresh = make_plan(eng, monkeypatch, "lap2d", op, P, deg, 3, 0)
	fresh.set_probes(X)
	fresh.run()
	ref = fresh.tridiag()
	fresh.close()
	assert all(np.array_equal(x, y) for x, y in zip(again, ref))


@pytest.mark.parametrize("m", [5, 8])
@pytest.mark.parametrize("orth", [3, 0])
def test_stop_rule_at_the_ends(eng, monkeypatch, ops, m, orth):
	"""A diagonal operator with exactly m distinct eigenvalues at deg = 8: the breakdown before the closing step (m = 5) and at
	it (m = 8). steps, beta and the quadrature equal the eager run bit for bit; a probe with NaN entries and an all-zero probe
	give the same numbers, flags or error."""
	deg, P = 8, 32
	A, op = ops(eng, f"diag{m}")
	X = oc.rademacher(A.shape[0], P, 40 + m)
	X[:, 3] = 0.0
	X[5, 7] = np.nan
	res = {}
	for lazy in (1, 0):
		plan = make_plan(eng, monkeypatch, f"diag{m}", op, P, deg, orth, lazy)
		assert plan.closing()["lazy"] == bool(lazy)
		plan.set_probes(X)
		plan.run()
		out = []
		for fun in ("identity", "exp"):
			try:
				out.append(plan.quadrature(fun))
			except Exception as e:  # noqa: BLE001  (the same error from both, if any)
				out.append(np.array([hash((type(e).__name__, str(e)))], dtype=np.float64))
		out += list(plan.tridiag())
		plan.close()
		res[lazy] = out
	for x, y in zip(res[1], res[0]):
		assert np.array_equal(x, y, equal_nan=True), (x, y)
	steps, beta = res[0][4], res[0][3]
	live = np.delete(np.arange(P), [3, 7])
	print(f"CLOSING-STOP m={m} orth={orth}: steps {np.unique(steps[live]).tolist()}, |beta_m| max {np.max(np.abs(beta[live, m])):.2e}, zero probe {steps[3]}, NaN probe {steps[7]}")
	assert np.all(steps[live] == m) and steps[3] == 0, steps


def test_staged_runs(eng, monkeypatch, ops):
	"""run_steps 3 + the rest: only the stage that reaches deg leaves a tail. quadrature_at at m < deg and the Gauss rule at m = deg
	do not launch it, the Gauss-Radau rule at m = deg (its border is beta_deg) does; all equal the eager plan."""
	A, op = ops(eng, "lap2d")
	P, deg = 130, 11
	X = oc.rademacher(A.shape[0], P, 8)
	res = {}
	for lazy in (1, 0):
		plan = make_plan(eng, monkeypatch, "lap2d", op, P, deg, 3, lazy)
		plan.set_probes(X)
		plan.run(upto=3)
		assert plan.closing()["pending"] is False
		mid = plan.tridiag()
		plan.run(upto=deg)
		assert plan.closing()["pending"] == bool(lazy)
		out = [plan.quadrature_at(7, "log"), plan.quadrature_at(7, "log", rule="radau", endpoint=0.0), plan.quadrature_at(deg, "log")]
		assert plan.closing()["pending"] == bool(lazy)
		out.append(plan.quadrature_at(deg, "log", rule="radau", endpoint=0.0))
		assert plan.closing()["pending"] is False
		out += list(mid) + list(plan.tridiag())
		plan.close()
		res[lazy] = out
	for x, y in zip(res[1], res[0]):
		assert np.array_equal(x, y)
	assert not np.array_equal(res[0][2], res[0][3])  # (the Radau value did use its border)


@pytest.mark.parametrize("first", ["columns", "flags", "verify", "census"])
@pytest.mark.parametrize("env", [{}, {"SLQ_OMEGA_RESCUE": 9}, {"SLQ_OMEGA_TRIP": 9}], ids=["plain", "rescue-at-closing", "read-at-closing"])
def test_window_diagnostics(eng, monkeypatch, ops, first, env):
	"""The edge recurrence's counters (offered, read, rescues, transitions), the per-step flags, the verify numbers and the census
	after a run equal the eager plan's, whichever is asked for first - that entry launches the tail. SLQ_OMEGA_RESCUE = deg - 1
	forces the rescue at the closing step, SLQ_OMEGA_TRIP = deg - 1 the read."""
	A, op = ops(eng, "lap2d")
	P, deg = 130, 10
	X = oc.rademacher(A.shape[0], P, 9)
	env = dict(env, **({"SLQ_OMEGA": 2} if first == "census" else {}))
	res = {}
	for lazy in (1, 0):
		plan = make_plan(eng, monkeypatch, "lap2d", op, P, deg, 3, lazy, env)
		assert plan.describe()["omega"] == (2 if first == "census" else 1)
		NP = plan.describe()["panels"]
		plan.window_columns(reset=True)
		plan.set_probes(X)
		plan.run()
		q = plan.quadrature("log")
		assert plan.closing()["pending"] == bool(lazy)
		call = {"columns": plan.window_columns, "flags": plan.window_flags, "verify": plan.window_verify, "census": plan.window_census}
		head = call[first]()
		assert plan.closing()["pending"] is False
		cols, flags, verify = plan.window_columns(), plan.window_flags(), plan.window_verify()
		out = {"q": q, "head": head, "cols": cols, "flags": flags, "verify": verify, "tridiag": plan.tridiag()}
		plan.close()
		res[lazy] = out
	one, zero = res[1], res[0]
	assert one["cols"] == zero["cols"] and one["verify"] == zero["verify"], (one["cols"], zero["cols"])
	assert NP == 2 and zero["cols"]["offered"] == (deg - 2) * NP, zero["cols"]  # steps 2 .. deg - 1, both panels: the closing step is counted
	if "SLQ_OMEGA_RESCUE" in env and first != "census":
		assert zero["cols"]["rescues"] >= NP and np.all(zero["flags"][1][deg - 1] == 1), zero["cols"]
	assert all(np.array_equal(x, y) for x, y in zip(one["flags"], zero["flags"]))
	assert all(np.array_equal(x, y) for x, y in zip(one["tridiag"], zero["tridiag"])) and np.array_equal(one["q"], zero["q"])
	if isinstance(zero["head"], dict):
		assert one["head"] == zero["head"]
	else:
		assert all(np.array_equal(x, y) for x, y in zip(np.atleast_1d(one["head"]), np.atleast_1d(zero["head"])))


@pytest.mark.parametrize("kind", ["keep", "recompute", "last_store", "sweeps"])
def test_plans_that_stay_eager(eng, monkeypatch, ops, kind):
	"""A kept basis, a recompute plan (forward run and replay), SLQ_LAST_STORE=1 and a closing step on the sweeps: closing() reports
	not lazy under either switch value, nothing is ever pending, the update class has deg launches per run, and results - the
	two-pass f(A)v of the recompute plan among them - do not depend on the switch."""
	A, op = ops(eng, "lap2d")
	P, deg = 64, 10
	orth = deg if kind == "sweeps" else 3
	X = oc.rademacher(A.shape[0], P, 12)
	kw = {"basis": kind} if kind in ("keep", "recompute") else {}
	env = {"SLQ_LAST_STORE": 1} if kind == "last_store" else {}
	res = {}
	for lazy in (1, 0):
		plan = make_plan(eng, monkeypatch, "lap2d", op, P, deg, orth, lazy, env, **kw)
		assert plan.closing() == {"lazy": False, "pending": False}
		plan.profile_enable(True)
		plan.set_probes(X)
		plan.run()
		assert plan.closing() == {"lazy": False, "pending": False}
		out = [plan.quadrature("log")]
		n = launches(plan)
		out += list(plan.tridiag())
		assert sum(launches(plan).values()) == 0
		if kw:
			out.append(plan.fun_action("exp", t=-0.1))
			assert plan.closing() == {"lazy": False, "pending": False}
			out += list(plan.tridiag())
		plan.profile_enable(False)
		plan.close()
		res[lazy] = (out, n)
	assert res[1][1] == res[0][1], (res[1][1], res[0][1])
	if kind != "sweeps":
		assert res[0][1]["reorth_update"] == deg, res[0][1]
	for x, y in zip(res[1][0], res[0][0]):
		assert np.array_equal(x, y)


def test_chebyshev_plans_stay_eager(eng, monkeypatch, ops):
	A, op = ops(eng, "lap2d")
	for k in KEYS:
		monkeypatch.delenv(k, raising=False)
	monkeypatch.setenv("SLQ_TILES", "2")
	for action in (False, True):
		plan = eng.ChebyshevPlan(op, 64, 10, action=action)
		plan.generate_probes("rademacher", seed=2)
		assert plan.closing() == {"lazy": False, "pending": False}
		plan.run((0.0, 8.0))
		assert plan.closing() == {"lazy": False, "pending": False}
		assert np.all(np.isfinite(plan.moments()))
		plan.close()


@pytest.mark.parametrize("orth", [3, 0])
def test_affine_operators_stay_eager(eng, monkeypatch, orth):
	"""A + t B has its values rewritten in place by set_parameter, and a deferred update pass would read them again: its plans have
	no lazy tail. run at t1, set_parameter(t2), then tridiag() and the Gauss-Radau rule at m = deg: the beta_deg of t1, equal to
	SLQ_LAST_STORE=2 and to a plan on which t never changed. (An affine operator has no upper copy: the merged sequence at
	orth 3, the separate one at orth 0, both with the no-store bit.)"""
	from primate_amd.operators import AffineOperator

	for k in KEYS + ("SLQ_TILES",):
		monkeypatch.delenv(k, raising=False)
	L = laplacian_2d(24)
	n, P, deg, t1, t2 = L.shape[0], 32, 8, 0.3, 1.7
	B = sp.diags(1.0 + (np.arange(n) % 7) / 7.0).tocsr()
	X = oc.rademacher(n, P, 21)
	op = eng.DeviceOperator(AffineOperator(L, B, t=t1))
	res = {}
	for how in ("default-moved", "eager-moved", "default-still"):
		op.set_parameter(t1)
		plan = make_plan(eng, monkeypatch, "affine", op, P, deg, orth, 0 if how == "eager-moved" else 1)
		assert plan.describe()["sequence"] == "fused" and plan.closing() == {"lazy": False, "pending": False}
		plan.profile_enable(True)
		plan.set_probes(X)
		launches(plan)
		plan.run()
		assert plan.closing() == {"lazy": False, "pending": False}
		assert launches(plan)[update_class(orth)] == deg
		q = plan.quadrature("log")
		if how != "default-still":
			op.set_parameter(t2)
		out = [q, plan.quadrature_at(deg, "log", rule="radau", endpoint=0.0), *plan.tridiag()]
		assert sum(launches(plan).values()) == 2  # (the two quadrature kernels: no pass of the run is launched behind set_parameter)
		plan.profile_enable(False)
		plan.close()
		res[how] = out
	op.close()
	for how in ("eager-moved", "default-still"):
		for x, y in zip(res["default-moved"], res[how]):
			assert np.array_equal(x, y), how
	assert np.all(res["default-moved"][3][:, deg] > 0)
