"""The edge recurrence of the Gram sequence: the update pass of a step with a full window of three columns
reads the window's oldest column only where k_fin_gram could not certify its zero projection from the inner products the step
already has (SLQ_OMEGA: 1 default, 0 every column read, 2 verify). Needs a real MI355X (`-m gpu`).

Bars: SLQ_OMEGA=1 against SLQ_OMEGA=0 on the same plan is np.array_equal on the tridiagonal and the quadrature wherever no rescue
happened (a skipped column carries gamma = 0 in either run, and every non-zero gamma comes from measured inner products); where a
rescue happened another kernel measured the entry in another summation order, and the run is held to the oracle bars of
tests/test_gpu_parity.py: per-probe quadrature of smooth functions 1e-8 relative (fp32: 3e-4), oracle_spread-based for the
ill-conditioned operator. Verify mode must report ZERO violations everywhere."""

import numpy as np
import pytest

import _omega_cases as oc
from conftest import laplacian_2d, laplacian_3d

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def _same(a, b):
	return all(np.array_equal(a[k], b[k]) for k in ("alpha", "beta", "steps", "log", "exp"))


def _tridiag_dist(a, b):
	return max(np.max(np.abs(a[k] - b[k])) / np.max(np.abs(b[k])) for k in ("alpha", "beta"))


def _oracle_bar(oracle, A, X, deg, orth, got, cols, rtol):
	ref = oracle.quad_batch(A, np.asfortranarray(X[:, cols]), deg, orth, fun="log", fresh_q=True)
	err = np.max(np.abs(got["log"][cols] / ref - 1.0))
	assert err <= rtol, f"quadrature {err:.2e} from the oracle (bar {rtol:.0e})"
	return err


GRIDS = {"lap2d_f64": (lambda: laplacian_2d(200), 1e-8), "lap3d_f64": (lambda: laplacian_3d(40), 1e-8), "lap3d_f32": (lambda: laplacian_3d(40).astype(np.float32), 3e-4)}


@pytest.mark.parametrize("case", list(GRIDS))
def test_default_equals_every_column_read(oracle, eng, monkeypatch, case):
	"""SLQ_OMEGA=1 (default) against SLQ_OMEGA=0 on wide and narrow panels (64, 32 and 16 lanes per row), fp64 and fp32, k = 24:
	the plans offer their full windows, skip columns, and hand out the same bits; the counters add up."""
	monkeypatch.setenv("SLQ_TILES", "2")
	make, rtol = GRIDS[case]
	A = make()
	n, deg = A.shape[0], 24
	op = eng.DeviceOperator(A)
	for P in (300, 100, 40) if A.dtype == np.float32 else (130, 64, 20):  # 64, 32 and 16 lanes per panel row
		X = oc.rademacher(n, P, 7 + P, A.dtype)
		off = oc.run(eng, monkeypatch, op, X, deg, 3, {"SLQ_OMEGA": 0})
		on = oc.run(eng, monkeypatch, op, X, deg, 3, {})
		assert on["info"]["sequence"] == "fused_gram" and on["info"]["omega"] == 1 and off["info"]["omega"] == 0, (on["info"], off["info"])
		c = on["cols"]
		print(f"OMEGA {case} P={P} panels={on['info']['panels']}: {c}")
		assert c["offered"] == (deg - 2) * on["info"]["panels"] and 0 <= c["read"] <= c["offered"] and c["violations"] == 0, c
		assert off["cols"]["offered"] == 0
		assert c["read"] < c["offered"], f"nothing was skipped: {c}"
		if c["rescues"] == 0:
			assert _same(on, off), f"{case} P={P}: default differs from SLQ_OMEGA=0 without a rescue"
		else:  # another kernel measured an entry in another summation order: the tridiagonal to 1e-10 (fp32: 3e-4) of the run that reads every column
			ab = _tridiag_dist(on, off)
			print(f"   {case} P={P}: {c['rescues']} rescue(s), tridiagonal {ab:.2e} from SLQ_OMEGA=0")
			assert ab <= (1e-10 if A.dtype == np.float64 else 3e-4), ab
		cols = [0, P // 2, P - 1]
		_oracle_bar(oracle, A, X, deg, 3, on, cols, rtol)
		## windows that are not offered: every other depth takes the sequence as it was
		for orth in (2, 6):
			o1 = oc.run(eng, monkeypatch, op, X, deg, orth, {})
			o0 = oc.run(eng, monkeypatch, op, X, deg, orth, {"SLQ_OMEGA": 0})
			assert o1["info"]["omega"] == 0 and o1["cols"]["offered"] == 0 and _same(o1, o0)
	op.close()


def _verify_zero(eng, monkeypatch, op, X, deg, tag, checked=False):
	v = oc.run(eng, monkeypatch, op, X, deg, 3, {"SLQ_OMEGA": 2})
	off = oc.run(eng, monkeypatch, op, X, deg, 3, {"SLQ_OMEGA": 0})
	c, w = v["cols"], v["verify"]
	print(f"OMEGA-VERIFY {tag}: omega {v['info']['omega']} sequence {v['info']['sequence']} {c} innovation {w['innovation']:.4f} eps|A| margin {w['margin']:.3f} c {w['c']} kappa {w['kappa']}")
	assert _same(v, off), f"{tag}: verify mode changed the results"
	assert c["violations"] == 0, f"{tag}: {c} {w}"
	if checked:  # the run compared at least one certificate with a measurement (an estimate was carried over a skipped step)
		assert v["info"]["omega"] == 2 and w["innovation"] > 0.0 and np.isfinite(w["margin"]), f"{tag}: nothing was checked: {c} {w}"
	return v


def test_verify_mode_reports_no_violation(golden, eng, monkeypatch):
	"""SLQ_OMEGA=2: the column is read, the measured decisions are applied (bitwise SLQ_OMEGA=0), and beside them the estimate and
	its radius run as the default would run them. A violation is a certificate that would have said "zero" where the measured
	|q_t . w| exceeds the threshold, or an estimate further from the measurement than its radius. Golden Laplacian, the k = 100 /
	300 plans that lose orthogonality, the ill-conditioned D L D, a ragged random band on tiles, fp32, the seed-79 graph.

	What the committed constants (c = 3.5, kappa = 4) let each case check: a certificate can hold over a skipped step only where
	tol / kappa = eps sqrt(n) / 2 exceeds about three theta = 10.5 eps ||A||_inf, i.e. from about 28,000 rows on the 5-point grid
	(63,500 on the 7-point one). The cases the issue names with ~10,000 rows (lap2d_100, lap3d_22) therefore read every column
	and the verify mode has nothing to compare on them (zero violations holds trivially: not covered); the same plans are run
	here on the 200^2 and 40^3 grids, where the device skips, and THOSE must have checked an estimate (`checked`). D L D with D
	over four decades has ||A||_inf ~ 1e5: theta is above tol for any n that fits a GPU, it always reads (not covered); a D L D
	over 0.4 decades on a 500^2 grid stands in. The golden Laplacian (576 rows) and the seed-79 graph (~1,500 rows, random) are
	not served by ring-fed tiles and are not offered (omega 0: not covered). A random SPD graph on tiles: scripts/fuzz_parity.py."""
	monkeypatch.setenv("SLQ_TILES", "2")
	L = laplacian_2d(int(golden["lap_m"]))
	op = eng.DeviceOperator(L)
	Xg = np.asfortranarray(golden["lap_probes"])
	v = _verify_zero(eng, monkeypatch, op, Xg, min(20, L.shape[0]), "golden laplacian")
	op.close()
	for name, A in (("lap2d_100", laplacian_2d(100)), ("lap3d_22", laplacian_3d(22))):
		op = eng.DeviceOperator(A)
		for deg in (100, 300):
			for P in (20, 64, 130):
				v = _verify_zero(eng, monkeypatch, op, oc.rademacher(A.shape[0], P, deg + P), deg, f"{name} k={deg} P={P}")
				assert v["info"]["omega"] == 2 and v["cols"]["offered"] > 0
		op.close()
	for name, A in (("lap2d_200", laplacian_2d(200)), ("lap3d_40", laplacian_3d(40))):
		op = eng.DeviceOperator(A)
		for deg in (100, 300):
			for P in (20, 64, 130):
				_verify_zero(eng, monkeypatch, op, oc.rademacher(A.shape[0], P, deg + P), deg, f"{name} k={deg} P={P}", checked=True)
		op.close()
	for dt in (np.float64, np.float32):
		A = oc.ill_conditioned(dt, m=500, decades=0.2)
		op = eng.DeviceOperator(A)
		_verify_zero(eng, monkeypatch, op, oc.rademacher(A.shape[0], 64, 98, dt), 60, f"D L D over 0.4 decades on 500^2 {np.dtype(dt).name}", checked=True)
		op.close()
		A = oc.ragged_band(dtype=dt, n=160011)
		op = eng.DeviceOperator(A)
		for P in (40, 64, 130):
			_verify_zero(eng, monkeypatch, op, oc.rademacher(A.shape[0], P, P, dt), 40, f"ragged band of 160,011 rows {np.dtype(dt).name} P={P}", checked=True)
		op.close()
		A = oc.ill_conditioned(dt)
		op = eng.DeviceOperator(A)
		_verify_zero(eng, monkeypatch, op, oc.rademacher(A.shape[0], 64, 99, dt), 60, f"D L D {np.dtype(dt).name}")
		op.close()
		A = oc.ragged_band(dtype=dt)
		op = eng.DeviceOperator(A)
		for P in (20, 64, 130):
			_verify_zero(eng, monkeypatch, op, oc.rademacher(A.shape[0], P, P, dt), 40, f"ragged band {np.dtype(dt).name} P={P}")
		op.close()
		A = laplacian_3d(40).astype(dt)
		op = eng.DeviceOperator(A)
		_verify_zero(eng, monkeypatch, op, oc.rademacher(A.shape[0], 200, 5, dt), 30, f"lap3d_40 {np.dtype(dt).name}", checked=True)
		op.close()
	A, X = oc.seed79()
	op = eng.DeviceOperator(A)
	_verify_zero(eng, monkeypatch, op, X, 37, "seed 79 (offered only if the tiles serve it)")
	op.close()


@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-8), (np.float32, 3e-4)])
def test_forced_trip_and_rescue(oracle, eng, monkeypatch, dtype, rtol):
	"""SLQ_OMEGA_TRIP=j makes every panel read at step j; SLQ_OMEGA_RESCUE=j makes every panel measure the missing entry by the
	rescue kernels at step j. Early, middle and last step, wide and narrow panels: the counters show it, a trip is followed by
	skipping again (a read -> skip transition), and the results stay what SLQ_OMEGA=0 gives (bitwise without a rescue; within
	the oracle bar with one)."""
	monkeypatch.setenv("SLQ_TILES", "2")
	A = laplacian_2d(200).astype(dtype)
	n, deg = A.shape[0], 24
	op = eng.DeviceOperator(A)
	for P in (260, 40) if dtype == np.float32 else (130, 20):  # 64 and 16 lanes per panel row
		X = oc.rademacher(n, P, 11 + P, dtype)
		cols = [0, P // 2, P - 1]
		off = oc.run(eng, monkeypatch, op, X, deg, 3, {"SLQ_OMEGA": 0})
		base = oc.run(eng, monkeypatch, op, X, deg, 3, {})
		NP = base["info"]["panels"]
		## steps at which NO panel of the untripped run reads: an early one, one in the middle, the last one (a trip there is the trip's doing)
		rd_b = base["flags"][0]
		quiet = [j for j in range(3, deg) if not rd_b[j].any()]
		assert len(quiet) >= 3, rd_b.T
		trips = sorted({quiet[0], min(quiet, key=lambda j: abs(j - deg // 2)), quiet[-1]})
		for j in trips:
			t = oc.run(eng, monkeypatch, op, X, deg, 3, {"SLQ_OMEGA_TRIP": j})
			rd_t = t["flags"][0]
			print(f"OMEGA-TRIP {np.dtype(dtype).name} P={P} j={j}: {t['cols']} (untripped {base['cols']}); steps read, panel 0: tripped {np.flatnonzero(rd_t[:, 0]).tolist()} untripped {np.flatnonzero(rd_b[:, 0]).tolist()}")
			assert np.all(rd_t[j] == 1) and np.all(rd_b[j] == 0), (j, rd_t.T, rd_b.T)  # the counters show the read: every panel, at the tripped step
			assert np.array_equal(rd_t[:j], rd_b[:j])  # (nothing before it moved)
			assert t["cols"]["read"] == int(rd_t.sum()) and t["cols"]["offered"] == (deg - 2) * NP
			if j < deg - 1:  # ... and the panels go back to skipping at once: the measured entry reset the radius
				assert np.all(rd_t[j + 1] == 0), (j, rd_t.T)
				assert t["cols"]["transitions"] == int(np.sum((rd_t[2:-2] == 1) & (rd_t[3:-1] == 0))), (t["cols"], rd_t.T)
			if t["cols"]["rescues"] == 0:
				assert _same(t, off)
			else:
				assert _tridiag_dist(t, off) <= (1e-10 if dtype == np.float64 else 3e-4)
			_oracle_bar(oracle, A, X, deg, 3, t, cols, rtol)
		for j in (3, deg // 2, deg - 1):
			r = oc.run(eng, monkeypatch, op, X, deg, 3, {"SLQ_OMEGA_RESCUE": j})
			print(f"OMEGA-RESCUE {np.dtype(dtype).name} P={P} j={j}: {r['cols']}")
			assert r["cols"]["rescues"] >= NP and np.all(r["flags"][1][j] == 1), (r["cols"], r["flags"][1].T)  # every panel, at the forced step
			err = _oracle_bar(oracle, A, X, deg, 3, r, cols, rtol)
			ab = _tridiag_dist(r, off)
			print(f"   rescue at j={j}: quadrature {err:.2e} from the oracle, tridiagonal {ab:.2e} from SLQ_OMEGA=0")
			assert ab <= (1e-10 if dtype == np.float64 else 3e-4)
		## a trip and a rescue in one run, the rescue right behind the trip
		both = oc.run(eng, monkeypatch, op, X, deg, 3, {"SLQ_OMEGA_TRIP": 6, "SLQ_OMEGA_RESCUE": 9})
		assert np.all(both["flags"][0][6] == 1) and np.all(both["flags"][1][9] == 1)
		_oracle_bar(oracle, A, X, deg, 3, both, cols, rtol)
	op.close()


def test_the_device_reads_the_column_by_itself(oracle, eng, monkeypatch):
	"""A natural trip: on the ill-conditioned D L D (and on k = 300, where orthogonality is lost) the device itself reads the
	column at some steps - 0 < read <= offered - and parity holds by the oracle-only bars of the existing tests (fp64: max(1e-6,
	10x oracle_spread) on the ill-conditioned operator, 1e-8 for smooth functions on the grid)."""
	from test_gpu_parity import oracle_spread

	monkeypatch.setenv("SLQ_TILES", "2")
	A = oc.ill_conditioned()
	P, deg = 64, 60
	X = oc.rademacher(A.shape[0], P, 99)
	cols = [0, 1, P // 2, P - 1]
	Xc = np.asfortranarray(X[:, cols])
	op = eng.DeviceOperator(A)
	on = oc.run(eng, monkeypatch, op, X, deg, 3, {})
	op.close()
	c = on["cols"]
	print(f"OMEGA-NATURAL D L D: {c}")
	assert on["info"]["omega"] == 1 and 0 < c["read"] <= c["offered"], c
	ref = oracle.quad_batch(A, Xc, deg, 3, fun="log", fresh_q=True, prefer="csr")
	spread = oracle_spread(oracle, A, Xc, deg, 3, funs=[("log", {})], seed=3)[1]["log"].max()
	err = np.max(np.abs(on["log"][cols] - ref) / np.abs(ref))
	print(f"   D L D orth 3: {err:.2e} from the oracle, oracle spread {spread:.2e}")
	assert err <= max(1e-6, 10.0 * spread)
	A = laplacian_3d(22)
	X = oc.rademacher(A.shape[0], 64, 300)
	op = eng.DeviceOperator(A)
	on = oc.run(eng, monkeypatch, op, X, 300, 3, {})
	op.close()
	c = on["cols"]
	print(f"OMEGA-NATURAL lap3d_22 k=300: {c}")
	assert 0 < c["read"] <= c["offered"], c
	cols = [0, 1, 32, 63]
	ref = oracle.quad_batch(A, np.asfortranarray(X[:, cols]), 300, 3, fun="log", fresh_q=True)
	assert np.max(np.abs(on["log"][cols] / ref - 1.0)) <= 1e-8
	## ... and where the device both skips and reads of its own accord: k = 300 on the 200^2 grid (tol / kappa is about seven theta:
	## the radius reaches the bar every few steps, the panel reads, the measured entry resets it)
	A = laplacian_2d(200)
	X = oc.rademacher(A.shape[0], 130, 301)
	op = eng.DeviceOperator(A)
	on = oc.run(eng, monkeypatch, op, X, 300, 3, {})
	off = oc.run(eng, monkeypatch, op, X, 300, 3, {"SLQ_OMEGA": 0})
	op.close()
	c, rd = on["cols"], on["flags"][0]
	print(f"OMEGA-NATURAL lap2d_200 k=300: {c}; steps read, panel 0: {np.flatnonzero(rd[:, 0]).tolist()}")
	assert 0 < c["read"] < c["offered"] and c["transitions"] > 0, c
	assert _same(on, off) if c["rescues"] == 0 else _tridiag_dist(on, off) <= 1e-10
	cols = [0, 1, 65, 129]
	ref = oracle.quad_batch(A, np.asfortranarray(X[:, cols]), 300, 3, fun="log", fresh_q=True)
	assert np.max(np.abs(on["log"][cols] / ref - 1.0)) <= 1e-8


def test_staged_runs_and_replays_keep_the_flags(eng, monkeypatch):
	"""The recurrence's state lives in the plan: a run in stages equals the one-shot run bit for bit with the default on, and
	so do two runs of the same plan (the state is cleared with the Gram rows)."""
	monkeypatch.setenv("SLQ_TILES", "2")
	A = laplacian_2d(200)
	n, P, deg = A.shape[0], 130, 24
	X = oc.rademacher(n, P, 3)
	op = eng.DeviceOperator(A)
	plan = eng.LanczosPlan(op, P, deg, 3)
	assert plan.describe()["omega"] == 1
	plan.set_probes(X)
	plan.run()
	one = plan.tridiag()
	c1 = plan.window_columns(reset=True)
	plan.set_probes(X)
	plan.run()
	two = plan.tridiag()
	c2 = plan.window_columns(reset=True)
	assert all(np.array_equal(a, b) for a, b in zip(one, two)) and c1 == c2
	plan.set_probes(X)
	for stop in (5, 6, 17, deg):
		plan.run(upto=stop)
	st = plan.tridiag()
	c3 = plan.window_columns(reset=True)
	assert all(np.array_equal(a, b) for a, b in zip(one, st)) and c3 == c1, (c1, c3)
	plan.close()
	op.close()
