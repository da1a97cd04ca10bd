"""The Chebyshev action f(A) X = sum_k c_k T_k(A~) X, what needs no GPU: the C-ABI symbols, the schedule of
the accumulation launches and the ring it needs (slq_debug_cheb_action_schedule: pure host logic), the NumPy yardstick of the
GPU tests against the exact sine-basis formula, and the argument errors of the Python layer."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from _cheb_action_ref import action_bar, action_eig, action_recurrence, action_recurrence_ld, coefficient_weight, col_norms, jackson_step_coefficients
from _cheb_ref import center_halfwidth, grid_laplacian
from primate_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_plan_create_chebyshev_action", "slq_plan_chebyshev_action", "slq_plan_chebyshev_action_dmat", "slq_debug_cheb_action_schedule")


def test_symbols_are_declared_exported_and_bound():
	hdr = (ROOT / "include" / "slq.h").read_text()
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint {s}\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"
	m = re.search(r"#define SLQ_CHEB_ACC_COLS (\d+)", (ROOT / "primate_amd" / "csrc" / "slq_format.hpp").read_text())
	assert m and 8 <= int(m.group(1)) <= 16
	from primate_amd import chebyshev, engine

	for name in ("action", "action_into", "describe"):
		assert callable(getattr(engine.ChebyshevPlan, name)), name
	assert chebyshev.ChebyshevFunction._matmat is not None and chebyshev.ChebyshevFunction._matvec is not None


## ---- the schedule --------------------------------------------------------------------------------------------------
def schedule(nsteps):
	"""(pieces [(t0, nc)], ring_slots, acc_cols) as the library decides them."""
	L = _capi.lib()
	npieces, S, K = C.c_int(), C.c_int(), C.c_int()
	assert L.slq_debug_cheb_action_schedule(nsteps, None, None, 0, C.byref(npieces), C.byref(S), C.byref(K)) == _capi.SLQ_OK
	cap = npieces.value
	t0, nc = (C.c_int * cap)(), (C.c_int * cap)()
	assert L.slq_debug_cheb_action_schedule(nsteps, t0, nc, cap, C.byref(npieces), None, None) == _capi.SLQ_OK
	assert npieces.value == cap
	return list(zip(t0[:], nc[:])), S.value, K.value


def simulate(nsteps, pieces, S, K):
	"""Run the ring: w_t lives in slot t % S; step j reads w_j and w_{j-1} and writes w_{j+1}; a piece is launched as soon as its
	last column exists. Returns None, or what went wrong."""
	slot = {0: 0}  # slot -> the column it holds
	consumed, queue = set(), list(pieces)
	for j in range(nsteps):
		dst = (j + 1) % S
		held = slot.get(dst)
		if held is not None:
			if held in (j, j - 1):
				return f"step {j} overwrites w_{held}, which it reads"
			if held not in consumed:
				return f"step {j} overwrites the unconsumed column {held}"
		slot[dst] = j + 1
		while queue and queue[0][0] + queue[0][1] - 1 <= j + 1:
			t0, nc = queue.pop(0)
			# issued when K columns are unconsumed, or after the last step - not earlier
			if not (nc == K or j == nsteps - 1):
				return f"piece ({t0}, {nc}) after step {j} is neither full nor the last"
			for t in range(t0, t0 + nc):
				if slot.get(t % S) != t:
					return f"piece ({t0}, {nc}) reads column {t}, which is not in the ring"
				consumed.add(t)
	return None if not queue else "pieces left over"


@pytest.mark.parametrize("nsteps", list(range(1, 41)) + [16384])
def test_schedule_consumes_every_column_once_on_the_smallest_ring(nsteps):
	pieces, S, K = schedule(nsteps)
	assert 8 <= K <= 16
	# every column 0 .. nsteps exactly once, ascending; no piece above K
	cols = [t for t0, nc in pieces for t in range(t0, t0 + nc)]
	assert cols == list(range(nsteps + 1))
	assert all(1 <= nc <= K for _, nc in pieces)
	assert len(pieces) == -(-(nsteps + 1) // K)
	assert simulate(nsteps, pieces, S, K) is None
	# minimality: one slot less and some step overwrites what is still needed
	assert S >= 2 and simulate(nsteps, pieces, S - 1, K) is not None


def test_schedule_rejects_bad_arguments():
	L = _capi.lib()
	n = C.c_int()
	for bad in (0, -3, 16385):
		assert L.slq_debug_cheb_action_schedule(bad, None, None, 0, C.byref(n), None, None) == _capi.SLQ_EINVAL
	assert L.slq_debug_cheb_action_schedule(5, None, None, 0, None, None, None) == _capi.SLQ_EINVAL
	# a short capacity writes what fits and still reports the count
	t0, nc = (C.c_int * 1)(), (C.c_int * 1)()
	assert L.slq_debug_cheb_action_schedule(100, t0, nc, 1, C.byref(n), None, None) == _capi.SLQ_OK
	assert n.value > 1 and t0[0] == 0 and nc[0] >= 8


## ---- the yardstick --------------------------------------------------------------------------------------------------
def test_restatement_matches_the_sine_basis_formula():
	"""The long-double restatement against U p(L) U^T Z on the 40 x 37 grid, p the same polynomial evaluated at the exact
	eigenvalues in long double: within B = eps_64 sum_k (k + 1) |c_k| ||z|| (measured: <= 0.21 B), for exp(-x) at degrees 9 and 18
	and a Jackson-damped step at degree 200; and the fp64 / fp32 restatements deviate from it at their own scale - the bar of the
	GPU tests is B wherever 8 D <= B."""
	from numpy.polynomial import chebyshev as npc

	from primate_amd.chebyshev import chebyshev_coefficients, spectral_bounds

	m1, m2, P = 40, 37, 6
	A = grid_laplacian(m1, m2)
	b = spectral_bounds(A, "gershgorin")
	c, h = center_halfwidth(b)
	Z = np.random.default_rng(21).standard_normal((m1 * m2, P))
	cases = [("exp9", chebyshev_coefficients("exp", 10, b, t=-1.0)), ("exp18", chebyshev_coefficients("exp", 19, b, t=-1.0)),
	         ("step200", jackson_step_coefficients(200, b, c))]  # fmt: skip
	eps = float(np.finfo(np.float64).eps)
	for name, coef in cases:
		Yld = action_recurrence(A, Z, coef, b, np.longdouble)
		assert Yld.dtype == np.longdouble
		assert np.array_equal(action_recurrence_ld(A, Z, coef, b, chunk=4), Yld)  # (chunks of columns in threads: the same bits)
		exact = action_eig(m1, m2, Z, lambda lam: npc.chebval(((lam.astype(np.longdouble) - c) / h), coef.astype(np.longdouble)).astype(np.float64))
		B = eps * coefficient_weight(coef) * col_norms(Z)
		# (the formula itself is an fp64 transform: its own error, a few eps ||p(A) z||, is inside B as well)
		err = col_norms(Yld - exact)
		print(f"{name}: long-double restatement against the formula, max err / B = {float(np.max(err / B)):.3f}")
		assert np.all(err <= B), (name, float(np.max(err / B)))
		for dt in (np.float64, np.float32):
			bar, D, Bf = action_bar(Yld, action_recurrence(A, Z, coef, b, dt), Z, coef, float(np.finfo(dt).eps))
			print(f"{name} {np.dtype(dt).name}: D / B = {float(np.min(D / Bf)):.3f} .. {float(np.max(D / Bf)):.3f}")
			assert np.all(D > 0) and np.all(D <= Bf), (name, dt)
			assert np.array_equal(bar, np.maximum(8.0 * D, Bf))


## ---- argument errors of the Python layer, raised before any device work -------------------------------------------------
def test_argument_errors_before_any_device_work(monkeypatch):
	from primate_amd import chebyshev, engine

	def no_device(*a, **k):
		raise AssertionError("device work before the arguments were checked")

	monkeypatch.setattr(engine, "DeviceOperator", no_device)
	monkeypatch.setattr(engine, "default_context", no_device)
	monkeypatch.setattr(chebyshev, "_as_device_operator", no_device)
	monkeypatch.setattr(_capi, "lib", no_device)
	A = grid_laplacian(6, 5)

	def plan(action=True, nsteps=4):
		p = engine.ChebyshevPlan.__new__(engine.ChebyshevPlan)  # (the argument checks read these fields and nothing else)
		p.nsteps, p.nprobes, p.is_action, p._h = nsteps, 2, action, None
		return p

	good = np.ones(5)
	bad = [
		lambda: chebyshev.ChebyshevFunction(A, "exp", deg=8, batch=0),
		lambda: chebyshev.ChebyshevFunction(A, "exp", deg=8, batch=-4),
		lambda: chebyshev.ChebyshevFunction(A, "exp", deg=8, batch=2.5),
		lambda: chebyshev.ChebyshevFunction(A, "exp", deg=8, batch=True),
		lambda: plan(action=False).action((0.0, 8.0), good),
		lambda: plan().action((0.0, 8.0), np.ones(4)),
		lambda: plan().action((0.0, 8.0), np.ones(6)),
		lambda: plan().action((0.0, 8.0), np.array([1.0, np.nan, 0.0, 0.0, 0.0])),
		lambda: plan().action((0.0, 8.0), np.array([1.0, np.inf, 0.0, 0.0, 0.0])),
		lambda: plan().action((8.0, 0.0), good),
		lambda: plan().action((0.0, np.inf), good),
		lambda: plan().action(3.0, good),
		lambda: plan().action_into((0.0, 8.0), np.ones(3), None, 0),
		lambda: plan(action=False).action_into((0.0, 8.0), good, None, 0),
	]
	for i, call in enumerate(bad):
		with pytest.raises(ValueError) as ei:
			call()
		assert "device work" not in str(ei.value), i
