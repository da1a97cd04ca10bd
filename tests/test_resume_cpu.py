"""Resumable runs / Gauss-Radau / adaptive degree: what needs no GPU. Argument checks made before any device work, the
refusal of the sharded entries, the C-ABI declarations, and the premises the GPU tests rest on, checked on the CPU oracle:
a prefix of a run is the run of that degree, the NumPy Radau construction agrees with 50 digits, and the bracket holds."""

import re
from pathlib import Path

import numpy as np
import pytest

from _radau_check import expected_stop, gauss_np, jacobi, radau_mp, radau_np, rule_distance
from conftest import laplacian_2d

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_plan_run_steps", "slq_plan_steps_done", "slq_plan_quadrature_at", "slq_quadrature_radau_batch")


def _no_library(monkeypatch):
	from primate_amd import _capi

	def touched(*a, **k):
		raise AssertionError("libslq was touched before the arguments were checked")

	monkeypatch.setattr(_capi, "lib", touched)


@pytest.mark.parametrize(
	"kw",
	[dict(deg_rtol=0.0), dict(deg_rtol=-1e-3), dict(deg_rtol=None), dict(deg_rtol=float("nan")), dict(stages=[5, 5, 10]), dict(stages=[10, 5]),
	 dict(stages=[0, 5]), dict(stages=[5, 31]), dict(stages=[]), dict(stages=[2.5, 5]), dict(stages=7), dict(deg_max=0), dict(deg_max=2.5),
	 dict(endpoint=float("inf")), dict(deg_step=0), dict(stages=[5, 10], deg_step=5), dict(fun=np.log), dict(X=("cauchy", 0, 0)), dict(X=("rademacher", 0, 0))],
)  # fmt: skip
def test_bad_adaptive_arguments_raise_before_the_library_is_touched(monkeypatch, kw):
	from primate_amd import engine

	_no_library(monkeypatch)
	args = dict(X=np.ones((8, 2)), deg_max=30, orth=3, fun="log", stages=None, deg_rtol=1e-3)
	args.update(kw)
	X = args.pop("X")
	with pytest.raises(ValueError):
		engine.quad_adaptive(object(), X, **args)


def test_default_stages():
	from primate_amd import engine

	assert engine._adaptive_args(30, None, 1e-3)[1] == [5, 10, 15, 20, 25, 30]
	assert engine._adaptive_args(32, None, 1e-3)[1] == [5, 10, 15, 20, 25, 30, 32]  # deg_max appended
	assert engine._adaptive_args(32, None, 1e-3, deg_step=10, first=20)[1] == [20, 30, 32]
	assert engine._adaptive_args(60, (5, 10, 60), 1e-3)[1] == [5, 10, 60]
	assert engine._adaptive_args(3, None, 1e-3, first=3)[1] == [3]


def test_rule_arguments_raise_before_the_library_is_touched(monkeypatch):
	from primate_amd import engine, integrate

	_no_library(monkeypatch)
	plan = object.__new__(engine.LanczosPlan)
	plan._h = None
	with pytest.raises(ValueError, match="endpoint"):
		plan.quadrature_at(3, "log", rule="radau")
	with pytest.raises(ValueError):
		plan.quadrature_at(3, "log", rule="radau", endpoint=float("nan"))
	with pytest.raises(ValueError, match="lobatto"):
		plan.quadrature_at(3, "log", rule="lobatto", endpoint=0.0)
	with pytest.raises(ValueError):
		plan.quadrature_at(3, np.log, return_stage=True)
	d, e = np.array([2.0, 2.0]), np.array([0.0, -1.0])
	for kw in (dict(), dict(endpoint=0.1), dict(residual=1.0), dict(endpoint=float("inf"), residual=1.0)):
		with pytest.raises(ValueError):
			integrate.quadrature(d, e, quad="radau", **kw)
	with pytest.raises(ValueError):
		integrate.quadrature(d, e, endpoint=0.1)  # belongs to quad="radau"
	with pytest.raises(ValueError):
		engine.quadrature_radau_batch(d[None], e[None], None, 0.1)


def test_matrix_function_checks_its_adaptive_arguments_first(monkeypatch):
	from primate_amd.operators import MatrixFunction

	_no_library(monkeypatch)
	A = np.eye(8)
	for kw in (dict(deg_max=30), dict(deg_max=30, deg_rtol=0.0), dict(deg_max=4, deg_rtol=1e-3, deg=5), dict(deg_max=30, deg_rtol=1e-3, deg_step=0),
			   dict(deg_rtol=1e-3), dict(endpoint=0.1), dict(deg_step=5), dict(deg_max=30, deg_rtol=1e-3, stale_ring=True),
			   dict(deg_max=30, deg_rtol=1e-3, endpoint=float("nan"))):  # fmt: skip
		with pytest.raises(ValueError):
			MatrixFunction(A, "log", **kw)
	with pytest.raises(ValueError):
		MatrixFunction(A, np.log, deg_max=30, deg_rtol=1e-3)  # a callable: the stage statistics are reduced on the device


def test_sharded_entries_refuse_an_adaptive_matrix_function(monkeypatch):
	from primate_amd import distributed
	from primate_amd.operators import MatrixFunction

	_no_library(monkeypatch)
	M = object.__new__(MatrixFunction)
	M._adaptive = dict(deg_max=30, stages=[5, 10, 30], deg_rtol=1e-3, endpoint=None)
	M.shape, M.dtype = (8, 8), np.dtype(np.float64)
	for call in (
		lambda: distributed.sharded_xtrace(M, 16),
		lambda: distributed.sharded_xtrace(M, 16, sketches="rows"),
		lambda: distributed.sharded_spectral_density(M),
		lambda: distributed.sharded_spectral_density(np.eye(8), deg_max=30, deg_rtol=1e-3),
		lambda: distributed.sharded_hutch(M.quad_generated),
		lambda: distributed.sharded_hutch(M.quad),
		lambda: distributed.sharded_hutch_device(M, 16),
		lambda: distributed.sharded_diag_device(M, 16, 20),
	):
		with pytest.raises(ValueError, match="adaptive"):
			call()


def test_new_entries_are_declared_and_bound():
	from primate_amd import _capi

	hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "slq.h").read_text(), flags=re.S)
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint\s+{s}\s*\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
	assert "SLQ_VERSION 100" in hdr
	L = _capi.lib()  # (loading needs no device)
	assert all(hasattr(L, s) for s in NEW_SYMBOLS)
	## NULL handles are arguments errors, not crashes
	assert L.slq_plan_run_steps(None, 1e-8, 5) == _capi.SLQ_EINVAL
	assert L.slq_plan_steps_done(None, None) == _capi.SLQ_EINVAL
	assert L.slq_plan_quadrature_at(None, 1, 0, 0.0, 0, None, None, None, None, None) == _capi.SLQ_EINVAL
	assert L.slq_quadrature_radau_batch(None, 1, 1, None, None, None, 0.0, 0, None, None, None, None) == _capi.SLQ_EINVAL


## ---- the premises of tests/test_gpu_resume.py, on the CPU oracle ------------------------------------------------------
def _rademacher(n, p, seed):
	rng = np.random.default_rng(seed)
	return np.asfortranarray(np.floor(rng.random((n, p)) * 2) * 2 - 1)


def _oracle_run(O, A, v, m, orth):
	o = min(orth, m)
	al, be = np.zeros(m + 1), np.zeros(m + 1)
	Q = np.zeros((A.shape[0], max(2, o)), order="F")
	O.lanczos(A, v, m, 1e-8, o, al, be, Q)
	return al, be


@pytest.mark.parametrize("orth", [0, 3, 10, 12])
def test_a_prefix_of_a_run_is_the_run_of_that_degree_bit_for_bit(oracle, orth):
	"""With a clean ring, steps j < orth project on all earlier vectors and later windows coincide: the first m steps of a
	(deg, orth) run are the (m, min(orth, m)) run. The oracle keeps a ring of max(orth, 2) columns either way."""
	A = laplacian_2d(24)
	V = _rademacher(A.shape[0], 3, 5)
	for deg in (20, 60):
		for i in range(V.shape[1]):
			al, be = np.zeros(deg + 1), np.zeros(deg + 1)
			Q = np.zeros((A.shape[0], max(2, orth)), order="F")
			oracle.lanczos(A, V[:, i], deg, 1e-8, orth, al, be, Q)
			for m in (3, 5, 11, 13, 20, 40):
				if m > deg:
					continue
				pa, pb = _oracle_run(oracle, A, V[:, i], m, orth)
				assert np.array_equal(pa[:m], al[:m]) and np.array_equal(pb[: m + 1], be[: m + 1]), (deg, orth, m)


def test_numpy_radau_rule_against_50_digits_and_its_defining_properties(oracle):
	A = laplacian_2d(24)
	lam = np.linalg.eigvalsh(A.toarray())
	a = lam[0] / 2
	v = _rademacher(A.shape[0], 1, 3)[:, 0]
	for m in (1, 2, 7, 20):
		al, be = _oracle_run(oracle, A, v, m, 3)
		r64, r50 = radau_np(al, be, m, a), radau_mp(al, be, m, a)
		assert rule_distance(r64, r50) < 1e-13
		assert abs(r64[0][0] - a) < 1e-13 and abs(r64[1].sum() - 1.0) < 1e-13 and np.all(r64[1] >= 0)
		## exact for polynomials up to degree 2m: the moments e1^T A^k e1 of the (normalised) probe
		u = v / np.linalg.norm(v)
		w = u.copy()
		for k in range(0, 2 * m + 1):
			mom = float(u @ w)
			assert abs(np.sum(r64[0] ** k * r64[1]) - mom) <= 1e-10 * mom, (m, k)  # (A is positive definite: mom > 0)
			w = A @ w
		## the forward recurrence the device runs gives the same border entry as the linear solve
		delta = al[0] - a
		for j in range(1, m):
			delta = al[j] - a - be[j] ** 2 / delta
		T = jacobi(al, be, m)
		rhs = np.zeros(m)
		rhs[-1] = be[m] ** 2
		assert abs(be[m] ** 2 / delta - np.linalg.solve(T - a * np.eye(m), rhs)[-1]) <= 1e-12 * abs(be[m] ** 2 / delta)


def test_the_bracket_holds_on_the_oracle():
	"""The 384 cases of test_gauss_and_radau_values_bracket_the_truth with the oracle's Lanczos and NumPy rules: no miss
	with a slack of 1e-12 |truth| (the device gets that plus its parity bar)."""
	from oracle import oracle as O

	O.build()
	A = laplacian_2d(24)
	n = A.shape[0]
	lam, U = np.linalg.eigh(A.toarray())
	a = lam[0] / 2
	funs = {"log": np.log, "inv": lambda x: 1.0 / x, "exp": lambda x: np.exp(-x)}
	ncase = 0
	for orth in (0, 3, 10, 60):
		V = _rademacher(n, 8, 100 + orth)
		C2 = (U.T @ V) ** 2
		for m in (5, 10, 20, 40):
			for i in range(8):
				al, be = _oracle_run(O, A, V[:, i], m, orth)
				g, r = gauss_np(al, be, m), radau_np(al, be, m, a)
				for name, f in funs.items():
					truth = float(f(lam) @ C2[:, i])
					gv, rv = float(np.sum(f(g[0]) * g[1]) * n), float(np.sum(f(r[0]) * r[1]) * n)
					slack = 1e-12 * abs(truth)
					assert min(gv, rv) - slack <= truth <= max(gv, rv) + slack, (orth, m, i, name)
					ncase += 1
	assert ncase == 384


def test_expected_stop_follows_the_documented_rule():
	stages = [5, 10, 20, 40]
	S = np.array([100.0, 101.0, 101.01, 101.0101])
	W = np.array([3.0, 0.5, 0.02, 1e-4])
	assert expected_stop(stages, S, W, 1e-3, False) == 20  # |101.01 - 101| / 101.01 = 9.9e-5
	assert expected_stop(stages, S, W, 1e-2, False) == 10  # never at the first stage: there is no earlier sum
	assert expected_stop(stages, S, W, 1.0, False) == 10
	assert expected_stop(stages, S, W, 1e-9, False) == 40
	assert expected_stop(stages, S, W, 1e-3, True) == 20
	assert expected_stop(stages, S, W, 1.0, True) == 5  # the bracket needs no earlier stage
	assert expected_stop(stages, S, W, 1e-9, True) == 40
