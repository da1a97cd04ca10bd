"""Two-pass f(A)v (recompute plans): what needs no GPU. The C-ABI declarations, the footprint arithmetic, the argument checks
made before any device work, and the premise of the GPU test against the kept basis - the bound between the two summation
orders of sum_t g_t W_t - checked on the CPU oracle's bases."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from _action_check import action_coeffs, order_bound, ordered_sum, random_spd_graph
from conftest import laplacian_2d

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_plan_create_recompute", "slq_plan_query_bytes_recompute", "slq_plan_basis_mode", "slq_fAv_batch_mode", "slq_plan_action_columns")
GB = 1e9


def _no_library(monkeypatch):
	from primate_amd import _capi

	def touched(*a, **k):
		raise AssertionError("libslq was touched before the arguments were checked")

	monkeypatch.setattr(_capi, "lib", touched)


def test_new_entries_are_declared_bound_and_exported():
	from primate_amd import _capi

	hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "slq.h").read_text(), flags=re.S)
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint\s+{s}\s*\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"


def test_recompute_footprint_is_independent_of_the_degree():
	"""slq_plan_query_bytes_recompute is host arithmetic: equal for deg = 30, 120, 1000; at most ring_slots + 10 panels; and the
	table of the 126^3 operator - a kept basis at deg = 120 does not exist on a 288 GB device, the recompute plan needs <= 58 GB."""
	from primate_amd import _capi

	L = _capi.lib()

	def rec(dtype, n, P, deg, orth):
		b = C.c_size_t()
		_capi.check(L.slq_plan_query_bytes_recompute(dtype, n, P, deg, orth, C.byref(b)))
		return b.value

	def ring(dtype, n, P, deg, orth, keep):
		b = C.c_size_t()
		_capi.check(L.slq_plan_query_bytes(dtype, n, P, deg, orth, keep, C.byref(b)))
		return b.value

	for dtype in (_capi.SLQ_F64, _capi.SLQ_F32):
		for n, P, orth in ((10**6, 256, 3), (10**6, 32, 0), (5000, 5, 10), (10**6, 130, 30)):
			sizes = {deg: rec(dtype, n, P, deg, orth) for deg in (30, 120, 1000)}
			assert len(set(sizes.values())) == 1, sizes
			slots = 2 if orth == 0 else max(orth + 1, 3)  # ring_slots(deg, orth, 0)
			ring0 = ring(dtype, n, P, 30, orth, 0)
			slot = ring0 // slots
			assert slot * slots == ring0
			assert ring0 + 2 * slot <= sizes[30] <= (slots + 10) * slot  # (the stash and the output at least)
	## small degrees: fewer extra slots
	assert rec(_capi.SLQ_F64, 1000, 8, 2, 0) < rec(_capi.SLQ_F64, 1000, 8, 30, 0)
	n = 126**3
	assert rec(_capi.SLQ_F64, n, 256, 50, 3) <= 58 * GB
	assert rec(_capi.SLQ_F64, n, 256, 120, 3) == rec(_capi.SLQ_F64, n, 256, 50, 3)
	assert ring(_capi.SLQ_F64, n, 256, 120, 3, 1) > 288 * GB
	assert 200 * GB < ring(_capi.SLQ_F64, n, 256, 50, 3, 1) < 215 * GB
	with pytest.raises(ValueError):
		rec(_capi.SLQ_F64, n, 256, 0, 3)
	with pytest.raises(ValueError):
		rec(_capi.SLQ_F64, 0, 256, 10, 3)


def test_basis_arguments_raise_before_the_library_is_touched(monkeypatch):
	from primate_amd import distributed, engine
	from primate_amd.operators import MatrixFunction

	_no_library(monkeypatch)
	for kw in (dict(basis="nope"), dict(basis="auto"), dict(basis=1), dict(keep_basis=True, basis="recompute"), dict(basis="")):
		with pytest.raises(ValueError):
			engine.LanczosPlan(object(), 4, 10, 3, **kw)
	for basis in ("nope", None, 2):
		with pytest.raises(ValueError):
			engine.fun_action_batch(object(), np.ones((8, 2)), 5, basis=basis)
		with pytest.raises(ValueError):
			MatrixFunction(np.eye(8), "exp", basis=basis)
	with pytest.raises(ValueError, match="callable"):
		MatrixFunction(np.eye(8), np.exp, basis="recompute")
	with pytest.raises(ValueError):
		engine.plan_query_bytes(np.float64, 100, 4, 10, 3, basis="auto")
	M = object.__new__(MatrixFunction)
	M._adaptive, M._basis = None, "auto"
	M.shape, M.dtype = (8, 8), np.dtype(np.float64)
	for call in (
		lambda: distributed.sharded_xtrace(M, 16),
		lambda: distributed.sharded_xtrace(M, 16, sketches="rows"),
		lambda: distributed.sharded_diag_device(object(), 16, 20, basis="auto"),
	):
		with pytest.raises(ValueError, match="auto"):
			call()
	with pytest.raises(ValueError):
		distributed.sharded_diag_device(object(), 16, 20, basis="nope")
	plan = object.__new__(engine.LanczosPlan)
	plan._h, plan.basis_kind = None, "recompute"
	with pytest.raises(ValueError, match="no basis"):
		plan.basis(0)


def test_basis_argument_resolution():
	from primate_amd import engine

	assert engine._basis_arg(False, None) is None
	assert engine._basis_arg(True, None) == "keep"
	assert engine._basis_arg(True, "keep") == "keep"
	assert engine._basis_arg(False, "keep") == "keep"
	assert engine._basis_arg(False, "recompute") == "recompute"
	assert engine._basis_arg(False, "auto", auto=True) == "auto"


@pytest.mark.parametrize("which", ["lap2d", "graph"])
@pytest.mark.parametrize("deg", [30, 120])
def test_forward_and_reverse_sums_differ_by_at_most_the_derived_bound(oracle, which, deg):
	"""The premise of the GPU test against the kept basis: the recompute plan adds g_t W_t for t = 0 .. deg - 1, the kept-basis
	combiner for t = deg - 1 .. 0; each partial sum is rounded once, so the two differ elementwise by at most
	deg eps sum_t |g_t| |W_t[row]|, and the test allows twice that for the rounding of g_t. Here on the oracle's bases with
	NumPy sums, which round every product as well: deg + 2 in place of deg."""
	A = laplacian_2d(24) if which == "lap2d" else random_spd_graph(600, 6.0, seed=3)
	n = A.shape[0]
	rng = np.random.default_rng(7)
	f = lambda x: np.exp(-0.1 * x)  # noqa: E731
	for orth in (0, 3, deg):
		v = rng.standard_normal(n)
		al, be, Q = np.zeros(deg + 1), np.zeros(deg + 1), np.zeros((n, deg), order="F")
		steps = oracle.lanczos(A, v.copy(), deg, 1e-8, orth, al, be, Q)
		assert steps == deg
		c = action_coeffs(al, be, deg, f)
		xnorm = np.linalg.norm(v)
		for dtype in (np.float64, np.float32):
			eps = float(np.finfo(dtype).eps)
			g = (xnorm * c).astype(dtype)
			fwd, rev = ordered_sum(Q, g, dtype, reverse=False), ordered_sum(Q, g, dtype, reverse=True)
			bound = 2.0 * order_bound(Q, c, xnorm, deg + 2, eps)
			diff = np.abs(fwd.astype(np.float64) - rev.astype(np.float64))
			assert np.all(diff <= bound), (which, deg, orth, dtype, float(np.max(diff / np.maximum(bound, 1e-300))))
