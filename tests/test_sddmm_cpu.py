"""The sampled dense-dense product and the gradient of tr f(A), what needs no GPU: the C-ABI symbols, the NumPy
model of the GPU tests against a dense product, the host schedule of the kernel's work items (slq_debug_sddmm_schedule: pure
host logic - every stored nonzero owned exactly once), the derivative tables against central differences, and the argument
errors raised before the library is touched."""

import re
from pathlib import Path

import numpy as np
import pytest

import _sddmm_ref as R
from primate_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_sddmm_create", "slq_sddmm_create_device", "slq_sddmm_update", "slq_sddmm_get", "slq_sddmm_ptr", "slq_sddmm_reset",
			   "slq_sddmm_destroy", "slq_debug_sddmm_schedule")  # fmt: skip


def test_symbols_are_declared_exported_and_bound():
	hdr = (ROOT / "include" / "slq.h").read_text()
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint {s}\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"
	from primate_amd import autograd, engine, grad

	for name in ("update", "get", "cuda_array", "reset", "close"):
		assert callable(getattr(engine.SddmmAccumulator, name)), name
	assert callable(grad.trace_grad) and callable(autograd.trace_fun)


## ---- the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [False, True])
def test_model_equals_the_dense_product_on_the_pattern(symmetric):
	P = R.random_pattern()
	rows, cols = R.pattern_rows_cols(P)
	rng = np.random.default_rng(3)
	n, m = P.shape[0], 7
	W, Z = rng.standard_normal((n, m)), rng.standard_normal((n, m))
	old = rng.standard_normal(P.nnz)
	alpha, beta = 0.3, -1.25
	D = W @ Z.T
	if symmetric:
		D = 0.5 * (D + D.T)
	want = beta * old + alpha * D[rows, cols]
	got = R.vals_ld(rows, cols, W, Z, alpha, beta, old, symmetric)
	b = R.bar(rows, cols, W, Z, alpha, beta, old, symmetric)
	assert got.dtype == np.longdouble and b.shape == (P.nnz,) and np.all(b > 0)
	assert np.all(np.abs(want - got.astype(np.float64)) <= b)
	## beta = 0 ignores the old values (NaN included), and W may be Z
	nan_old = np.full(P.nnz, np.nan)
	g0 = R.vals_ld(rows, cols, W, W, 2.0, 0.0, nan_old, symmetric)
	assert np.all(np.abs((2.0 * (W @ W.T))[rows, cols] - g0.astype(np.float64)) <= R.bar(rows, cols, W, W, 2.0, 0.0, None, symmetric))


def test_patterns_are_what_the_gpu_tests_need():
	G, P, E = R.grid_pattern(), R.random_pattern(), R.empty_pattern()
	assert G.shape == (143, 143) and G.shape[0] % 64 != 0
	assert P.shape == (300, 300) and P.nnz % 64 != 0 and (abs(P - P.T)).nnz == 0
	lens = np.diff(P.indptr)
	assert lens.max() == 299 and lens.min() == 0
	assert E.nnz == 0


## ---- the schedule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["grid", "random", "empty"])
def test_schedule_owns_every_nonzero_exactly_once(which):
	from primate_amd.engine import sddmm_schedule

	P = {"grid": R.grid_pattern, "random": R.random_pattern, "empty": R.empty_pattern}[which]()
	n, nnz = P.shape[0], P.nnz
	S = sddmm_schedule(P.indptr)
	k = S["row0"].size
	owners = np.zeros(nnz, dtype=np.int64)
	lens = np.diff(P.indptr)
	for i in range(k):
		r0, nr, kind, e0, e1 = (int(S[key][i]) for key in ("row0", "nrows", "kind", "e0", "e1"))
		assert 0 <= r0 and nr >= 1 and r0 + nr <= n
		assert 0 <= e0 < e1 <= nnz, "an item owns a non-empty range inside the pattern"
		assert (e0, e1) == (P.indptr[r0], P.indptr[r0 + nr]), "the range is that of the item's rows"
		if kind == 1:
			assert nr == 1 and lens[r0] > S["long_row"]
		else:
			assert kind == 0 and nr <= 64 and r0 // 64 == (r0 + nr - 1) // 64, "a short item stays inside one aligned block of 64 rows"
			assert np.all(lens[r0 : r0 + nr] <= S["long_row"])
		owners[e0:e1] += 1
	assert np.all(owners == 1), f"{int(np.sum(owners != 1))} stored nonzeros are not owned exactly once"
	assert S["nlong"] == int(np.sum(lens > S["long_row"])) == int(np.sum(S["kind"] == 1))
	assert S["grid"] == -(-k // S["waves"])
	if which == "empty":
		assert k == 0 and S["grid"] == 0, "nnz = 0 launches nothing"
	if which == "random":
		assert S["nlong"] == 1


def test_schedule_refuses_a_bad_rowptr():
	from primate_amd.engine import sddmm_schedule

	with pytest.raises(ValueError, match="row 1"):
		sddmm_schedule(np.array([0, 3, 2, 4]))
	with pytest.raises(ValueError, match="rowptr\\[0\\]"):
		sddmm_schedule(np.array([1, 3, 4]))


## ---- the derivative tables ------------------------------------------------------------------------------------------
def _central(f, x, h):
	return (f(x + h) - f(x - h)) / (2.0 * h)


_CASES = [("identity", {}, (0.2, 3.0)), ("sqrt", {}, (0.5, 4.0)), ("log", {}, (0.5, 4.0)), ("inv", {}, (0.5, 4.0)), ("exp", {"t": -0.3}, (-2.0, 3.0)),
		  ("exp", {}, (-1.0, 1.0)), ("smoothstep", {"a": 0.5, "b": 2.5}, (0.6, 2.4)), ("smoothstep", {}, (0.05, 0.95))]  # fmt: skip


@pytest.mark.parametrize("name,kw,interval", _CASES)
def test_derivative_callables_against_central_differences(name, kw, interval):
	from primate_amd.grad import DERIVATIVE_NAMES, derivative_callable
	from primate_amd.special import param_callable

	assert name in DERIVATIVE_NAMES
	f, d = param_callable(name, **dict(kw)), derivative_callable(name, **kw)
	x = np.linspace(interval[0], interval[1], 22)[1:-1]  # 20 interior points
	np.testing.assert_allclose(np.asarray(d(x), dtype=np.float64), _central(f, x, 1e-5), rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("name,kw,interval", [("log", {}, (0.5, 4.0)), ("exp", {"t": -0.3}, (-2.0, 3.0)), ("exp", {}, (-1.0, 1.0))])
def test_lanczos_derivative_table_against_central_differences(name, kw, interval):
	from primate_amd.grad import lanczos_derivative
	from primate_amd.special import param_callable

	dname, dkw, scale = lanczos_derivative(name, kw)
	assert dname in _capi.FUN_IDS
	f, d = param_callable(name, **dict(kw)), param_callable(dname, **dict(dkw))
	x = np.linspace(interval[0], interval[1], 22)[1:-1]
	np.testing.assert_allclose(scale * d(x), _central(f, x, 1e-5), rtol=1e-6)


def test_tables_refuse_what_they_do_not_hold():
	from primate_amd.grad import derivative_callable, lanczos_derivative

	assert lanczos_derivative("identity", {}) is None
	for name in ("numrank", "sqrt", "inv", "abs", "smoothstep", "softsign"):
		with pytest.raises(ValueError, match="Chebyshev"):
			lanczos_derivative(name, {})
	for name in ("abs", "numrank", "softsign"):
		with pytest.raises(ValueError, match="dfun"):
			derivative_callable(name)
	with pytest.raises(ValueError, match="Unknown"):
		derivative_callable("cosh")


## ---- argument errors before the library is touched -------------------------------------------------------------------
def test_argument_errors_need_no_device():
	from primate_amd import autograd, engine, grad

	with pytest.raises(ValueError, match="MatrixFunction or a ChebyshevFunction"):
		grad.trace_grad(np.eye(3))
	with pytest.raises(ValueError, match="SciPy sparse matrix or a torch sparse-CSR"):
		engine.SddmmAccumulator(np.eye(3))
	with pytest.raises(ValueError, match="torch sparse-CSR"):
		autograd.trace_fun(np.eye(3))
	with pytest.raises(ValueError, match="device:sphere"):
		grad._probe_loader("device:sphere", 0, None, 10, 4, chebyshev=True)
	with pytest.raises(ValueError, match="Invalid distribution"):
		grad._probe_loader("device:cauchy", 0, None, 10, 4, chebyshev=False)
	with pytest.raises(ValueError, match="n x count"):
		grad._probe_loader(None, 0, np.zeros((9, 4)), 10, 4, chebyshev=False)
	with pytest.raises(ValueError, match="pdf must be"):
		grad._probe_loader(None, 0, None, 10, 4, chebyshev=False)


def test_trace_fun_refuses_a_host_tensor_and_an_unknown_method():
	import torch

	from primate_amd import autograd

	A = torch.sparse_csr_tensor(torch.tensor([0, 1, 2]), torch.tensor([0, 1]), torch.tensor([1.0, 2.0], dtype=torch.float64), size=(2, 2))
	with pytest.raises(ValueError, match="must live on the GPU"):
		autograd.trace_fun(A)
	with pytest.raises(ValueError, match="unknown method"):
		autograd.trace_fun(A, method="arnoldi")
	with pytest.raises(ValueError, match="torch sparse-CSR"):
		autograd.trace_fun(A.to_dense())
