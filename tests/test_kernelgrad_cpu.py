"""Hyperparameter gradients of the kernel operator, what needs no GPU: the C-ABI symbols, the long-double model
of the GPU tests against central differences of the dense matrix of `_kernelop_ref`, the condition and an fp64 emulation of the device
evaluation inside the bar for every GPU case, faults the bar must notice, the host schedule of an update, every refusal raised
before the library is touched, and the raw entries on NULL handles. (scripts/kernelgrad_check.cpp runs the host part of
csrc/slq_kernelgrad.hpp under the host sanitizers as a program of its own.)"""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _kernelgrad_ref as G
import _kernelop_ref as R
from primate_amd import _capi
from primate_amd.operators import KernelOperator, MatrixFunction

ROOT = Path(__file__).resolve().parent.parent
LD = np.longdouble
NEW_SYMBOLS = ("slq_kernel_grad_create", "slq_kernel_grad_update", "slq_kernel_grad_get", "slq_kernel_grad_reset", "slq_kernel_grad_destroy",
			   "slq_debug_kernel_grad_schedule")  # fmt: skip


def test_symbols_are_declared_exported_and_bound():
	hdr = (ROOT / "include" / "slq.h").read_text()
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint {s}\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"
	assert L.slq_version() == 100


## ---- the model against central differences ---------------------------------------------------------------------------------------
def _bilinear(X, name, ls, s, noise, Z, W) -> LD:
	"""sum C (.) A(theta) in long double with A the dense matrix of `_kernelop_ref` on the rounded z."""
	z = R.scaled_points(X, ls, np.float64)
	A = LD(s) * R.phi(name, R.r2_exact(z))
	A[np.diag_indices_from(A)] += LD(noise)
	return np.sum((Z.astype(LD) @ W.astype(LD).T) * A)


def _central(f, x: float, h: float):
	"""(derivative, its own error): the central difference at step h, and the h^2 remainder estimated from the step 2 h -
	|D(h) - D(2h)| / 3 - plus the rounding of the differenced values, eps |f| / h."""
	f1, f2 = (f(x + h) - f(x - h)) / (2 * h), (f(x + 2 * h) - f(x - 2 * h)) / (4 * h)
	return f1, abs(f1 - f2) / 3 + 4 * R.eps_of(np.float64) * abs(f(x)) / h


@pytest.mark.parametrize("name", R.PROFILES)
@pytest.mark.parametrize("d", [1, 3, 17])
def test_the_model_is_the_derivative_of_the_dense_matrix(name, d):
	"""The rounding of z to float64 makes sum C (.) A(l) a staircase in l at the scale eps: the differences see it as noise eps |f| / h,
	which is part of their own error. The tolerance is that error (printed), with a factor 4 on the remainder estimate."""
	n, m = 40, 3
	X = R.points(n, d, seed=d)
	ls = 0.4 * np.sqrt(d) * (1.0 + np.arange(d) / d)
	s, noise = 1.3, 0.1
	rng = np.random.default_rng(d)
	Z, W = rng.standard_normal((n, m)), rng.standard_normal((n, m))
	g, _ = G.model(R.scaled_points(X, ls, np.float64), name, ls, s, Z, W)
	h = 1e-4
	for k in sorted({0, d // 2, d - 1}):
		def f(v, k=k):
			l2 = ls.copy()
			l2[k] = v
			return _bilinear(X, name, l2, s, noise, Z, W)
		fd, err = _central(f, ls[k], h * ls[k])
		print(f"{name} d={d} l[{k}]: model {float(g[k]):.12e} differences {float(fd):.12e} +- {float(err):.2e}")
		assert abs(fd - g[k]) <= 4 * err + 1e-18, (name, d, k, float(fd - g[k]), float(err))
	fd, err = _central(lambda v: _bilinear(X, name, ls, v, noise, Z, W), s, h)
	assert abs(fd - g[d]) <= 4 * err + 1e-18, (name, "outputscale", float(fd - g[d]), float(err))
	fd, err = _central(lambda v: _bilinear(X, name, ls, s, v, Z, W), noise, h)
	assert abs(fd - g[d + 1]) <= 4 * err + 1e-18, (name, "noise", float(fd - g[d + 1]), float(err))
	## a scalar lengthscale's gradient is the sum over the dimensions
	gs, _ = G.model(R.scaled_points(X, 0.7, np.float64), name, 0.7, s, Z, W)
	fd, err = _central(lambda v: _bilinear(X, name, v, s, noise, Z, W), 0.7, h * 0.7)
	assert abs(fd - np.sum(gs[:d])) <= 4 * err + 1e-18, (name, "scalar lengthscale", float(fd - np.sum(gs[:d])), float(err))


## ---- the condition, and an emulation inside the bar, for every GPU case ------------------------------------------------------------
@pytest.mark.parametrize("case", G.GPU_CASES, ids=[G.case_id(c) for c in G.GPU_CASES])
def test_condition_and_emulation_for_every_gpu_case(case):
	(X, ls, s, noise, Z, W), z, g, bar = G.case_model(case)
	ratio = G.check_condition(g, bar)
	w = G.worst(G.emulate(z, case[3], ls, s, Z, W), g, bar)
	print(f"{G.case_id(case)}: bar / max |g| = {ratio:.2e}, emulation / bar = {w:.3f}")
	assert np.all(np.isfinite(g.astype(np.float64))) and w <= 1.0, (case, w)


def test_the_bar_notices_a_dropped_remainder_tile():
	case = (257, 8, 65, "rbf", False, 0.0, False)
	(X, ls, s, noise, Z, W), z, g, bar = G.case_model(case)
	assert G.worst(G.emulate(z, "rbf", ls, s, Z, W, jmax=256), g, bar) > 1e3


def test_the_bar_notices_a_wrong_sign_of_one_difference():
	case = (257, 8, 65, "rbf", False, 0.0, False)
	(X, ls, s, noise, Z, W), z, g, bar = G.case_model(case)
	bad, _ = G.model(z, "rbf", ls, s, Z, W, flip=(40, 41, 2))
	assert G.worst(bad.astype(np.float64), g, bar) > 1e3
	assert bad[0] == g[0] and bad[8] == g[8]  # (one dimension only)


def test_matern12_with_duplicate_rows_is_finite():
	X = R.points(30, 2)
	X[7] = X[3]
	X[11] = X[3]
	z = R.scaled_points(X, 0.5, np.float64)
	assert np.array_equal(z[7], z[3])
	W = R.probes(30, 4)
	g, bar = G.model(z, "matern12", 0.5, 2.0, W, W)
	e = G.emulate(z, "matern12", 0.5, 2.0, W, W)
	assert np.all(np.isfinite(g.astype(np.float64))) and np.all(np.isfinite(bar.astype(np.float64))) and np.all(np.isfinite(e))
	assert np.all(G.chi("matern12", np.zeros(3)) == 0.0)


## ---- the schedule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 127, 128, 129, 1000, 20000])
def test_schedule_partitions_rows_points_and_columns(n):
	from primate_amd.engine import kernel_grad_schedule

	for m in (1, 63, 64, 65, 128, 300):
		for cus in (256, 8, 1):
			S = kernel_grad_schedule(n, m, cus)
			assert S["rows"] == 128 and S["nrb"] == -(-n // 128)
			owners = np.zeros(n, dtype=int)
			for b in range(S["nrb"]):
				owners[b * S["rows"] : min(n, (b + 1) * S["rows"])] += 1
			assert np.all(owners == 1)
			assert S["chunk_cols"] == 64 and (S["chunks"] - 1) * 64 < m <= S["chunks"] * 64
			b = S["begin"]
			assert 1 <= S["slabs"] <= 16 and b[0] == 0 and b[-1] == n and all(x < y for x, y in zip(b, b[1:]))
			assert all(x % 16 == 0 for x in b[:-1]) and all(v == -1 for v in S["rest"]) and S["slabs"] <= -(-n // 16)
			owners = np.zeros(n, dtype=int)
			for x, y in zip(b, b[1:]):
				owners[x:y] += 1
			assert np.all(owners == 1)
			## the addition limit the bar assumes: a lane's run over its slab, lanes, waves, the partials of one launch
			assert (b[1] - b[0] + 15) + 4 + 8 + S["nrb"] * S["slabs"] <= 2 * n + 64


def test_schedule_entry_checks_its_arguments():
	L = _capi.lib()
	out = (C.c_int64 * 22)()
	assert L.slq_debug_kernel_grad_schedule(100, 64, 256, out, 21) == _capi.SLQ_EINVAL
	assert L.slq_debug_kernel_grad_schedule(100, 64, 256, None, 22) == _capi.SLQ_EINVAL
	for args in ((0, 64, 256), (100, 0, 256), (100, 64, 0), (1 << 31, 64, 256)):
		assert L.slq_debug_kernel_grad_schedule(*args, out, 22) == _capi.SLQ_EINVAL, args


def test_raw_entries_refuse_null_handles_without_a_device():
	L = _capi.lib()
	h = C.c_void_p()
	cnt = C.c_int64()
	vals = np.zeros(3)
	assert L.slq_kernel_grad_create(None, None, C.byref(h)) == _capi.SLQ_EINVAL
	assert L.slq_kernel_grad_create(None, None, None) == _capi.SLQ_EINVAL
	assert L.slq_kernel_grad_update(None, None, 0, None, 0, 1, 1.0, 1.0) == _capi.SLQ_EINVAL
	assert L.slq_kernel_grad_get(None, _capi.ptr(vals), 3, C.byref(cnt)) == _capi.SLQ_EINVAL
	assert L.slq_kernel_grad_reset(None) == _capi.SLQ_EINVAL
	assert L.slq_kernel_grad_destroy(None) == _capi.SLQ_OK


## ---- refusals, before the library is touched ---------------------------------------------------------------------------------------
X5 = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 1.0], [6.0, 8.0], [3.0, 4.0]])


def _fake_function(K, dtype=np.float64, builtin=("log", {}), stale=False, adaptive=None):
	M = MatrixFunction.__new__(MatrixFunction)  # (no device here: every refusal comes before anything is run)
	M._A, M.dtype, M.shape = K, np.dtype(dtype), K.shape
	M._builtin, M._stale_ring, M._adaptive = builtin, stale, adaptive
	return M


def test_every_python_refusal():
	import scipy.sparse as sp

	from primate_amd import engine, grad
	from primate_amd.chebyshev import ChebyshevFunction

	K = KernelOperator(X5, noise=0.1)
	with pytest.raises(ValueError, match="MatrixFunction or a ChebyshevFunction"):
		grad.kernel_trace_grad(K)
	with pytest.raises(ValueError, match="KernelOperator"):
		grad.kernel_trace_grad(_fake_function(sp.identity(5, format="csr")))
	with pytest.raises(ValueError, match="fp64 only"):
		grad.kernel_trace_grad(_fake_function(KernelOperator(X5.astype(np.float32)), dtype=np.float32))
	with pytest.raises(ValueError, match="fp64 only"):
		grad.kernel_trace_grad(_fake_function(KernelOperator(X5.astype(np.float32))))
	with pytest.raises(ValueError, match="stale_ring"):
		grad.kernel_trace_grad(_fake_function(K, stale=True))
	with pytest.raises(ValueError, match="adaptive"):
		grad.kernel_trace_grad(_fake_function(K, adaptive=dict(deg_max=40)))
	with pytest.raises(ValueError, match="built-in"):
		grad.kernel_trace_grad(_fake_function(K, builtin=None))
	with pytest.raises(ValueError, match="not a built-in spectral function"):
		grad.kernel_trace_grad(_fake_function(K, builtin=("sqrt", {})))
	with pytest.raises(ValueError, match="must be >= 1"):
		grad.kernel_trace_grad(_fake_function(K), count=0)
	with pytest.raises(ValueError, match="Invalid distribution"):
		grad.kernel_trace_grad(_fake_function(K), pdf="cauchy")
	with pytest.raises(ValueError, match="n x count"):
		grad.kernel_trace_grad(_fake_function(K), probes=np.ones((4, 3)))
	Mc = ChebyshevFunction.__new__(ChebyshevFunction)
	Mc._A, Mc.dtype, Mc.shape = K, np.dtype(np.float64), K.shape
	Mc._fun = grad.param_callable("log")
	with pytest.raises(ValueError, match="device:sphere"):
		grad.kernel_trace_grad(Mc, pdf="device:sphere")
	Mc._fun = np.log
	with pytest.raises(ValueError, match="built-in"):
		grad.kernel_trace_grad(Mc)
	## identity needs no device at all: it is exact
	est, grads, info = grad.kernel_trace_grad(_fake_function(K, builtin=("identity", {})), count=4)
	assert est == 5 * (1.0 + 0.1) and grads["outputscale"] == 5.0 and grads["noise"] == 5.0 and np.array_equal(grads["lengthscale"], [0.0])
	assert info["acc_count"] == 0 and info["count"] == 4
	## the quadratic form and the accumulator
	with pytest.raises(ValueError, match="KernelOperator"):
		grad.kernel_quadratic_grad(sp.identity(5, format="csr"), np.ones(5))
	with pytest.raises(ValueError, match="fp64 only"):
		grad.kernel_quadratic_grad(KernelOperator(X5.astype(np.float32)), np.ones(5))
	with pytest.raises(ValueError, match="one shape"):
		grad.kernel_quadratic_grad(K, np.ones(4))
	with pytest.raises(ValueError, match="one shape"):
		grad.kernel_quadratic_grad(K, np.ones((5, 2)), np.ones((5, 3)))

	class _Op:
		kind, dtype = "csr", np.dtype(np.float64)

	with pytest.raises(ValueError, match="kind 'csr'"):
		engine.KernelGradAccumulator(_Op())
	_Op.kind, _Op.dtype = "kernel", np.dtype(np.float32)
	with pytest.raises(ValueError, match="fp64 only"):
		engine.KernelGradAccumulator(_Op())


def test_the_older_entries_point_to_the_new_ones():
	from primate_amd import autograd, grad

	K = KernelOperator(X5, noise=0.1)
	with pytest.raises(ValueError, match="hyperparameter gradients.*kernel_trace_grad"):
		grad.trace_grad(_fake_function(K))
	with pytest.raises(ValueError, match="hyperparameter gradients.*kernel_trace_fun"):
		autograd.trace_fun(K)
	with pytest.raises(ValueError, match="unknown method"):
		autograd.kernel_trace_fun(X5, "rbf", 1.0, 1.0, 0.1, method="pade")
