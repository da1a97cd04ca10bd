"""The pivoted-Cholesky preconditioner of the kernel operator, what needs no GPU: the NumPy model of the factor
on the issue's case table inside half of every bar of tests/_kernelprecond_ref.py (the device is held to the whole bar), the early
stop, M = P^{-1/2} without an orthonormal basis against eigh, the two log-determinant identities, the claim that motivates the
feature - degree-20 Lanczos is exact to 1e-9 on B = M A M and off by more than 1 on A at noise 1e-4 -, the host
`PreconditionedKernelOperator` against the same models, the C-ABI symbols and the refusals raised before a device is touched.
(scripts/kernelprecond_check.cpp runs the host part of csrc/slq_kernelprecond.hpp under the host sanitizers as a program of its own.)"""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _kernelop_ref as R
import _kernelprecond_ref as P
from primate_amd import _capi
from primate_amd.operators import KernelOperator, PreconditionedKernelOperator, precond_g

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_kernel_precond_create", "slq_kernel_precond_refresh", "slq_kernel_precond_info", "slq_kernel_precond_get",
			   "slq_kernel_precond_apply", "slq_kernel_precond_apply_dmat", "slq_debug_kernel_precond_addresses", "slq_debug_kernel_precond_timing")  # fmt: skip
IDS = [P.case_id(c) for c in P.CASES]


def test_symbols_are_declared_exported_and_bound():
	hdr = (ROOT / "include" / "slq.h").read_text()
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint {s}\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"
	shape = (ROOT / "primate_amd" / "csrc" / "slq_plan_shape.hpp").read_text()
	assert re.search(r"\bOP_KERNEL_PRECOND = 6\b", shape) and _capi.OP_KERNEL_PRECOND == 6


_models = {}


def emulated(c):
	"""(L, pivots, d) of the float64 emulation of the definition on the norms-plus-dot K0: once per case."""
	if c not in _models:
		z, K0, dK = P.k0_model(c)
		_models[c] = P.factor(P.emulate_k0(z, c[2], c[4]), c[4], c[6])
	return _models[c]


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_factor_model_properties(c):
	"""Distinct pivots, d >= 0, (L L^T)[p, :] = K0[p, :] at every pivot, the greedy choice at every step: the float64 emulation at 0.5
	of the bars the device is held to at 1.0."""
	L, piv, d = emulated(c)
	assert np.all(d >= 0)
	got = P.check_factor(c, L, piv, 0.5, "emulation")
	if c is P.EARLY_STOP:
		assert got["rank"] == 9 and got["rank"] < c[6]  # (the model of the issue: rank 9 of 64)
	else:
		assert got["rank"] == min(c[6], c[0])


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_inverse_square_root_and_logdet(c):
	"""M = (I - L G L^T) / sigma from the r x r eigendecomposition is within 16 eps cond(P) max |ref| of eigh(P)^{-1/2}; logdet P from
	the same eigenvalues is within 1e-9 n of slogdet(P); logdet P + logdet(M A M) = logdet A to 1e-9 |logdet A|. The host operator's
	`inv_sqrt`, `_matmat`, `logdet_precond`, `rank` and `pivots` are the model's."""
	n, d, name, ell, s, sigma2, rank, _ = c
	L, piv, dres = emulated(c)
	K = P.operator(c)
	B = K.preconditioned(rank)
	assert isinstance(B, PreconditionedKernelOperator) and B._slq_kind == "kernel_precond" and B.dtype == np.float64 and B.shape == (n, n) and B.base is K
	m = B.host_model()
	r = int(np.sum(piv >= 0))
	assert B.rank == r and np.array_equal(B.pivots, piv[:r])
	assert B.residual_trace == pytest.approx(float(np.sum(dres)), rel=1e-6, abs=1e-12 * n * s)
	Minv, cond, logdet_p, Pm = P.dense_p(m["L"], sigma2)
	X = R.probes(n, 7, seed=n)
	ref = Minv @ X
	got = B.inv_sqrt(X)
	frac = float(np.max(np.abs(got - ref))) / P.apply_bar(cond, ref)
	print(f"[kernelprecond-cpu] {P.case_id(c)}: cond(P) {cond:.2e} M error / (16 eps cond max|ref|) {frac:.3f} logdet P {B.logdet_precond:.6f} (slogdet {logdet_p:.6f})")
	assert frac <= 1.0
	assert abs(B.logdet_precond - logdet_p) <= 1e-9 * n
	A = R.dense_matrix(P.k0_model(c)[0], name, s, sigma2)
	logdet_a = float(np.linalg.slogdet(A)[1])
	Bd = Minv @ A @ Minv
	logdet_b = float(np.linalg.slogdet(0.5 * (Bd + Bd.T))[1])
	assert abs(B.logdet_precond + logdet_b - logdet_a) <= 1e-9 * abs(logdet_a)
	## the host product is M A M
	Y = B @ X
	want = Minv @ (A @ (Minv @ X))
	lim = 64 * np.finfo(np.float64).eps * cond * np.linalg.norm(A, 2) / sigma2 * float(np.max(np.abs(X))) * np.sqrt(n)
	assert float(np.max(np.abs(Y - want))) <= lim
	assert np.allclose(B @ X[:, 0], Y[:, 0], rtol=0, atol=lim)  # (_matvec is _matmat on one column)


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_product_emulation_fits_half_the_bar(c):
	"""The host operator's B X - float64 NumPy from the definition - on 260 columns against the model of
	_kernelprecond_ref.product_model, at 0.5 of the bar the device's product is held to at 1.0."""
	n = c[0]
	B = P.operator(c).preconditioned(c[6])
	X = R.probes(n, max(P.COLUMN_COUNTS), seed=n + 1)
	Y, bar = P.product_model(c, B.host_model()["L"], X)
	got = B @ X
	frac = float(np.max(np.max(np.abs(got - Y), axis=0) / bar))
	print(f"[kernelprecond-cpu] {P.case_id(c)}: product emulation error / bar {frac:.2e} (bar / max|Y| {float(np.max(bar / np.max(np.abs(Y), axis=0))):.2e})")
	assert frac <= 0.5


def test_g_is_smooth_and_monotone():
	t = np.array([0.0, 5e-324, 1e-300, 1e-30, 1e-20, 1e-10, 1e-6, 1e-3, 1.0, 1e3, 1e8])
	for sigma2 in (1e-6, 1.0, 100.0):
		g = precond_g(t * sigma2, sigma2)
		assert np.all(np.isfinite(g)) and g[0] == 0.5 / sigma2 and np.all(np.diff(g) <= 0)
		big = t >= 1e-3
		assert np.allclose(g[big], (1 - 1 / np.sqrt(1 + t[big])) / (t[big] * sigma2), rtol=1e-12)
	assert precond_g(np.array([-1e-12]), 2.0)[0] == 0.25


def test_lanczos_needs_the_preconditioner(oracle):
	"""The claim of the issue's table as a test: n = 400 uniform points in [0, 1]^2, rbf, lengthscale 0.3, s = 1, noise 1e-4, rank 64.
	The oracle's degree-20 Gauss rule for v^T log(.) v is within 1e-9 of the exact value on the dense B = M A M for every one of 16
	Rademacher probes, and off by more than 1 on the dense A."""
	n, deg = 400, 20
	X = R.points(n, 2, seed=400)
	K = KernelOperator(X, "rbf", lengthscale=0.3, outputscale=1.0, noise=1e-4)
	B = K.preconditioned(64)
	A = R.dense_matrix(K.scaled_points(), "rbf", 1.0, 1e-4)
	Minv, cond, _, _ = P.dense_p(B.host_model()["L"], 1e-4)
	Bd = Minv @ A @ Minv
	Bd = 0.5 * (Bd + Bd.T)
	rng = np.random.default_rng(11)
	V = np.asfortranarray(np.floor(rng.random((n, 16)) * 2) * 2 - 1)
	worst = {}
	for which, Mat in (("B", Bd), ("A", A)):
		lam, U = np.linalg.eigh(Mat)
		exact = np.sum((U.T @ V) ** 2 * np.log(lam)[:, None], axis=0)
		got = oracle.quad_batch(np.asfortranarray(Mat), V, deg, deg, fun="log", fresh_q=True)
		worst[which] = (float(np.max(np.abs(got - exact))), float(np.min(np.abs(got - exact))), float(lam[-1] / lam[0]))
	print(f"[kernelprecond-cpu] deg-20 Gauss rule for v^T log v: worst error on B {worst['B'][0]:.2e} (cond {worst['B'][2]:.3f}); on A worst {worst['A'][0]:.2e}, best {worst['A'][1]:.2e} (cond {worst['A'][2]:.2e})")
	assert worst["B"][0] <= 1e-9
	assert worst["A"][0] > 1.0


def test_host_refusals():
	X = R.points(12, 2, seed=1)
	with pytest.raises(ValueError, match="noise > 0"):
		KernelOperator(X, noise=0.0).preconditioned(4)
	with pytest.raises(ValueError, match="fp64 only"):
		KernelOperator(X.astype(np.float32), noise=0.1).preconditioned(4)
	K = KernelOperator(X, noise=0.1)
	for bad in (0, 257, -3):
		with pytest.raises(ValueError, match="rank"):
			K.preconditioned(bad)
	with pytest.raises(ValueError, match="tol"):
		K.preconditioned(4, tol=-1.0)
	with pytest.raises(ValueError, match="KernelOperator"):
		PreconditionedKernelOperator(np.eye(3), 2)
	assert K.preconditioned(100).rank_max == 12  # (clamped to n)
	## the gradient entries say that the new kind is not theirs
	from primate_amd import grad
	from primate_amd.operators import MatrixFunction

	B = K.preconditioned(4)

	class FakeM(MatrixFunction):
		def __init__(self):
			self._A, self.dtype = B, np.dtype(np.float64)

	with pytest.raises(ValueError, match="preconditioner"):
		grad.kernel_trace_grad(FakeM())
	with pytest.raises(ValueError, match="preconditioned kernel operator"):
		grad.trace_grad(FakeM(), None)
	with pytest.raises(ValueError, match="preconditioner"):
		grad.kernel_quadratic_grad(B, np.ones(12))


def test_raw_entries_refuse_null_and_foreign_handles_without_a_device():
	L = _capi.lib()
	h = C.c_void_p()
	buf = np.zeros(4)
	assert L.slq_kernel_precond_create(None, None, 4, 0.0, C.byref(h)) == _capi.SLQ_EINVAL and b"NULL" in L.slq_last_error()
	assert L.slq_kernel_precond_refresh(None) == _capi.SLQ_EINVAL
	assert L.slq_kernel_precond_info(None, None, None, None, None, None) == _capi.SLQ_EINVAL
	assert L.slq_kernel_precond_get(None, None, None, 0, None, None) == _capi.SLQ_EINVAL
	assert L.slq_kernel_precond_apply(None, _capi.ptr(buf), 4, _capi.ptr(buf), 4, 1) == _capi.SLQ_EINVAL
	assert L.slq_kernel_precond_apply_dmat(None, None, 0, None, 0, 1) == _capi.SLQ_EINVAL
	assert L.slq_debug_kernel_precond_addresses(None, None) == _capi.SLQ_EINVAL
