"""The marginal likelihood through the preconditioner, what needs no GPU: the host model's exact part
tr(P^-1 dA/dtheta) (`PreconditionedKernelOperator.trace_grad_exact`, float64 NumPy from H) against the dense inverse inside half of the
bar the device is held to, H itself, the identity between the two forms of the estimator on explicit probes, the `auto` rule, the
statistics that motivate it - the control variate wins with a good factor and loses with a poor one - as a seeded regression, the
C-ABI symbols and the refusals that now point to gp.logdet_grad. (scripts/gp_mll_check.cpp runs precond_finish's H under the host
sanitizers as a program of its own.)

Measured here (error / bar of the emulation, worst component): n1 0.013, n40-matern12 0.032, n400-matern32 0.0015, n40-matern52 0.025,
early stop 0.46 - there the noise component's bar is 100 eps of a value of 3e7, and what fills it is the rounding of the Gram matrix
L^T L that H is the inverse of, amplified by 1 / sigma2: not a term of the bar, which takes H as given."""

import re
from pathlib import Path

import numpy as np
import pytest

import _gp_mll_ref as M
import _kernelgrad_ref as G
import _kernelop_ref as R
from primate_amd import _capi, gp
from primate_amd.operators import KernelOperator

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_kernel_precond_columns", "slq_kernel_precond_trace_grad", "slq_debug_kernel_precond_h")
IDS = [M.case_id(c) for c in M.CASES]


def test_symbols_are_declared_exported_and_bound():
	hdr = (ROOT / "include" / "slq.h").read_text()
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint {s}\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"
	ver = L.slq_version
	ver.restype = int
	assert ver() == 100
	assert L.slq_kernel_precond_columns(None, 0, 0, 1, None, 0) == _capi.SLQ_EINVAL
	assert L.slq_kernel_precond_trace_grad(None, None, 1.0, 0.0) == _capi.SLQ_EINVAL
	assert L.slq_debug_kernel_precond_h(None, None) == _capi.SLQ_EINVAL


@pytest.mark.parametrize("c", M.CASES, ids=IDS)
def test_exact_part_of_the_host_model(c):
	"""trace_grad_exact() against tr(P^-1 D) of the dense inverse on the same L: the bar discriminates (<= 1e-6 max |g| per group),
	and the float64 emulation stays inside half of it. H is the inverse of L^T L + sigma2 I."""
	n, d, name, ell, s, sigma2, rank, note = c
	B = M.operator(c).preconditioned(rank)
	hm = B.host_model()
	L, H = hm["L"], hm["H"]
	if c is M.EARLY_STOP:
		assert B.rank < min(rank, n)
	g, bar, trD = M.exact_model(c, L, H)
	ratio = G.check_condition(g, bar) if n > 1 else 0.0  # (one point: the lengthscale group is exactly 0 with a bar of 0)
	got = B.trace_grad_exact()
	frac = G.worst(got, g, bar)
	print(f"[gp-mll-cpu] {M.case_id(c)}: rank {B.rank} bar / max|g| {ratio:.2e} emulation error / bar {frac:.3f}")
	assert frac <= 0.5
	r = L.shape[1]
	resid = H @ (L.T @ L + sigma2 * np.eye(r)) - np.eye(r)
	cond = (float(np.max(hm["t"])) + sigma2) / sigma2
	assert np.array_equal(H, H.T) or np.allclose(H, H.T, rtol=0, atol=64 * np.finfo(float).eps * r / sigma2)
	assert float(np.max(np.abs(resid))) <= 64 * np.finfo(float).eps * r * cond
	## the device's entry point with explicit factors is the same function
	assert np.array_equal(B.trace_grad_exact(L=L, H=H), got)


def _dense_setup(n, d, name, ell, s, sigma2, rank, seed):
	X = R.points(n, d, seed=seed)
	K = KernelOperator(X, name, lengthscale=ell, outputscale=s, noise=sigma2)
	z = K.scaled_points().astype(np.float64)
	B = K.preconditioned(rank)
	L = B.host_model()["L"]
	A = M.dense_a(z, name, s, sigma2).astype(np.float64)
	D = M.dense_D(z, name, ell, s).astype(np.float64)
	Minv, cond = M.minv_dense(L, sigma2)
	return K, B, L, A, D, Minv


def test_the_two_forms_differ_by_the_control_variate():
	"""on - off = tr(P^-1 D) - mean_c (M w_c)^T D (M w_c) on explicit probes, for every component."""
	n, sigma2 = 40, 1e-3
	K, B, L, A, D, Minv = _dense_setup(n, 3, "matern52", 0.5, 1.3, sigma2, 12, seed=5)
	W = M.rademacher(n, 16, seed=3)
	on, _, Vm = M.estimator_terms(A, Minv, D, W, True)
	off, _, _ = M.estimator_terms(A, Minv, D, W, False)
	exact = M.trace_inv(M.inv_ld(M.dense_p(L, sigma2)), D.astype(M.LD)).astype(np.float64)
	cv = np.array([np.mean(np.einsum("ic,ic->c", Vm, Dk @ Vm)) for Dk in D])
	lhs = (exact + on.mean(axis=0)) - off.mean(axis=0)
	assert np.allclose(lhs, exact - cv, rtol=1e-9, atol=1e-9 * float(np.max(np.abs(exact))))
	## and both are estimates of tr(A^-1 D): with n probes spanning the space (W W^T = n I for a Hadamard-like set) they are exact;
	## here: the mean over MANY probes approaches it - checked loosely, the sharp statement is the identity above
	full = M.trace_inv(M.inv_ld(A.astype(M.LD)), D.astype(M.LD)).astype(np.float64)
	Wm = M.rademacher(n, 4096, seed=4)
	est = exact + M.estimator_terms(A, Minv, D, Wm, True)[0].mean(axis=0)
	se = M.estimator_terms(A, Minv, D, Wm, True)[0].std(axis=0, ddof=1) / np.sqrt(4096)
	assert np.all(np.abs(est - full) <= 5 * se + 1e-9 * np.abs(full))


def test_auto_rule_and_ritz_values():
	assert gp.control_variate_auto(1.99) is True and gp.control_variate_auto(2.0) is True and gp.control_variate_auto(2.01) is False
	## the largest eigenvalue of the tridiagonals, probe by probe, honouring the steps each took
	rng = np.random.default_rng(0)
	deg = 6
	a, b = rng.uniform(1.0, 2.0, (3, deg + 1)), rng.uniform(0.1, 0.5, (3, deg + 1))
	b[:, 0] = 0.0
	steps = np.array([deg, 3, 1], dtype=np.int32)
	want = -np.inf
	for i, k in enumerate(steps):
		T = np.diag(a[i, :k]) + np.diag(b[i, 1:k], 1) + np.diag(b[i, 1:k], -1)
		want = max(want, float(np.linalg.eigvalsh(T)[-1]))
	assert gp.ritz_max(a, b, steps) == want
	assert gp.ritz_max(np.array([[1.5, 9.0]]), np.array([[0.0, 9.0]]), np.array([1])) == 1.5  # (entries beyond the steps are not read)


## the issue's table: (n, d, profile, lengthscale, sigma2, rank, control variate wins?)
TABLE = ((400, 2, "rbf", 0.3, 1e-4, 64, True), (400, 2, "rbf", 0.3, 1e-4, 16, False), (300, 2, "matern32", 0.3, 1e-3, 64, False))


@pytest.mark.parametrize("row", TABLE, ids=[f"n{r[0]}-{r[2]}-r{r[5]}" for r in TABLE])
def test_control_variate_statistics(row):
	"""Exact dense solves, 32 seeded Rademacher probes: the standard error of every component with the control variate on against off.
	Only the ordering is asserted - on below off where lambda_max(B) <= 2, above it where the factor is poor (the lengthscale and
	outputscale components; the noise component's two errors are close there) - and lambda_max(B) against the rule's threshold."""
	n, d, name, ell, sigma2, rank, wins = row
	K, B, L, A, D, Minv = _dense_setup(n, d, name, ell, 1.0, sigma2, rank, seed=n)
	Bd = Minv @ A @ Minv
	lam_max = float(np.linalg.eigvalsh(0.5 * (Bd + Bd.T))[-1])
	W = M.rademacher(n, 32, seed=11)
	on = M.estimator_terms(A, Minv, D, W, True)[0]
	off = M.estimator_terms(A, Minv, D, W, False)[0]
	fold = lambda v: np.concatenate([v[:, :d].sum(axis=1, keepdims=True), v[:, d:]], axis=1)  # noqa: E731  (a scalar lengthscale)
	se_on, se_off = (fold(v).std(axis=0, ddof=1) / np.sqrt(32) for v in (on, off))
	print(f"[gp-mll-cpu] n {n} {name} sigma2 {sigma2:g} rank {rank}: lambda_max(B) {lam_max:.4g}  off {se_off}  on {se_on}")
	assert gp.control_variate_auto(lam_max) is wins
	if wins:
		assert np.all(se_on < se_off)
	else:
		assert np.all(se_on[:2] > se_off[:2])


def test_refusals_point_to_logdet_grad():
	from primate_amd import autograd, grad
	from primate_amd.operators import MatrixFunction

	K = KernelOperator(R.points(12, 2, seed=1), noise=0.1)
	B = K.preconditioned(4)

	class FakeM(MatrixFunction):
		def __init__(self):
			self._A, self.dtype = B, np.dtype(np.float64)

	with pytest.raises(ValueError, match="gp.logdet_grad"):
		grad.kernel_trace_grad(FakeM())
	with pytest.raises(ValueError, match="gp.logdet_grad"):
		grad.trace_grad(FakeM(), None)
	with pytest.raises(ValueError, match="gp.logdet_grad"):
		grad.kernel_quadratic_grad(B, np.ones(12))
	with pytest.raises(ValueError, match="gp.logdet_grad"):
		autograd.trace_fun(B)
	## argument checks that touch no device
	with pytest.raises(ValueError, match="KernelOperator"):
		gp.logdet_grad(np.eye(3))
	with pytest.raises(ValueError, match="KernelOperator"):
		gp.mll(np.eye(3), np.ones(3))
	with pytest.raises(ValueError, match="count"):
		gp.logdet_grad(K, count=1)
	with pytest.raises(ValueError, match="fp64 only"):
		gp.mll(KernelOperator(R.points(12, 2, seed=1).astype(np.float32), noise=0.1), np.ones(12))
	with pytest.raises(ValueError, match="whole batches"):
		gp._batches(24, 16, np.zeros((12, 23)), 12, "logdet_grad")
	assert gp._batches(64, 16, None, 12, "x")[:2] == (4, 16) and gp._batches(20, 16, None, 12, "x")[:2] == (2, 10)
