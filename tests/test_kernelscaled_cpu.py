"""The diagonally scaled kernel operator without a GPU: the host model of KernelOperator(diag_scale=) against the
long-double model of tests/_kernelscaled_ref.py, the validation messages, every Python refusal of a scaled operator - raised before
the library is touched - and the declaration of the three new ABI symbols. The cases the GPU test runs are checked here for
R.check_condition: the bar must stay a small fraction of the result, or passing it says nothing."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _kernelop_ref as R
import _kernelscaled_ref as S
from primate_amd import _capi
from primate_amd.operators import KernelOperator, MatrixFunction

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_kernel_set_diag_scale", "slq_kernel_get_diag_scale", "slq_debug_kernel_diag_scale")


def test_symbols_are_declared_exported_bound_and_cited():
	hdr = (ROOT / "include" / "slq.h").read_text()
	doc = (ROOT / "INTEGRATION.md").read_text()
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint {s}\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"
		assert s in doc, f"{s} is not cited in INTEGRATION.md"
	assert L.slq_kernel_set_diag_scale(None, None, 0) == _capi.SLQ_EINVAL
	assert L.slq_kernel_get_diag_scale(None, None, 0, None) == _capi.SLQ_EINVAL
	assert L.slq_debug_kernel_diag_scale(None, None) == _capi.SLQ_EINVAL


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("name", R.PROFILES)
def test_host_matmat_against_the_model(name, dtype):
	"""The host _matmat (float64 NumPy from the definition, on the rounded z and c) within the model's bar for the operator's dtype - in
	float32 the bar is that of an fp32 evaluation, which a float64 one sits far inside; what is checked is that the two agree on WHAT is
	computed: c on both sides, the diagonal s c_i^2 + sigma2, rows with c_i = 0 equal to sigma2 e_i^T."""
	n, d, ell, s, noise = 130, 3, 0.5, 1.3, 0.05
	X = R.points(n, d, seed=4, dtype=dtype)
	W = R.probes(n, 7, seed=4, dtype=dtype)
	c = S.scale(n, 4, dtype)
	K = KernelOperator(X, name, lengthscale=ell, outputscale=s, noise=noise, dtype=dtype, diag_scale=c.astype(np.float64))
	assert K.diag_scale.dtype == np.dtype(dtype) and np.array_equal(K.diag_scale, c)
	z = R.scaled_points(X, ell, dtype)
	Y, bar = S.model(z, name, s, noise, c, W)
	R.check_condition(Y, bar, dtype)
	got = K._matmat(W)
	if dtype == np.float64:
		assert S.worst(got, Y, bar) <= 1.0
	else:  # (the result was rounded to fp32 once more: half an ulp of it on top of the bar)
		assert np.all(np.abs(got.astype(S.LD) - Y) <= bar + S.LD(R.eps_of(dtype)) * np.abs(Y))
	A = K.rows(np.arange(n))
	c64 = c.astype(np.float64)
	assert np.allclose(np.diag(A), s * c64 * c64 + noise, rtol=1e-15, atol=0) and np.allclose(A, A.T, rtol=1e-13, atol=0)
	for i in np.flatnonzero(c == 0):
		e = np.zeros(n)
		e[i] = noise
		assert np.array_equal(A[i], e)
	assert np.max(np.abs(A - S.dense_matrix(z, name, s, noise, c))) <= 1e-12 * np.max(np.abs(A))


def test_unit_scale_is_the_unscaled_host_model():
	X = R.points(65, 5, seed=1)
	W = R.probes(65, 4, seed=1)
	kw = dict(lengthscale=0.7, outputscale=2.0, noise=0.01)
	K0, K1 = KernelOperator(X, "matern52", **kw), KernelOperator(X, "matern52", diag_scale=np.ones(65), **kw)
	assert np.array_equal(K0._matmat(W), K1._matmat(W)) and np.array_equal(K0.rows([0, 64]), K1.rows([0, 64]))
	K1.set_diag_scale(np.full(65, 2.0))
	assert not np.array_equal(K0._matmat(W), K1._matmat(W))
	K1.set_diag_scale(None)
	assert K1.diag_scale is None and np.array_equal(K0._matmat(W), K1._matmat(W))
	## cross() and features() ignore the scale
	K1.set_diag_scale(np.full(65, 3.0))
	Xn = R.points(6, 5, seed=2)
	assert np.array_equal(K0.cross(Xn) @ W, K1.cross(Xn) @ W)
	om = np.random.default_rng(0).standard_normal((8, 5))
	assert np.array_equal(K0.features(frequencies=om).matrix(), K1.features(frequencies=om).matrix())


def test_the_bar_notices_a_missing_scale():
	"""One side of the scale dropped, or a scale entry off by one place, is orders of magnitude outside the bar."""
	n, d, ell = R.CPU_CASES[1]
	z = R.scaled_points(R.points(n, d), ell, np.float64)
	W = R.probes(n, 3)
	c = S.scale(n, 0, np.float64)
	Y, bar = S.model(z, "rbf", 1.0, 0.1, c, W)
	R.check_condition(Y, bar, np.float64)
	cl = c.astype(S.LD)
	rows_only = cl[:, None] * R.model(z, "rbf", 1.0, 0.0, W)[0] + S.LD(0.1) * W.astype(S.LD)
	assert float(np.max(np.abs(rows_only - Y) / np.where(bar == 0, 1, bar))) > 1e6
	shifted = S.model(z, "rbf", 1.0, 0.1, np.roll(c, 1), W)[0]
	assert float(np.max(np.abs(shifted - Y) / np.where(bar == 0, 1, bar))) > 1e6


def test_validation_messages():
	X = R.points(20, 2, seed=3)
	c = np.ones(20)
	for bad, val in ((-1.0, "-1.0"), (np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
		cb = c.copy()
		cb[7] = bad
		cb[11] = -2.0  # (the FIRST bad entry is named)
		with pytest.raises(ValueError, match=rf"diag_scale\[7\] = {re.escape(val)}"):
			KernelOperator(X, diag_scale=cb)
	with pytest.raises(ValueError, match=r"19 entries, the operator n = 20"):
		KernelOperator(X, diag_scale=np.ones(19))
	K = KernelOperator(X, diag_scale=c)
	with pytest.raises(ValueError, match=r"21 entries"):
		K.set_diag_scale(np.ones(21))
	assert np.array_equal(K.diag_scale, c)  # (a refused change changes nothing)
	## finite in float64, not in float32: refused for the fp32 operator only
	big = c.copy()
	big[2] = 1e300
	KernelOperator(X, diag_scale=big)
	with pytest.raises(ValueError, match=r"diag_scale\[2\]"):
		KernelOperator(X.astype(np.float32), diag_scale=big)
	## zeros are allowed, and the scale is rounded once to the dtype
	c32 = np.full(20, 0.1)
	c32[0] = 0.0
	K32 = KernelOperator(X.astype(np.float32), diag_scale=c32)
	assert K32.diag_scale.dtype == np.float32 and K32.diag_scale[0] == 0 and K32.diag_scale[1] == np.float32(0.1)


def test_every_python_refusal_comes_before_the_library(monkeypatch):
	"""Each entry that is not built for a scaled operator raises ValueError naming the entries that are, without creating a device
	operator: lanczos._as_device_operator and engine.DeviceOperator are replaced by a function that fails the test."""
	from primate_amd import autograd, engine, gp, grad, lanczos

	def touched(*a, **k):
		raise AssertionError("the library was touched before the refusal")

	monkeypatch.setattr(engine, "DeviceOperator", touched)
	monkeypatch.setattr(engine, "default_context", touched)
	monkeypatch.setattr(lanczos, "_as_device_operator", touched)
	monkeypatch.setattr(gp, "_as_device_operator", touched)
	n = 30
	X = R.points(n, 2, seed=5)
	y = np.sin(X[:, 0])
	K = KernelOperator(X, "rbf", lengthscale=0.5, noise=0.1, diag_scale=np.full(n, 0.5))
	names = "fixed_noise_posterior.*laplace"
	with pytest.raises(ValueError, match=names):
		K.preconditioned(10)
	M = MatrixFunction.__new__(MatrixFunction)  # (no device here: the refusal comes before anything is run)
	M._A, M.dtype, M.shape = K, np.dtype(np.float64), K.shape
	calls = {
		"grad.kernel_trace_grad": lambda: grad.kernel_trace_grad(M),
		"grad.kernel_quadratic_grad": lambda: grad.kernel_quadratic_grad(K, y),
		"grad.kernel_point_grad": lambda: grad.kernel_point_grad(K, y),
		"autograd.kernel_trace_fun(X=K)": lambda: autograd.kernel_trace_fun(K, "rbf", 0.5, 1.0, 0.1),
		"autograd.kernel_trace_fun(diag_scale=)": lambda: autograd.kernel_trace_fun(X, "rbf", 0.5, 1.0, 0.1, diag_scale=np.ones(n)),
		"gp.logdet": lambda: gp.logdet(K),
		"gp.logdet(rank=0)": lambda: gp.logdet(K, rank=0),
		"gp.logdet_grad": lambda: gp.logdet_grad(K),
		"gp.logdet_grad(rank=0)": lambda: gp.logdet_grad(K, rank=0),
		"gp.mll": lambda: gp.mll(K, y),
		"gp.posterior": lambda: gp.posterior(K, y, X[:3]),
		"gp.posterior_grad": lambda: gp.posterior_grad(K, y, X[:3]),
		"gp.sample_paths": lambda: gp.sample_paths(K, y),
		"gp.feature_posterior": lambda: gp.feature_posterior(K, y),
	}
	for who, call in calls.items():
		with pytest.raises(ValueError, match=names):
			call()
	## the new entries build the scaled operator themselves: they take the prior's operator, and say so
	for call in (lambda: gp.fixed_noise_posterior(K, y, 0.1, X[:3]), lambda: gp.laplace(K, np.sign(y), "logit")):
		with pytest.raises(ValueError, match="without a diagonal scale"):
			call()
	## ... and check their own arguments before the library, too
	K0 = KernelOperator(X, "rbf", lengthscale=0.5, noise=0.0)
	with pytest.raises(ValueError, match="point 4"):
		gp.fixed_noise_posterior(K0, y, np.where(np.arange(n) == 4, 0.0, 0.1), X[:3])
	with pytest.raises(ValueError, match="scalar or"):
		gp.fixed_noise_posterior(K0, y, np.ones(n + 1), X[:3])
	with pytest.raises(ValueError, match="unknown likelihood"):
		gp.laplace(K0, np.sign(y), "probit")
	with pytest.raises(ValueError, match="noise = 0"):
		gp.laplace(KernelOperator(X, noise=0.1), np.sign(y), "logit")
	with pytest.raises(ValueError, match="labels"):
		gp.laplace(K0, y, "logit")
	with pytest.raises(ValueError, match="non-negative integers"):
		gp.laplace(K0, y, "poisson")
	with pytest.raises(ValueError, match="fp64 only"):
		gp.laplace(KernelOperator(X.astype(np.float32)), np.sign(y), "logit")


def test_likelihoods_are_their_closed_forms():
	"""log p, its gradient and W of both likelihoods against central differences of log p."""
	from primate_amd.gp import laplace_likelihood

	rng = np.random.default_rng(2)
	f = rng.standard_normal(12) * 2
	for lik, t in (("logit", (rng.random(12) < 0.5).astype(float)), ("poisson", rng.poisson(3.0, 12).astype(float))):
		lp, g, W = laplace_likelihood(lik, t, f)
		assert np.all(W >= 0)
		h = 1e-5
		for i in range(12):
			e = np.zeros(12)
			e[i] = h
			lp1, g1, _ = laplace_likelihood(lik, t, f + e)
			lp0, g0, _ = laplace_likelihood(lik, t, f - e)
			assert abs((lp1 - lp0) / (2 * h) - g[i]) <= 1e-8 * max(1.0, abs(g[i]))
			assert abs(-(g1[i] - g0[i]) / (2 * h) - W[i]) <= 1e-8 * max(1.0, W[i])
	## a saturated logistic: W underflows to exactly 0, the gradient does not become nan
	lp, g, W = laplace_likelihood("logit", np.array([1.0, 0.0]), np.array([800.0, -800.0]))
	assert np.all(W == 0) and np.all(np.isfinite(g)) and np.isfinite(lp)


## the cases of tests/test_gpu_kernelscaled.py, checked here for their condition (no GPU needed for that)
def test_the_gpu_cases_discriminate():
	import test_gpu_kernelscaled as G

	for c in G.CASES:
		X, W, z, cs, Y, bar, K = G.case_data(c)
		R.check_condition(Y, bar, c[0])
