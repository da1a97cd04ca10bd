"""Hyperparameter gradients of the kernel operator on the device: the raw accumulator against the long-double model
of `_kernelgrad_ref`, elementwise within its forward bar, at every case of the issue (one tile and less, a remainder tile, several row
blocks and slabs, the d > 16 instantiation, a full 64-column chunk and one column more, duplicate points under matern12, an offset
of 1e4); accumulation, reset, run-to-run bits, a parameter change; the driver `kernel_trace_grad` on explicit probes against the model
on the factors it used; the exact identity; the quadratic form; the torch function; the accumulator's hold on its operator."""

import gc

import numpy as np
import pytest

import _kernelgrad_ref as G
import _kernelop_ref as R
from primate_amd.operators import KernelOperator, MatrixFunction

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def _device(eng, X, name, ls, s, noise):
	K = KernelOperator(X, name, lengthscale=ls, outputscale=s, noise=noise)
	return K, eng.DeviceOperator(K)


def _matrices(eng, op, Z, W):
	n, m = Z.shape
	Zd, Wd = eng.DeviceMatrix(n, m, ctx=op.ctx), eng.DeviceMatrix(n, m, ctx=op.ctx)
	Zd.set(0, Z)
	Wd.set(0, W)
	return Zd, Wd


def _one_update(eng, op, Z, W, alpha=1.0):
	Zd, Wd = _matrices(eng, op, Z, W)
	acc = eng.KernelGradAccumulator(op)
	acc.update(Zd, 0, Wd, 0, Z.shape[1], alpha=alpha, beta=0.0)
	vals, cnt = acc.get()
	for x in (acc, Zd, Wd):
		x.close()
	return vals, cnt


@pytest.mark.parametrize("case", G.GPU_CASES, ids=[G.case_id(c) for c in G.GPU_CASES])
def test_accumulator_against_the_model(eng, case):
	(X, ls, s, noise, Z, W), z, g, bar = G.case_model(case)
	ratio = G.check_condition(g, bar)
	K, op = _device(eng, X, case[3], ls, s, noise)
	assert np.array_equal(K.scaled_points(), z)
	vals, cnt = _one_update(eng, op, Z, W)
	op.close()
	w = G.worst(vals, g, bar)
	print(f"{G.case_id(case)}: bar / max |g| = {ratio:.2e}, worst |got - model| / bar = {w:.4f}")
	assert cnt == case[2] and vals.shape == (case[1] + 2,) and np.all(np.isfinite(vals))
	assert w <= 1.0, (case, vals, g.astype(np.float64))


def test_two_updates_equal_one_of_the_concatenated_columns(eng):
	case = (257, 8, 65, "rbf", False, 0.0, False)
	(X, ls, s, noise, Z, W), z, g, bar = G.case_model(case)
	cut = 30
	g1, bar1 = G.model(z, "rbf", ls, s, Z[:, :cut], W[:, :cut])
	g2, bar2 = G.model(z, "rbf", ls, s, Z[:, cut:], W[:, cut:])
	K, op = _device(eng, X, "rbf", ls, s, noise)
	Zd, Wd = _matrices(eng, op, Z, W)
	acc = eng.KernelGradAccumulator(op)
	acc.update(Zd, 0, Wd, 0, 65, beta=0.0)
	one, _ = acc.get()
	acc.update(Zd, 0, Wd, 0, cut, beta=0.0)
	acc.update(Zd, cut, Wd, cut, 65 - cut, beta=1.0)
	two, cnt = acc.get()
	assert cnt == 65 + 65
	w_model, w_one = G.worst(two, g1 + g2, bar1 + bar2), G.worst(two, one.astype(G.LD), bar + bar1 + bar2)
	print(f"two updates: / (bar1 + bar2) against the model {w_model:.4f}; against one update / (bar + bar1 + bar2) {w_one:.4f}")
	assert w_model <= 1.0 and w_one <= 1.0
	## alpha and beta: 2 vals - 0.5 (the last 35 columns)
	acc.update(Zd, cut, Wd, cut, 65 - cut, alpha=-0.5, beta=2.0)
	three, _ = acc.get()
	assert G.worst(three, 2 * (g1 + g2) - 0.5 * g2, 2 * (bar1 + bar2) + 0.5 * bar2 + 4 * G.EPS * np.abs(2 * (g1 + g2))) <= 1.0
	## reset: zeros and a count of 0; the next update gives the bits of the first
	acc.reset()
	vals, cnt = acc.get()
	assert cnt == 0 and np.array_equal(vals, np.zeros(10))
	acc.update(Zd, 0, Wd, 0, 65, beta=1.0)
	again, cnt = acc.get()
	assert cnt == 65 and np.array_equal(again, one), "two runs must give identical bits"
	## refused updates leave the values alone
	for args in ((Zd, 0, Wd, 0, 0), (Zd, 60, Wd, 0, 6), (Zd, 0, Wd, -1, 4), (Zd, 0, Wd, 0, 66)):
		with pytest.raises(Exception, match="columns|m = 0"):
			acc.update(*args)
	short = eng.DeviceMatrix(256, 4, ctx=op.ctx)
	with pytest.raises(Exception, match="257 points"):
		acc.update(short, 0, Wd, 0, 4)
	with pytest.raises(Exception, match="finite"):
		acc.update(Zd, 0, Wd, 0, 4, alpha=np.nan)
	assert np.array_equal(acc.get()[0], one)
	for x in (short, acc, Zd, Wd, op):
		x.close()


def test_identical_bits_over_several_slabs_and_a_parameter_change(eng):
	n, d, m = 1000, 3, 8
	X = R.points(n, d, seed=9)
	rng = np.random.default_rng(9)
	Z, W = rng.standard_normal((n, m)), rng.standard_normal((n, m))
	K, op = _device(eng, X, "matern52", 0.4, 1.0, 0.0)
	a, _ = _one_update(eng, op, Z, W)
	b, _ = _one_update(eng, op, Z, W)
	assert np.array_equal(a, b), "two runs must give identical bits"
	## set_parameters, then update: the next update sees the new operator - the bits of a fresh one
	acc = eng.KernelGradAccumulator(op)
	Zd, Wd = _matrices(eng, op, Z, W)
	acc.update(Zd, 0, Wd, 0, m, beta=0.0)
	K.set_parameters(lengthscale=[0.3, 0.5, 0.7], outputscale=2.5, noise=0.2)
	acc.update(Zd, 0, Wd, 0, m, beta=0.0)
	changed, _ = acc.get()
	K2, op2 = _device(eng, X, "matern52", [0.3, 0.5, 0.7], 2.5, 0.2)
	fresh, _ = _one_update(eng, op2, Z, W)
	assert np.array_equal(changed, fresh) and not np.array_equal(changed, a)
	for x in (acc, Zd, Wd, op, op2):
		x.close()


def test_create_refuses_other_operators(eng):
	import ctypes as C

	import scipy.sparse as sp

	from primate_amd import _capi

	A = eng.DeviceOperator(sp.identity(40, format="csr"))
	h = C.c_void_p()
	assert _capi.lib().slq_kernel_grad_create(A.ctx._h, A._h, C.byref(h)) == _capi.SLQ_EINVAL
	assert b"kind 'csr'" in _capi.lib().slq_last_error()
	A.close()
	K32 = KernelOperator(R.points(40, 2, dtype=np.float32), "rbf")
	op = eng.DeviceOperator(K32)
	assert _capi.lib().slq_kernel_grad_create(op.ctx._h, op._h, C.byref(h)) == _capi.SLQ_EINVAL
	assert b"fp32" in _capi.lib().slq_last_error()
	op.close()


def test_the_accumulator_outlives_a_del_of_the_python_operator(eng):
	case = (17, 4, 4, "matern32", True, 0.0, False)
	(X, ls, s, noise, Z, W), z, g, bar = G.case_model(case)
	K, op = _device(eng, X, "matern32", ls, s, noise)
	acc = eng.KernelGradAccumulator(op)
	Zd, Wd = _matrices(eng, op, Z, W)
	del op, K
	gc.collect()
	acc.update(Zd, 0, Wd, 0, 4, beta=0.0)
	vals, _ = acc.get()
	assert G.worst(vals, g, bar) <= 1.0
	for x in (acc, Zd, Wd):
		x.close()


## ---- the drivers ---------------------------------------------------------------------------------------------------------------------
def _driver_inputs():
	n, d, count = 200, 2, 24
	X = R.points(n, d, seed=4)
	V = np.asfortranarray(np.sign(np.random.default_rng(4).standard_normal((n, count))))
	return n, d, count, X, V


@pytest.mark.parametrize("ls", [0.35, [0.3, 0.5]], ids=["scalar", "perdim"])
def test_driver_against_the_model_on_its_own_factors(eng, ls):
	from primate_amd.grad import kernel_trace_grad

	n, d, count, X, V = _driver_inputs()
	K = KernelOperator(X, "matern32", lengthscale=ls, outputscale=1.2, noise=0.1)
	M = MatrixFunction(K, "log", deg=20, orth=20)
	est, grads, info = kernel_trace_grad(M, probes=V, count=count, batch=16)
	assert info["count"] == count and info["acc_count"] == count and info["quad"].shape == (count,)
	## Z through the existing action, in the driver's batches (a full one and a partial one)
	Mi = MatrixFunction(K, "inv", deg=20, orth=20)
	Zh = np.hstack([Mi @ V[:, :16], Mi @ V[:, 16:]])
	z = R.scaled_points(X, ls, np.float64)
	g, bar = G.model(z, "matern32", ls, 1.2, Zh / count, V)
	ratio = G.check_condition(g, bar)
	got = np.concatenate([grads["lengthscale"], [grads["outputscale"], grads["noise"]]])
	if np.size(ls) > 1:
		want, wbar = g, bar
	else:  # (a scalar lengthscale: the sum over the dimensions, taken on the host)
		assert grads["lengthscale"].shape == (1,)
		want, wbar = np.concatenate([[g[:d].sum()], g[d:]]), np.concatenate([[bar[:d].sum() + d * G.EPS * np.abs(g[:d]).sum()], bar[d:]])
	w = G.worst(got, want, wbar)
	print(f"driver: bar / max |g| = {ratio:.2e}, worst |got - model| / bar = {w:.4f}; est {est:.12e}")
	assert w <= 1.0, (got, want.astype(np.float64))
	## est: the quadrature of the same runs - a kept-basis plan per batch on the same probes
	quad = []
	for c0, m in ((0, 16), (16, 8)):
		plan = eng.LanczosPlan(M._op, m, 20, 20, basis="keep")
		plan.set_probes(np.asfortranarray(V[:, c0 : c0 + m]))
		plan.run(M._rtol)
		quad.append(plan.quadrature("log"))
		plan.close()
	assert np.array_equal(info["quad"], np.concatenate(quad)) and est == float(np.mean(info["quad"]))


def test_chebyshev_route_against_the_model_on_its_own_factors(eng):
	"""A ChebyshevFunction goes through `_chebyshev_batch`: Z = p'(A) V with the coefficients of 1 / x on M's bounds - the action an
	"inv" ChebyshevFunction of the same degree and bounds computes, fetched on the host in the driver's batches."""
	from primate_amd.chebyshev import ChebyshevFunction
	from primate_amd.grad import kernel_trace_grad

	n, d, count, X, V = _driver_inputs()
	ls = [0.3, 0.5]
	K = KernelOperator(X, "rbf", lengthscale=ls, outputscale=1.2, noise=0.1)
	bounds = (0.05, 1.2 * n + 1.0)  # (sigma2 <= lambda(A) <= s n + sigma2)
	M = ChebyshevFunction(K, "log", deg=40, bounds=bounds)
	est, grads, info = kernel_trace_grad(M, probes=V, count=count, batch=16)
	assert info["acc_count"] == count and est == float(np.mean(info["quad"])) and np.all(np.isfinite(info["quad"]))
	Mi = ChebyshevFunction(K, "inv", deg=40, bounds=bounds)
	Zh = np.hstack([Mi @ V[:, :16], Mi @ V[:, 16:]])
	g, bar = G.model(R.scaled_points(X, ls, np.float64), "rbf", ls, 1.2, Zh / count, V)
	ratio = G.check_condition(g, bar)
	w = G.worst(np.concatenate([grads["lengthscale"], [grads["outputscale"], grads["noise"]]]), g, bar)
	print(f"chebyshev driver: bar / max |g| = {ratio:.2e}, worst |got - model| / bar = {w:.4f}")
	assert w <= 1.0
	for x in (M, Mi):
		x.close()
	with pytest.raises(ValueError, match="device:sphere"):
		kernel_trace_grad(ChebyshevFunction(K, "log", deg=10, bounds=bounds), pdf="device:sphere", count=8)


def test_identity_is_exact_and_launches_nothing(eng, monkeypatch):
	from primate_amd.grad import kernel_trace_grad

	n, d, count, X, V = _driver_inputs()
	K = KernelOperator(X, "rbf", lengthscale=[0.3, 0.5], outputscale=1.5, noise=0.25)
	M = MatrixFunction(K, "identity", deg=20)

	def refuse(*a, **k):
		raise AssertionError("identity must not touch the device")

	monkeypatch.setattr(eng, "KernelGradAccumulator", refuse)
	monkeypatch.setattr(eng, "DeviceMatrix", refuse)
	monkeypatch.setattr(M, "_plan", refuse)
	est, grads, info = kernel_trace_grad(M, count=8, batch=8, seed=1)
	assert est == n * 1.75 and np.array_equal(grads["lengthscale"], [0.0, 0.0]) and grads["outputscale"] == n and grads["noise"] == n
	assert info["acc_count"] == 0


def test_quadratic_grad_against_the_model(eng):
	from primate_amd.grad import kernel_quadratic_grad

	case = (257, 3, 16, "matern12", False, 1e4, True)
	(X, ls, s, noise, Z, W), z, g, bar = G.case_model(case)
	K = KernelOperator(X, "matern12", lengthscale=ls, outputscale=s, noise=noise)
	grads = kernel_quadratic_grad(K, Z, W)
	got = np.array([grads["lengthscale"][0], grads["outputscale"], grads["noise"]])
	want, wbar = np.concatenate([[g[:3].sum()], g[3:]]), np.concatenate([[bar[:3].sum() + 3 * G.EPS * np.abs(g[:3]).sum()], bar[3:]])
	assert G.worst(got, want, wbar) <= 1.0
	## V = None: U on both sides, one vector
	u = Z[:, 0].copy()
	g1, bar1 = G.model(z, "matern12", ls, s, u, u)
	grads = kernel_quadratic_grad(K, u)
	got = np.array([grads["lengthscale"][0], grads["outputscale"], grads["noise"]])
	want, wbar = np.concatenate([[g1[:3].sum()], g1[3:]]), np.concatenate([[bar1[:3].sum() + 3 * G.EPS * np.abs(g1[:3]).sum()], bar1[3:]])
	assert G.worst(got, want, wbar) <= 1.0


@pytest.mark.parametrize("per_dim", [False, True], ids=["scalar", "perdim"])
def test_torch_backward_leaves_the_drivers_numbers(eng, per_dim):
	import torch

	from primate_amd.autograd import kernel_trace_fun
	from primate_amd.grad import kernel_trace_grad

	n, d, count, X, V = _driver_inputs()
	ls0 = [0.3, 0.5] if per_dim else 0.35

	def params():
		return (torch.tensor(ls0, dtype=torch.float64, requires_grad=True), torch.tensor(1.2, dtype=torch.float64, requires_grad=True),
				torch.tensor(0.1, dtype=torch.float64, requires_grad=True))  # fmt: skip

	K = KernelOperator(X, "matern52", lengthscale=ls0, outputscale=1.2, noise=0.1)
	est, grads, _ = kernel_trace_grad(MatrixFunction(K, "log", deg=20), pdf="device:rademacher", count=48, batch=32, seed=5)
	ls, s, v = params()
	loss = kernel_trace_fun(X, "matern52", ls, s, v, "log", deg=20, count=48, seed=5, batch=32)
	assert loss.ndim == 0 and float(loss.detach()) == est
	loss.backward()
	assert ls.grad.shape == ls.shape and np.array_equal(np.atleast_1d(ls.grad.numpy()), grads["lengthscale"])
	assert float(s.grad) == grads["outputscale"] and float(v.grad) == grads["noise"]
	ls, s, v = params()
	(3 * kernel_trace_fun(X, "matern52", ls, s, v, "log", deg=20, count=48, seed=5, batch=32)).backward()
	assert np.array_equal(np.atleast_1d(ls.grad.numpy()), 3.0 * grads["lengthscale"])
	assert float(s.grad) == 3.0 * grads["outputscale"] and float(v.grad) == 3.0 * grads["noise"]
