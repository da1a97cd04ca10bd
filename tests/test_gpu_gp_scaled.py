"""gp.fixed_noise_posterior and gp.laplace on the diagonally scaled kernel operator, each result against dense NumPy
on the matrix of the same rounded points (tests/_kernelop_ref.py: dense_matrix).

The cases: n = 300 points in [0, 1]^2, lengthscale 0.3, outputscale 1, rbf and matern32. For fixed per-point noise log-uniform in
[1e-2, 1] the scaled operator D K0 D + I has condition 2.1e3 .. 2.4e3 here (asserted <= 5e3), where full-reorthogonalised Lanczos
reaches 1e-13 at 100 steps: the bars are 1e-9 relative, those of gp.posterior's own tests at that conditioning. For the Laplace fits
B = I + W^{1/2} K0 W^{1/2} has condition <= 28 (W <= 1/4 for the logistic). Each item prints its figures before it asserts."""

import numpy as np
import pytest

import _kernelop_ref as R

pytestmark = pytest.mark.gpu

N, D, M, ELL, S0 = 300, 2, 40, 0.3, 1.0
PROFILES = ("rbf", "matern32")
_cache = {}


def case(name, n=N):
	"""Points, new points, the dense K0, K(X*, X), a latent sample and the operator of the prior: computed once, read-only."""
	key = (name, n)
	if key not in _cache:
		from primate_amd.operators import KernelOperator

		X = R.points(n, D, seed=11)
		Xn = R.points(M, D, seed=13)
		K = KernelOperator(X, name, lengthscale=ELL, outputscale=S0, noise=0.0)
		K0 = R.dense_matrix(R.scaled_points(X, ELL, np.float64), name, S0, 0.0)
		Cm = K.cross(Xn) @ np.eye(n)
		lam, U = np.linalg.eigh(K0)
		f_true = (U * np.sqrt(np.maximum(lam, 0.0))) @ np.random.default_rng(17).standard_normal(n)
		for Z in (X, Xn, K0, Cm, f_true):
			Z.setflags(write=False)
		_cache[key] = (X, Xn, K, K0, Cm, f_true)
	return _cache[key]


## ---- fixed per-point noise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROFILES)
def test_fixed_noise_posterior_against_the_dense_solve(name):
	from primate_amd import gp

	X, Xn, K, K0, Cm, f_true = case(name)
	rng = np.random.default_rng(12)
	nv = np.exp(rng.uniform(np.log(1e-2), np.log(1.0), N))
	y = f_true + np.sqrt(nv) * rng.standard_normal(N)
	c = 1.0 / np.sqrt(nv)
	cond = float(np.linalg.cond(c[:, None] * K0 * c[None, :] + np.eye(N)))
	assert cond <= 5e3, f"cond(D K0 D + I) = {cond:.3e}"
	A = K0 + np.diag(nv)
	want_mean = Cm @ np.linalg.solve(A, y)
	want_var = S0 - np.einsum("ij,ji->i", Cm, np.linalg.solve(A, Cm.T))
	mean, var, info = gp.fixed_noise_posterior(K, y, nv, Xn, deg=100)
	e_mean = float(np.max(np.abs(mean - want_mean)) / np.max(np.abs(want_mean)))
	e_var = float(np.max(np.abs(var - want_var)) / S0)
	print(f"[gp-scaled] fixed noise {name}: cond {cond:.3e} mean err {e_mean:.2e} var err {e_var:.2e} steps {info['steps']}")
	assert K.diag_scale is None and K.noise == 0.0  # (K is not mutated)
	assert e_mean <= 1e-9 and e_var <= 1e-9
	assert info["zero_columns"] == [] and info["batches"] == 1


def test_fixed_noise_constant_equals_posterior():
	"""noise_var constant: the same posterior as gp.posterior on K with that noise, within the bar both are held to - through two
	different operators (sigma2 I beside K0, and D K0 D + I)."""
	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	name = "matern32"
	X, Xn, K, K0, Cm, f_true = case(name)
	v = 0.05
	y = f_true + np.sqrt(v) * np.random.default_rng(14).standard_normal(N)
	mean, var, _ = gp.fixed_noise_posterior(K, y, v, Xn, deg=100)
	Kv = KernelOperator(X, name, lengthscale=ELL, outputscale=S0, noise=v)
	mean2, var2, _ = gp.posterior(Kv, y, Xn, deg=100)
	## ... and K.noise takes part: e = K.noise + noise_var
	mean3, var3, _ = gp.fixed_noise_posterior(KernelOperator(X, name, lengthscale=ELL, outputscale=S0, noise=0.02), y, np.full(N, 0.03), Xn, deg=100)
	e = [float(np.max(np.abs(a - mean2)) / np.max(np.abs(mean2))) for a in (mean, mean3)] + [float(np.max(np.abs(a - var2)) / S0) for a in (var, var3)]
	print(f"[gp-scaled] constant noise against posterior: mean {e[0]:.2e} {e[1]:.2e} var {e[2]:.2e} {e[3]:.2e}")
	assert max(e) <= 1e-9


## ---- Laplace ----------------------------------------------------------------------------------------------------------------
def dense_newton(K0, t, lik, tol=1e-13, max_iter=100):
	"""Plain Newton on Psi(f) = log p(y|f) - f^T K0^-1 f / 2 in the stable form of Rasmussen & Williams, Algorithm 3.1, dense."""
	from primate_amd.gp import laplace_likelihood

	n = K0.shape[0]
	f = np.zeros(n)
	a = np.zeros(n)
	for it in range(1, max_iter + 1):
		lp, g, W = laplace_likelihood(lik, t, f)
		sw = np.sqrt(W)
		B = np.eye(n) + sw[:, None] * K0 * sw[None, :]
		b = W * f + g
		a = b - sw * np.linalg.solve(B, sw * (K0 @ b))
		f_new = K0 @ a
		done = np.max(np.abs(f_new - f)) <= tol * max(1.0, np.max(np.abs(f_new)))
		f = f_new
		if done:
			break
	lp, g, W = laplace_likelihood(lik, t, f)
	return f, a, W, g, lp - 0.5 * float(a @ f), it


def dense_predict(K0, Cm, W, g):
	sw = np.sqrt(W)
	B = np.eye(K0.shape[0]) + sw[:, None] * K0 * sw[None, :]
	Ct = sw[:, None] * Cm.T
	return Cm @ g, S0 - np.einsum("ji,ji->i", Ct, np.linalg.solve(B, Ct)), B


def laplace_case(name, lik, n=N):
	key = ("laplace", name, lik, n)
	if key not in _cache:
		from primate_amd import gp

		X, Xn, K, K0, Cm, f_true = case(name, n)
		rng = np.random.default_rng(19)
		if lik == "logit":
			y = np.where(rng.random(n) < 1.0 / (1.0 + np.exp(-2.0 * f_true)), 1.0, -1.0)
			t = 0.5 * (y + 1.0)
		else:
			y = t = rng.poisson(np.exp(0.5 * f_true + 0.5)).astype(np.float64)
		ref = dense_newton(K0, t, lik)
		post = gp.laplace(K, y, lik)
		_cache[key] = (post, ref, K0, Cm, Xn)
	return _cache[key]


@pytest.mark.parametrize("name,lik,n", [("rbf", "logit", N), ("matern32", "logit", N), ("matern32", "poisson", 257)])
def test_laplace_against_dense_newton(name, lik, n):
	from scipy.special import expit

	post, (f, a, W, g, psi, it_ref), K0, Cm, Xn = laplace_case(name, lik, n)
	fmax = float(np.max(np.abs(f)))
	e_f = float(np.max(np.abs(post.f_hat - f)) / fmax)
	mean_ref, var_ref, B = dense_predict(K0, Cm, W, g)
	out = post.predict(Xn)
	mean, var = out[0], out[1]
	e_mean = float(np.max(np.abs(mean - mean_ref)) / np.max(np.abs(mean_ref)))
	e_var = float(np.max(np.abs(var - var_ref)) / S0)
	print(f"[gp-scaled] laplace {lik} {name} n={n}: iterations {post.iterations} (dense {it_ref}) cond(B) {np.linalg.cond(B):.1f} "
		  f"f_hat err {e_f:.2e} objective {post.objective:.6f} (dense {psi:.6f}) mean err {e_mean:.2e} var err {e_var:.2e} halvings {post.info['halvings']}")  # fmt: skip
	assert post.converged and post.iterations <= 15
	assert e_f <= 1e-9
	assert np.max(np.abs(post.W - W)) <= 1e-9 * np.max(W) and np.max(np.abs(post.a - a)) <= 1e-8 * np.max(np.abs(a))
	assert abs(post.objective - psi) <= 1e-9 * abs(psi)
	assert e_mean <= 1e-9 and e_var <= 1e-9
	if lik == "logit":
		prob_ref = expit(mean_ref / np.sqrt(1.0 + np.pi * var_ref / 8.0))
		assert len(out) == 3 and float(np.max(np.abs(out[2] - prob_ref))) <= 1e-8
	else:
		assert len(out) == 2


def test_laplace_log_marginal():
	"""Deterministic part: with the probes given, every per-probe quadrature v^T log(B) v is within 1e-8 relative of the dense
	eigendecomposition's. Statistical part: seed fixed, count = 256: |value - exact| <= 4 reported standard errors."""
	post, (f, a, W, g, psi, it_ref), K0, Cm, Xn = laplace_case("rbf", "logit")
	sw = np.sqrt(post.W)
	B = np.eye(N) + sw[:, None] * K0 * sw[None, :]
	lam, U = np.linalg.eigh(B)
	V = np.where(np.random.default_rng(23).random((N, 16)) < 0.5, -1.0, 1.0)
	want = np.einsum("ic,i,ic->c", U.T @ V, np.log(lam), U.T @ V)
	value, se = post.log_marginal(deg=30, probes=V)
	e_q = float(np.max(np.abs(post.quadratures / want - 1.0)))
	assert value == pytest.approx(post.objective - 0.5 * float(np.mean(post.quadratures)), rel=1e-14)
	exact = post.objective - 0.5 * float(np.sum(np.log(lam)))
	value2, se2 = post.log_marginal(count=256, deg=30, seed=5)
	print(f"[gp-scaled] log marginal: per-probe quadrature err {e_q:.2e}; value {value2:.4f} exact {exact:.4f} ({abs(value2 - exact) / se2:.2f} standard errors of {se2:.4f})")
	assert e_q <= 1e-8
	assert post.quadratures.shape == (256,) and se2 > 0 and abs(value2 - exact) <= 4.0 * se2
	assert post.log_marginal(count=256, deg=30, seed=5) == (value2, se2)


def test_laplace_saturated_point():
	"""A logit fit in which one W_i underflows to exactly 0 - c_i = 0, row i of B is e_i^T - still predicts, and matches the dense
	reference, at that row too. The mode of a smooth prior cannot saturate a logistic by itself (|f| would have to pass 700), so the fit
	is taken to its mode first and then one f is FORCED: the posterior object is given f_hat with f_i = 800, as the issue sets the case."""
	from primate_amd import gp

	name = "rbf"
	X, Xn, K, K0, Cm, f_true = case(name)
	post, ref, *_ = laplace_case(name, "logit")
	i = 7
	f = post.f_hat.copy()
	f[i] = 800.0 if post._t[i] == 1.0 else -800.0
	lp, g, W = gp.laplace_likelihood("logit", post._t, f)
	assert W[i] == 0.0
	Ks = gp._scaled_operator(K, np.sqrt(W), 1.0)
	from primate_amd import engine

	forced = gp.LaplacePosterior(K, "logit", post._t, engine.DeviceOperator(Ks), f, post.a, W, g, 0, True, 0.0, 40, -1, dict())
	try:
		## the product at the saturated row: exactly the row of the identity
		Y = forced._op.matmat(np.eye(N))
		assert np.array_equal(Y[i], np.eye(N)[i]) and np.array_equal(Y[:, i], np.eye(N)[i])
		mean, var, prob = forced.predict(Xn)
		mean_ref, var_ref, B = dense_predict(K0, Cm, W, g)
		e_mean = float(np.max(np.abs(mean - mean_ref)) / np.max(np.abs(mean_ref)))
		e_var = float(np.max(np.abs(var - var_ref)) / S0)
		V = np.where(np.random.default_rng(29).random((N, 8)) < 0.5, -1.0, 1.0)
		forced.log_marginal(deg=30, probes=V)
		lam, U = np.linalg.eigh(B)
		want = np.einsum("ic,i,ic->c", U.T @ V, np.log(lam), U.T @ V)
		e_q = float(np.max(np.abs(forced.quadratures / want - 1.0)))
		print(f"[gp-scaled] saturated point {i}: W_i {W[i]} mean err {e_mean:.2e} var err {e_var:.2e} quadrature err {e_q:.2e}")
		assert e_mean <= 1e-9 and e_var <= 1e-9 and e_q <= 1e-8
	finally:
		forced.close()


def test_handles_close():
	from primate_amd import gp

	X, Xn, K, K0, Cm, f_true = case("rbf")
	y = np.where(f_true > 0, 1.0, 0.0)  # (labels in {0, 1})
	with gp.laplace(K, y, "logit", max_iter=2) as post:
		assert post.iterations == 2 and not post.converged and post._op is not None
	assert post._op is None
	with pytest.raises(ValueError, match="closed"):
		post.predict(Xn)
	post.close()
