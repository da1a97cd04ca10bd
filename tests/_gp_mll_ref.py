"""The model of the marginal-likelihood tests and its bars.

Notation of §4.18: A = K0 + sigma2 I on the ROUNDED z of the operator, P = L L^T + sigma2 I for a given factor L (the device's, or the
host model's), M = P^{-1/2}, B = M A M. D_theta = dA/dtheta as §4.16 has it (`_kernelgrad_ref`): D_lk = (s / l_k) chi(r2) (z_ik - z_jk)^2,
D_s = phi(r2), D_sigma2 = I; tr D = 0, n, n.

The dense model: `dense_D` builds the d + 2 matrices in long double, `trace_inv` contracts them with a long-double inverse
(`inv_ld`: 50-digit arithmetic up to n = 64, beyond it numpy's float64 `inv` refined by two Newton-Schulz steps X <- X (2 I - P X)
in long double: the float64 inverse alone carries eps cond(P) / sigma2 per entry, which is the size of the bar), so that tr(A^-1 D) and tr(P^-1 D) are known far inside every bar here.

The bar of the exact part. The code under test evaluates

    g = sigma^-2 [tr D - sum_ij C_ij D_ij],        C = (L H) L^T,  H = (L^T L + sigma2 I)^-1,

by gradient updates with Z = L H and W = L in chunks of 64 columns. The sum is what §4.16's accumulator computes for the pair (Z, W),
and its forward bound `_kernelgrad_ref.model(...)[1]` covers it for ANY chunking (the chunk sums are more partial sums of the same
terms: the bound's S = (2 n + 64) eps admits them). tr D is an integer below 2^53: exact. What is left is the scale by
alpha / sigma2 (one rounding of the sum, inside the 2 eps |g| of §4.16's bar), the chunk accumulations and the last addition of
n / sigma2, each a rounding of a partial value bounded by |tr D| / sigma2 + |sum| / sigma2 <= 2 |tr D| / sigma2 for the outputscale
and the noise (0 <= sum <= tr D there up to the bar: C and D_s are positive semi-definite) - at most ceil(r / 64) + 3 <= (n + r) / 2
of them. Hence

    bar_theta = sigma^-2 bar16_theta(Z = L H, W = L) + (n + r) eps sigma^-2 |tr D_theta|,        eps = 2^-53,

a forward bound on the arithmetic given H. (The error of H itself - Jacobi's V is orthogonal to r eps, not exactly - is NOT in the
bar: the tests hold the code to the bar against tr(P^-1 D) of the dense inverse, so an inaccurate H fails them.)
Each case asserts first that the bar is at most 1e-6 max |g| per group: passing a wider one would say nothing.
"""

import numpy as np

import _kernelgrad_ref as G
import _kernelop_ref as R

LD = np.longdouble
EPS = LD(2.0) ** -53

## (n, d, profile, lengthscale, s, sigma2, rank_max, note)
CASES = (
	(1, 1, "rbf", 1.0, 1.0, 1e-2, 1, ""),
	(40, 3, "matern12", 0.5, 2.0, 1e-3, 37, "rpad>rank"),
	(400, 3, "matern32", (0.3, 0.45, 0.6), 1.0, 1e-4, 64, "perdim"),
	(40, 17, "matern52", 2.0, 1.5, 1e-2, 37, ""),
	(40, 1, "rbf", 0.4, 0.5, 1e-6, 64, "early-stop"),
)
EARLY_STOP = CASES[4]


def case_id(c) -> str:
	return f"n{c[0]}-d{c[1]}-{c[2]}-r{c[6]}" + (f"-{c[7]}" if c[7] else "")


def case_points(c) -> np.ndarray:
	return R.points(c[0], c[1], seed=c[0] + c[1]).copy()


def operator(c):
	from primate_amd.operators import KernelOperator

	n, d, name, ell, s, sigma2, rank, _ = c
	return KernelOperator(case_points(c), name, lengthscale=np.asarray(ell, dtype=np.float64) if isinstance(ell, tuple) else ell, outputscale=s, noise=sigma2)


def dense_D(z: np.ndarray, name: str, ls, s: float) -> np.ndarray:
	"""(d + 2, n, n) long double: dA/dtheta for the d lengthscales, the outputscale and the noise, on the rounded points z."""
	n, d = z.shape
	ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (d,)).astype(LD)
	zl = z.astype(LD)
	r2 = R.r2_exact(z)
	ch = G.chi(name, r2)
	out = np.zeros((d + 2, n, n), dtype=LD)
	for k in range(d):
		D = zl[:, k][:, None] - zl[None, :, k]
		out[k] = LD(s) / ls[k] * ch * D * D
	out[d] = R.phi(name, r2)
	out[d + 1] = np.eye(n, dtype=LD)
	return out


def inv_ld(Pm: np.ndarray) -> np.ndarray:
	"""The inverse of a symmetric positive definite matrix, rounded to long double. Up to n = 64 in 50-digit arithmetic (mpmath, which
	comes with torch's sympy): at sigma2 = 1e-6 cond(P) is 4e7, and the bar of the noise component is 100 eps of the value - a long-double
	inverse (eps_ld cond = 2e-12) is not a reference for it. Beyond: float64 inv, then two Newton-Schulz steps in long double
	(cond <= 4e6 in these cases: eps_ld cond is a hundredth of the tightest bar)."""
	n = Pm.shape[0]
	Pl = Pm.astype(LD)
	if n <= 64:
		import mpmath

		with mpmath.workdps(50):
			hi = Pl.astype(np.float64)
			lo = (Pl - hi.astype(LD)).astype(np.float64)  # (hi + lo is the long double exactly)
			X = (mpmath.matrix(hi.tolist()) + mpmath.matrix(lo.tolist())) ** -1
			out = np.empty((n, n), dtype=LD)
			for i in range(n):
				for j in range(n):
					h = float(X[i, j])
					out[i, j] = LD(h) + LD(float(X[i, j] - mpmath.mpf(h)))
		return LD(0.5) * (out + out.T)
	X = np.linalg.inv(Pm.astype(np.float64)).astype(LD)
	two = LD(2) * np.eye(n, dtype=LD)
	for _ in range(2):
		X = X @ (two - Pl @ X)
	return LD(0.5) * (X + X.T)


def trace_inv(Xinv: np.ndarray, D: np.ndarray) -> np.ndarray:
	"""tr(Xinv D_theta) for every theta, in Xinv's precision."""
	return np.array([np.sum(Xinv * Dk) for Dk in D], dtype=Xinv.dtype)


def dense_a(z: np.ndarray, name: str, s: float, sigma2: float) -> np.ndarray:
	"""A = s phi(r2) + sigma2 I in long double."""
	A = LD(s) * R.phi(name, R.r2_exact(z))
	A[np.diag_indices(z.shape[0])] += LD(sigma2)
	return A


def dense_p(L: np.ndarray, sigma2: float) -> np.ndarray:
	Ll = L.astype(LD)
	Pm = Ll @ Ll.T
	Pm[np.diag_indices(L.shape[0])] += LD(sigma2)
	return Pm


def exact_model(c, L: np.ndarray, H: np.ndarray):
	"""(g, bar, trD): tr(P^-1 D_theta) of the dense inverse for the factor L, and the bar of the module docstring with Z = L H."""
	n, d, name, ell, s, sigma2, rank, _ = c
	z = R.scaled_points(case_points(c), np.asarray(ell, dtype=np.float64), np.float64)
	D = dense_D(z, name, ell, s)
	g = trace_inv(inv_ld(dense_p(L, sigma2)), D)
	_, bar16 = G.model(z, name, ell, s, L @ H, L)
	trD = np.array([0.0] * d + [float(n), float(n)], dtype=LD)
	r = L.shape[1]
	bar = bar16 / LD(sigma2) + LD(n + r) * EPS * trD / LD(sigma2)
	return g, bar, trD


def minv_dense(L: np.ndarray, sigma2: float):
	"""(M = P^{-1/2}, cond P) by eigh in float64."""
	lam, U = np.linalg.eigh(dense_p(L, sigma2).astype(np.float64))
	return (U / np.sqrt(lam)) @ U.T, float(lam[-1] / lam[0])


def estimator_terms(A64: np.ndarray, Minv: np.ndarray, D64: np.ndarray, Wp: np.ndarray, on: bool, Binv_action=None):
	"""(per-probe values (count x (d + 2)), U, Vm) of the estimator on the explicit probes Wp (n x count):
	(M (B^-1 [- I]) w)^T D_theta (M w), B^-1 w exact (solve) or by `Binv_action(B, W)`."""
	Bd = Minv @ A64 @ Minv
	Bd = 0.5 * (Bd + Bd.T)
	T = np.linalg.solve(Bd, Wp) if Binv_action is None else Binv_action(Bd, Wp)
	if on:
		T = T - Wp
	U, Vm = Minv @ T, Minv @ Wp
	vals = np.array([np.einsum("ic,ic->c", U, Dk @ Vm) for Dk in D64]).T
	return vals, U, Vm


def rademacher(n: int, count: int, seed: int) -> np.ndarray:
	rng = np.random.default_rng(seed)
	return np.asfortranarray(np.floor(rng.random((n, count)) * 2) * 2 - 1)


## ---- the fingerprint of `posterior` (scripts/op_fingerprint.py --posterior; profiles/gp_mll_posterior_fingerprint.txt) -----------
def posterior_fingerprint_lines() -> list:
	"""sha256 of posterior's mean and variance on one seeded case, without and with the preconditioner: the lines a library must
	reproduce bit for bit (n = 300, matern52, d = 3, sigma2 = 1e-3, two columns of y, one of them zero, 37 new points)."""
	import hashlib

	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	rng = np.random.default_rng(719)
	X = rng.random((300, 3))
	y = np.zeros((300, 2))
	y[:, 0] = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(300)
	Xnew = rng.random((37, 3))
	K = KernelOperator(X, "matern52", lengthscale=0.4, outputscale=1.2, noise=1e-3)
	lines = []
	for rank, deg in ((0, 60), (100, 20)):
		mean, var, info = gp.posterior(K, y, Xnew, deg=deg, precond_rank=rank)
		h = hashlib.sha256()
		for x in (mean, var):
			h.update(np.ascontiguousarray(x, dtype=np.float64).tobytes())
		lines.append(f"posterior matern52 n=300 d=3 m=37 precond_rank={rank} deg={deg} sum={float(np.sum(mean) + np.sum(var)):.12e} sha={h.hexdigest()[:16]}")
	return lines
