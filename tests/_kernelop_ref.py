"""The model of the kernel operator's tests and its bar.

The model takes z ROUNDED TO THE OPERATOR'S DTYPE (the operator is defined on these z), forms r2_ij = sum_k (z_ik - z_jk)^2 in long
double - no cancellation - applies the profile and computes Y = A W in long double.

The bar per output element is a forward bound on an evaluation by norms plus dot product in the operator's dtype, not a fitted number:

    dr2_ij = (d + 3) eps (|z_i|^2 + |z_j|^2 + 2 |z_i| |z_j|)                       eps = unit roundoff of the dtype
    dK_ij  = s |phi(max(r2 - dr2, 0)) - phi(r2 + dr2)| + C_EXP eps K_ij,   dK_ii = C_EXP eps K_ii
    bar_ic = sum_j dK_ij |W_jc| + (n + 2) eps sum_j K_ij |W_jc| + 2 eps sigma2 |W_ic|

dr2: the two norms carry d roundings each, the dot product d, the two additions and the product by 2 three more, every one
relative to a partial sum bounded by (|z_i| + |z_j|)^2. dK: phi is monotone in r2, so the change of phi over [r2 - dr2, r2 + dr2] bounds
what the error of r2 does; C_EXP eps K is the profile's own arithmetic (sqrt, the polynomial, the rounding of exp's argument, exp
itself). (n + 2) eps: the n-term sum of the second product, the product by s and the last fma. C_EXP = 4 as the issue sets it.
"""

import numpy as np

LD = np.longdouble
PROFILES = ("rbf", "matern12", "matern32", "matern52")
C_EXP = 4.0
## the issue's CPU cases: (n, d, lengthscale), points uniform in [0, 1]^d
CPU_CASES = ((257, 1, 0.3), (257, 3, 0.5), (257, 8, 1.0), (130, 17, 1.5))


def eps_of(dtype) -> float:
	return float(np.finfo(np.dtype(dtype)).eps) / 2.0


def points(n: int, d: int, seed: int = 0, offset: float = 0.0, dtype=np.float64) -> np.ndarray:
	return (np.random.default_rng(1000 + seed).random((n, d)) + offset).astype(dtype)


def probes(n: int, p: int, seed: int = 0, dtype=np.float64) -> np.ndarray:
	return np.asfortranarray(np.random.default_rng(2000 + seed).standard_normal((n, p)).astype(dtype))


def scaled_points(X: np.ndarray, lengthscale, dtype) -> np.ndarray:
	"""z as the operator defines it: the mean per dimension is the float64 sum in row order over n, (x - mean) / l is float64
	arithmetic, and the result is rounded once to `dtype`."""
	X = np.asarray(X, dtype=dtype)
	X = X.reshape(-1, 1) if X.ndim == 1 else X
	mean = np.cumsum(X, axis=0, dtype=np.float64)[-1] / np.float64(X.shape[0])
	ls = np.broadcast_to(np.asarray(lengthscale, dtype=np.float64), (X.shape[1],))
	return ((X.astype(np.float64) - mean) / ls).astype(dtype)


def phi(name: str, r2):
	"""The profile on an array of r2 (any float type; long double stays long double)."""
	r2 = np.asarray(r2)
	T = r2.dtype.type
	if name == "rbf":
		return np.exp(-r2 / T(2))
	r = np.sqrt(r2)
	if name == "matern12":
		return np.exp(-r)
	if name == "matern32":
		a = np.sqrt(T(3)) * r
		return (T(1) + a) * np.exp(-a)
	if name == "matern52":
		a = np.sqrt(T(5)) * r
		return (T(1) + a + T(5) * r2 / T(3)) * np.exp(-a)
	raise ValueError(name)


def r2_exact(z: np.ndarray, rows=None) -> np.ndarray:
	"""sum_k (z_ik - z_jk)^2 in long double for the rows `rows` (default all) against every point."""
	zl = z.astype(LD)
	zi = zl if rows is None else zl[np.asarray(rows)]
	out = np.zeros((zi.shape[0], zl.shape[0]), dtype=LD)
	for k in range(zl.shape[1]):
		diff = zi[:, k][:, None] - zl[:, k][None, :]
		out += diff * diff
	return out


def model(z: np.ndarray, name: str, s: float, noise: float, W: np.ndarray, rows=None):
	"""(Y, bar) in long double for the output rows `rows` (default all): Y = (s phi(r2) + noise I) W on the rounded z, and the
	forward bound of the module docstring for an evaluation in z's dtype."""
	n, d = z.shape
	idx = np.arange(n) if rows is None else np.asarray(rows)
	eps = LD(eps_of(z.dtype))
	r2 = r2_exact(z, idx)
	K = LD(s) * phi(name, r2)
	Wl, Wa = W.astype(LD), np.abs(W.astype(LD))
	Y = K @ Wl + LD(noise) * Wl[idx]
	nrm = np.sqrt(np.sum(z.astype(LD) ** 2, axis=1))
	dr2 = LD(d + 3) * eps * (nrm[idx][:, None] + nrm[None, :]) ** 2
	dK = LD(s) * np.abs(phi(name, np.maximum(r2 - dr2, LD(0))) - phi(name, r2 + dr2)) + LD(C_EXP) * eps * K
	dK[np.arange(idx.size), idx] = LD(C_EXP) * eps * K[np.arange(idx.size), idx]
	bar = dK @ Wa + LD(n + 2) * eps * (K @ Wa) + LD(2) * eps * LD(noise) * Wa[idx]
	return Y, bar


def dense_matrix(z: np.ndarray, name: str, s: float, noise: float) -> np.ndarray:
	"""A in float64 from the long-double model (for the oracle and numpy.linalg)."""
	A = (LD(s) * phi(name, r2_exact(z))).astype(np.float64)
	A[np.diag_indices_from(A)] += noise
	return A


def emulate(z: np.ndarray, name: str, s: float, noise: float, W: np.ndarray) -> np.ndarray:
	"""The norms-plus-dot evaluation entirely in z's dtype (NumPy): what a device kernel computes up to summation order."""
	T = z.dtype.type
	nrm = np.sum(z * z, axis=1, dtype=z.dtype)
	r2 = np.maximum(nrm[:, None] + nrm[None, :] - T(2) * (z @ z.T), T(0))
	np.fill_diagonal(r2, T(0))
	K = T(s) * phi(name, r2).astype(z.dtype)
	return (K @ W.astype(z.dtype) + T(noise) * W.astype(z.dtype)).astype(z.dtype)


def check_condition(Y, bar, dtype) -> float:
	"""The bar must stay a small fraction of the result, or passing it says nothing: max bar / max |Y| <= 1e-3 (fp32), 1e-10 (fp64)."""
	ratio = float(np.max(bar) / np.max(np.abs(Y)))
	limit = 1e-3 if np.dtype(dtype) == np.float32 else 1e-10
	assert ratio <= limit, f"the bar is {ratio:.3e} of max |Y| (limit {limit:g}): the case does not discriminate"
	return ratio


def worst(got: np.ndarray, Y, bar) -> float:
	"""max |got - Y| / bar."""
	return float(np.max(np.abs(got.astype(LD) - Y) / bar))
