"""The model of the diagonally scaled kernel operator's tests and its bar, on top of tests/_kernelop_ref.py (which
it changes nothing in).

With c ROUNDED TO THE OPERATOR'S DTYPE (the operator is defined on the rounded c, as on the rounded z) and
(Y0, bar0) = R.model(z, name, s, 0, c[:, None] * W) in long double - the unscaled, noise-free operator applied to diag(c) W -

    Y_i   = c_i Y0_i + sigma2 W_i
    bar_i = c_i (bar0_i + 2 eps sum_j K_ij c_j |W_j|) + 2 eps sigma2 |W_i|

bar0 already bounds the evaluation of sum_j K_ij (c_j W_j) by norms plus dot product in the dtype; the 2 eps term covers the two
roundings the scale adds per term: K_ij c_j before the second product, and c_i beside s in the epilogue. The noise term is the last
fma's, as in the unscaled model.
"""

import numpy as np

import _kernelop_ref as R

LD = np.longdouble


def scale(n: int, seed: int, dtype, zeros: bool = True) -> np.ndarray:
	"""c log-uniform in [0.1, 10], rounded to `dtype`, with two entries exactly 0 where n >= 15 (a saturated likelihood)."""
	rng = np.random.default_rng(3000 + seed)
	c = np.exp(rng.uniform(np.log(0.1), np.log(10.0), n))
	if zeros and n >= 15:
		c[[3, n - 2]] = 0.0
	return c.astype(dtype)


def model(z: np.ndarray, name: str, s: float, noise: float, c: np.ndarray, W: np.ndarray, rows=None):
	"""(Y, bar) in long double for the output rows `rows` (default all) of A = s diag(c) phi(r2) diag(c) + noise I on the rounded z and c."""
	assert c.dtype == z.dtype
	n = z.shape[0]
	idx = np.arange(n) if rows is None else np.asarray(rows)
	eps = LD(R.eps_of(z.dtype))
	cl = c.astype(LD)
	Wl = W.astype(LD)
	cW = cl[:, None] * Wl
	Y0, bar0 = R.model(z, name, s, 0.0, cW, rows=rows)
	K = LD(s) * R.phi(name, R.r2_exact(z, idx))
	Y = cl[idx][:, None] * Y0 + LD(noise) * Wl[idx]
	bar = cl[idx][:, None] * (bar0 + LD(2) * eps * (K @ np.abs(cW))) + LD(2) * eps * LD(noise) * np.abs(Wl[idx])
	return Y, bar


def dense_matrix(z: np.ndarray, name: str, s: float, noise: float, c: np.ndarray) -> np.ndarray:
	"""A in float64 from the long-double model."""
	cl = c.astype(LD)
	A = (cl[:, None] * (LD(s) * R.phi(name, R.r2_exact(z))) * cl[None, :]).astype(np.float64)
	A[np.diag_indices_from(A)] += noise
	return A


def worst(got: np.ndarray, Y, bar) -> float:
	"""max |got - Y| / bar; where the bar is exactly 0 (a row with c_i = 0 and no noise: the result is exactly 0) the two must be equal."""
	err = np.abs(got.astype(LD) - Y)
	zero = bar == 0
	assert np.all(err[zero] == 0), "an element whose bar is exactly 0 is not exact"
	return float(np.max(np.where(zero, LD(0), err / np.where(zero, LD(1), bar)))) if err.size else 0.0
