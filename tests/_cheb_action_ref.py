"""NumPy restatement of the Chebyshev action Y = sum_k c_k T_k(A~) Z, A~ = (A - c) / h: the yardstick of the action tests.

`action_recurrence` is the DIRECT recurrence w_0 = z, w_1 = A~ z, w_{k+1} = 2 A~ w_k - w_{k-1} with Y += c_k w_k after every
step, carried in `dtype` (matrix, vectors, coefficients). np.longdouble is the yardstick (SciPy's CSR product and NumPy's
dense product both run in it); the fp64 and fp32 runs give the restatement's own deviation, which the bar is made of.
`action_eig` is the exact U f(L) U^T Z of the 5-point grid Laplacian through its sine basis."""

import numpy as np

from _cheb_ref import center_halfwidth


def action_recurrence(A, Z, coef, bounds, dtype=np.float64):
	"""Y (n, P) in `dtype` for the columns of Z and the coefficients c_0 .. c_deg. A: anything with `astype` and `@` on (n, P)
	arrays. coef may be a list of coefficient vectors (of any lengths): the list of their Y, from ONE pass over the w_k - every
	Y takes the operations, in the order, of a call of its own."""
	dt = np.dtype(dtype).type
	c, h = center_halfwidth(bounds)
	A = A.astype(dt) if hasattr(A, "astype") else A
	Z = np.asarray(Z, dtype=dt)
	many = isinstance(coef, (list, tuple))
	coefs = [np.asarray(cf, dtype=np.float64).astype(dt) for cf in (coef if many else [coef])]
	inv_h, c_h = dt(1.0 / h), dt(c / h)  # (the device's scalars: formed in fp64, rounded to the dtype)

	def at(W):  # A~ W, in the order the device forms it: (1/h) (A W) - (c/h) W
		return (inv_h * np.asarray(A @ W, dtype=dt) - c_h * W).astype(dt, copy=False)

	Ys = [(cf[0] * Z).astype(dt, copy=False) for cf in coefs]
	wp, wc = None, Z
	for k in range(1, max(cf.size for cf in coefs)):
		w = at(Z) if k == 1 else (dt(2.0) * at(wc) - wp).astype(dt, copy=False)
		wp, wc = wc, w
		for i, cf in enumerate(coefs):
			if k < cf.size:
				Ys[i] = (Ys[i] + cf[k] * w).astype(dt, copy=False)
	return Ys if many else Ys[0]


def action_recurrence_ld(A, Z, coef, bounds, chunk=32, workers=8):
	"""action_recurrence in np.longdouble over chunks of `chunk` columns in threads: NumPy has no BLAS for long double (its loops
	release the GIL), and the recurrence treats every column on its own - the same bits as one call, several times sooner."""
	from concurrent.futures import ThreadPoolExecutor

	Ald = A.astype(np.longdouble) if hasattr(A, "astype") else A
	Z = np.asarray(Z)
	many = isinstance(coef, (list, tuple))
	coefs = list(coef) if many else [coef]
	cols = [slice(i, min(i + chunk, Z.shape[1])) for i in range(0, Z.shape[1], chunk)]
	with ThreadPoolExecutor(max_workers=workers) as ex:
		parts = list(ex.map(lambda c: action_recurrence(Ald, Z[:, c], coefs, bounds, np.longdouble), cols))
	Ys = [np.concatenate([p[i] for p in parts], axis=1) for i in range(len(coefs))]
	return Ys if many else Ys[0]


def col_norms(X):
	X = np.asarray(X)
	return np.sqrt(np.sum(X.astype(np.longdouble) ** 2, axis=0)).astype(np.float64)


def coefficient_weight(coef):
	"""sum_k (k + 1) |c_k|: the growth of one rounding per step through the recurrence (|T_k| <= 1, |T_k'| <= k^2 is not needed:
	w_k carries k + 1 roundings of size eps ||z||)."""
	coef = np.abs(np.asarray(coef, dtype=np.float64))
	return float(np.sum((np.arange(coef.size) + 1.0) * coef))


def action_bar(Y_ld, Y_F, Z, coef, eps):
	"""Per column: max(8 D_i, B_i) with D_i = ||Y_F - Y_ld||_2 the deviation of the restatement carried in the operator's dtype
	from the long-double yardstick (the 8 is for the device's other summation order, as _cheb_ref.rounding_bar's) and
	B_i = eps sum_k (k + 1) |c_k| ||z_i||_2. Returns (bar, D, B)."""
	D = col_norms(np.asarray(Y_F, dtype=np.longdouble) - Y_ld)
	B = float(eps) * coefficient_weight(coef) * col_norms(Z)
	return np.maximum(8.0 * D, B), D, B


def action_eig(m1, m2, Z, f):
	"""U f(lam) U^T Z of grid_laplacian(m1, m2) through the orthonormal DST-I along both grid axes (its own inverse): exact at any size."""
	from scipy.fft import dstn

	l1 = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, m1 + 1) / (m1 + 1))
	l2 = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, m2 + 1) / (m2 + 1))
	lam = l1[:, None] + l2[None, :]
	Z = np.asarray(Z, dtype=np.float64)
	C = dstn(Z.reshape(m1, m2, -1), type=1, norm="ortho", axes=(0, 1))
	return dstn(C * f(lam)[:, :, None], type=1, norm="ortho", axes=(0, 1)).reshape(m1 * m2, -1)


def jackson_step_coefficients(deg, bounds, cut):
	"""c_0 .. c_deg of the Jackson-damped step 1[x <= cut] on `bounds` (a spectral projector's polynomial): the step's exact
	Chebyshev coefficients (theta_c = arccos x~_cut: c_0 = 1 - theta_c / pi, c_k = -2 sin(k theta_c) / (k pi)) times the Jackson factors."""
	from primate_amd.chebyshev import damping_factors

	c, h = center_halfwidth(bounds)
	th = np.arccos(np.clip((cut - c) / h, -1.0, 1.0))
	k = np.arange(1, deg + 1, dtype=np.float64)
	coef = np.concatenate([[1.0 - th / np.pi], -2.0 * np.sin(k * th) / (k * np.pi)])
	return coef * damping_factors("jackson", deg + 1)
