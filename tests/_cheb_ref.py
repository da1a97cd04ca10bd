"""NumPy restatement of the Chebyshev moments mu_k = z^T T_k(A~) z, A~ = (A - c) / h: the yardstick of the Chebyshev tests.

`moments_recurrence` is the DIRECT recurrence w_0 = z, w_1 = A~ z, w_{k+1} = 2 A~ w_k - w_{k-1}, mu_k = z . w_k - one product
per moment, no doubling identity, so that it shares no algebra with the device's mu_{2j+2} = 2 ||w_{j+1}||^2 - mu_0. Carried in
`dtype` (vectors, coefficients and dots), fp64 by default. `moments_eig` is the exact form sum_i (u_i . z)^2 cos(k arccos l~_i)."""

import math

import numpy as np


def center_halfwidth(bounds):
	a, b = float(bounds[0]), float(bounds[1])
	return 0.5 * (a + b), 0.5 * (b - a)


def moments_recurrence(A, Z, nmom, bounds, dtype=np.float64):
	"""mu[i, k] for the columns z_i of Z and k = 0 .. nmom - 1. A: anything with `@` on (n, P) arrays."""
	dt = np.dtype(dtype).type
	c, h = center_halfwidth(bounds)
	A = A.astype(dt) if hasattr(A, "astype") else A
	Z = np.asarray(Z, dtype=dt)
	inv_h, c_h = dt(1.0 / h), dt(c / h)

	def at(W):  # A~ W, in the order the device forms it: (1/h) (A W) - (c/h) W
		return (inv_h * np.asarray(A @ W, dtype=dt) - c_h * W).astype(dt, copy=False)

	def dot(X, Y):
		# column dots. fp64 (the yardstick): the fp64 products summed exactly (math.fsum) and rounded once, so that the yardstick's
		# own summation error - a few ulp of mu_0 for any fp64 summation order over n terms, the whole budget (k + 1) eps mu_0 of the
		# first moments - does not enter. Other dtypes (the restatement the bar is made of): summed in dt along a contiguous axis,
		# NumPy's pairwise sum
		prod = np.ascontiguousarray((X * Y).T)
		if dt is np.float64:
			return np.array([math.fsum(col) for col in prod])
		return np.sum(prod, axis=1, dtype=dt)

	mu = np.zeros((Z.shape[1], nmom), dtype=dt)
	wp, wc = Z, None
	for k in range(nmom):
		if k == 0:
			w = Z
		elif k == 1:
			w = at(Z)
		else:
			w = (dt(2.0) * at(wc) - wp).astype(dt, copy=False)
			wp = wc
		wc = w
		mu[:, k] = dot(Z, w)
	return mu.astype(np.float64)


def moments_eig(lam, UtZ, nmom, bounds):
	"""Exact moments from the eigenvalues `lam` (n) and the coefficients UtZ = U^T Z (n, P) of the probes in the eigenbasis."""
	c, h = center_halfwidth(bounds)
	th = np.arccos(np.clip((np.asarray(lam, dtype=np.float64) - c) / h, -1.0, 1.0))
	w2 = np.asarray(UtZ, dtype=np.float64) ** 2  # (n, P)
	k = np.arange(nmom, dtype=np.float64)
	return (np.cos(np.outer(k, th)) @ w2).T  # (P, nmom)


def grid_laplacian(m1, m2, dtype=np.float64):
	"""5-point Dirichlet Laplacian of an m1 x m2 grid, point (i1, i2) at row i1 * m2 + i2."""
	import scipy.sparse as sp

	def T(m):
		return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))

	A = (sp.kron(sp.identity(m1), T(m2)) + sp.kron(T(m1), sp.identity(m2))).tocsr().astype(dtype)
	A.sort_indices()
	return A


def grid_laplacian_eig(m1, m2, Z):
	"""(lam, U^T Z) of grid_laplacian(m1, m2) from its sine basis (an orthonormal DST-I along both grid axes): exact at any size."""
	from scipy.fft import dstn

	l1 = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, m1 + 1) / (m1 + 1))
	l2 = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, m2 + 1) / (m2 + 1))
	lam = (l1[:, None] + l2[None, :]).ravel()
	Z = np.asarray(Z, dtype=np.float64)
	C = dstn(Z.reshape(m1, m2, -1), type=1, norm="ortho", axes=(0, 1))
	return lam, C.reshape(m1 * m2, -1)


def rounding_bar(mu64, muF, eps):
	"""The allowed deviation (P, nmom) of a device run in a dtype of unit roundoff `eps` from the fp64 yardstick mu64: 8x the
	deviation of the restatement carried in that dtype (muF), maximised over k per probe - the 8 is for the device's other
	summation order over blocks and waves -, never below (k + 1) eps mu_0."""
	dev = np.max(np.abs(muF - mu64), axis=1, keepdims=True)
	k = np.arange(mu64.shape[1], dtype=np.float64)[None, :]
	return np.maximum(8.0 * dev, (k + 1.0) * eps * np.abs(mu64[:, :1]))
