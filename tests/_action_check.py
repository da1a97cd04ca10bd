"""Helpers of the two-pass f(A)v tests (test_action_cpu.py, test_gpu_action.py): the coefficients of the action from a
Jacobi matrix, the derived elementwise bound between two summation orders of sum_t g_t W_t, and the test operators."""

import numpy as np
import scipy.sparse as sp


def random_spd_graph(n, avg_deg, seed, dtype=np.float64):
	"""Symmetric graph Laplacian + I of a G(n, p) graph: SPD, irregular row degrees, scattered neighbours."""
	rng = np.random.default_rng(seed)
	m = int(n * avg_deg / 2)
	i, j = rng.integers(0, n, m), rng.integers(0, n, m)
	keep = i != j
	W = sp.coo_matrix((rng.uniform(0.5, 2.0, keep.sum()), (i[keep], j[keep])), shape=(n, n))
	W = (W + W.T).tocsr()
	W.sum_duplicates()
	A = (sp.diags(np.asarray(W.sum(axis=1)).ravel() + 1.0) - W).tocsr().astype(dtype)
	A.sort_indices()
	return A


def dense_spd(n, seed, dtype=np.float64):
	rng = np.random.default_rng(seed)
	B = rng.standard_normal((n, n))
	A = B @ B.T / n + 0.5 * np.eye(n)
	return np.asfortranarray((A + A.T) / 2, dtype=dtype)


def action_coeffs(alpha, beta, deg, f):
	"""c = Y (f(theta) * Y[0, :]) of the deg x deg Jacobi matrix (alpha[:deg], beta[1:deg]), in fp64: f(A) x ~= ||x|| Q c."""
	a = np.asarray(alpha, dtype=np.float64)[:deg]
	b = np.asarray(beta, dtype=np.float64)[1:deg]
	th, Y = np.linalg.eigh(np.diag(a) + np.diag(b, 1) + np.diag(b, -1))
	return Y @ (f(th) * Y[0, :])


def order_bound(Q, c, xnorm, terms, eps):
	"""terms * eps * sum_t |g_t| |W_t[row]| with g_t W_t = xnorm c_t q_t (Q: normalised columns), evaluated in fp64: what two
	summation orders of the same `terms` terms, each partial sum rounded once, can differ by elementwise."""
	return terms * eps * xnorm * (np.abs(np.asarray(Q, dtype=np.float64)) @ np.abs(c))


def ordered_sum(Q, g, dtype, reverse):
	"""sum_t g_t Q[:, t] accumulated in `dtype`, t ascending or descending (NumPy: product and sum each rounded)."""
	Qd, gd = np.asarray(Q, dtype=dtype), np.asarray(g, dtype=dtype)
	y = np.zeros(Qd.shape[0], dtype=dtype)
	order = range(Qd.shape[1] - 1, -1, -1) if reverse else range(Qd.shape[1])
	for t in order:
		y = (y + (gd[t] * Qd[:, t]).astype(dtype)).astype(dtype)
	return y
