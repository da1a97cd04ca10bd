"""Independent constructions of the Gauss and Gauss-Radau rules of a Jacobi matrix, for tests/test_gpu_resume.py and
tests/test_resume_cpu.py: NumPy (`numpy.linalg.solve` + `eigh` of the bordered matrix) and 50 digits (mpmath).

alpha: the m diagonal entries; beta: m + 1 entries, beta[0] unused, beta[i] couples i - 1 and i, beta[m] couples the
border (the norm of the Lanczos residual after m steps)."""

import numpy as np


def jacobi(alpha, beta, m):
	T = np.diag(np.asarray(alpha[:m], dtype=np.float64))
	for i in range(1, m):
		T[i, i - 1] = T[i - 1, i] = beta[i]
	return T


def gauss_np(alpha, beta, m):
	w, Z = np.linalg.eigh(jacobi(alpha, beta, m))
	return w, Z[0] ** 2


def radau_np(alpha, beta, m, a):
	"""(nodes, weights) of the (m + 1)-point rule with a node at a: (J_m - a I) delta = beta_m^2 e_m, border a + delta_m."""
	T = jacobi(alpha, beta, m)
	rhs = np.zeros(m)
	rhs[-1] = beta[m] ** 2
	delta = np.linalg.solve(T - a * np.eye(m), rhs)
	B = np.zeros((m + 1, m + 1))
	B[:m, :m] = T
	B[m, m] = a + delta[-1]
	B[m, m - 1] = B[m - 1, m] = beta[m]
	w, Z = np.linalg.eigh(B)
	return w, Z[0] ** 2


def radau_mp(alpha, beta, m, a, dps: int = 50):
	"""The same rule in `dps` digits (the fp64 entries taken as exact), returned rounded to fp64."""
	import mpmath as mp

	with mp.workdps(dps):
		T = mp.zeros(m, m)
		for i in range(m):
			T[i, i] = mp.mpf(float(alpha[i]))
		for i in range(1, m):
			T[i, i - 1] = T[i - 1, i] = mp.mpf(float(beta[i]))
		bm = mp.mpf(float(beta[m]))
		rhs = mp.zeros(m, 1)
		rhs[m - 1] = bm * bm
		delta = mp.lu_solve(T - mp.mpf(float(a)) * mp.eye(m), rhs)
		B = mp.zeros(m + 1, m + 1)
		for i in range(m):
			for j in range(m):
				B[i, j] = T[i, j]
		B[m, m] = mp.mpf(float(a)) + delta[m - 1]
		B[m, m - 1] = B[m - 1, m] = bm
		E, Q = mp.eigsy(B)
		nodes = np.array([float(E[i]) for i in range(m + 1)])
		weights = np.array([float(Q[0, i] ** 2) for i in range(m + 1)])
	o = np.argsort(nodes)
	return nodes[o], weights[o]


def rule_distance(r1, r2):
	"""Largest absolute difference of nodes and of weights between two rules of the same size."""
	return max(float(np.max(np.abs(r1[0] - r2[0]))), float(np.max(np.abs(r1[1] - r2[1]))))


def stage_statistics(gauss, radau=None):
	"""What the adaptive driver reads per stage, from per-probe values: (S, width) = (sum gauss, sum |radau - gauss|)."""
	S = float(np.sum(gauss))
	return S, (float(np.sum(np.abs(radau - gauss))) if radau is not None else 0.0)


def expected_stop(stages, S, width, deg_rtol, endpoint: bool):
	"""The stage the documented rule stops at (the last one if none meets it)."""
	for k, m in enumerate(stages):
		if endpoint and width[k] <= deg_rtol * abs(S[k]):
			return m
		if not endpoint and k >= 1 and abs(S[k] - S[k - 1]) <= deg_rtol * abs(S[k]):
			return m
	return stages[-1]
