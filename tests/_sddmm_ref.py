"""NumPy model of the sampled dense-dense product on a CSR pattern (slq_sddmm_update): the yardstick of tests/test_gpu_sddmm.py,
validated on the CPU by tests/test_sddmm_cpu.py.

    vals[e] = beta * old[e] + alpha * sum_{j < m} W[row(e), j] * Z[col(e), j]        (symmetric: the summand is
              0.5 * (W[r, j] Z[c, j] + Z[r, j] W[c, j]))

`vals_ld` carries it in np.longdouble. `bar` is the standard dot-product bound gamma_T ~ T u on T terms (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1), u = 2^-53, with two more roundings for the scale and the add and a factor 2 of
slack:  bar[e] = 2 (T + 2) u (|alpha| sum_j |W_rj| |Z_cj| + |beta| |old_e|),  T = m, or 2 m when symmetric (there the
magnitude sum is the symmetric one, 0.5 (|W_r| |Z_c| + |Z_r| |W_c|))."""

import numpy as np

U = 2.0**-53


def pattern_rows_cols(pattern):
	"""(rows, cols) of the stored entries of a SciPy CSR matrix, in storage order."""
	indptr, indices = np.asarray(pattern.indptr), np.asarray(pattern.indices)
	return np.repeat(np.arange(indptr.size - 1), np.diff(indptr)), indices.astype(np.int64)


def _products(W, Z, rows, cols, symmetric, dtype):
	W, Z = np.asarray(W, dtype=dtype), np.asarray(Z, dtype=dtype)
	s = np.sum(W[rows, :] * Z[cols, :], axis=1)
	if symmetric:
		s = dtype(0.5) * (s + np.sum(Z[rows, :] * W[cols, :], axis=1))
	return s


def vals_ld(rows, cols, W, Z, alpha=1.0, beta=1.0, old=None, symmetric=False):
	"""The update in np.longdouble. W, Z: (n, m) arrays (the m columns the update reads). old: the values before (None: zeros)."""
	ld = np.longdouble
	old = np.zeros(len(rows), dtype=ld) if old is None else np.asarray(old, dtype=ld)
	out = ld(alpha) * _products(W, Z, rows, cols, symmetric, ld)
	return out if beta == 0.0 else ld(beta) * old + out


def bar(rows, cols, W, Z, alpha=1.0, beta=1.0, old=None, symmetric=False):
	"""The rounding bar of one update, per stored entry (float64)."""
	m = np.asarray(W).shape[1]
	T = 2 * m if symmetric else m
	mag = _products(np.abs(W), np.abs(Z), rows, cols, symmetric, np.longdouble)
	old = np.zeros(len(rows)) if old is None else np.abs(np.asarray(old, dtype=np.longdouble))
	return np.asarray(2.0 * (T + 2) * U * (abs(alpha) * mag + abs(beta) * old), dtype=np.float64)


## ---- the patterns of the tests --------------------------------------------------------------------------------------
def grid_pattern():
	"""The 13 x 11 grid Laplacian: n = 143 (not a multiple of 64), 3 to 5 entries per row."""
	from _cheb_ref import grid_laplacian

	return grid_laplacian(13, 11)


def random_pattern(n=300, seed=7):
	"""A 300-row random symmetric pattern (about 6 entries per row) with one empty row (and column) and one full row (and column):
	a row longer than any chunk and than the long-row threshold, an empty row, nnz no multiple of 64. Values: all ones."""
	import scipy.sparse as sp

	rng = np.random.default_rng(seed)
	k = 3 * n
	i, j = rng.integers(0, n, k), rng.integers(0, n, k)
	D = np.zeros((n, n), dtype=bool)
	D[i, j] = True
	D |= D.T
	full, empty = 77, 130
	D[full, :] = D[:, full] = True
	D[empty, :] = D[:, empty] = False
	P = sp.csr_matrix(D.astype(np.float64))
	P.sort_indices()
	assert P.indptr[empty + 1] == P.indptr[empty] and P.indptr[full + 1] - P.indptr[full] == n - 1
	if P.nnz % 64 == 0:  # (drop one symmetric pair: the count must not be a multiple of the wave)
		raise AssertionError("choose another seed: nnz is a multiple of 64")
	return P


def empty_pattern(n=70):
	import scipy.sparse as sp

	return sp.csr_matrix((n, n), dtype=np.float64)
