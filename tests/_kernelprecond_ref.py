"""The model of the pivoted-Cholesky preconditioner's tests and its bars.

K0 = s phi(r2) comes from tests/_kernelop_ref.py: long double on the rounded z, with its elementwise forward bound dK0 for an
evaluation by norms plus dot product in float64 (the bound of §4.15 without the product: dr2, the change of phi over
[r2 - dr2, r2 + dr2], C_EXP eps K; C_EXP eps K alone on the diagonal, where r2 is 0 exactly). One refinement, which asks MORE of
the code: a pair of bitwise-equal rounded points (the duplicates case) also has dr2 = 0. The factor's column kernel accumulates
z_p . z_i by the same in-order fma chain that produced |z_i|^2, so for z_i == z_p the dot product IS the norm, bit for bit, and
fma(-2, g, 2 g) is exactly 0; the emulation below sums in the same order for the same reason. Without it matern12, whose phi has
a square-root cusp at 0, would carry sqrt(dr2) ~ 6e-8 s on those pairs and no bar of 1e-9 s could hold on the issue's own case.

A factor (L, pivots) - the device's, or the NumPy emulation of the definition in float64 - is checked against it with forward
bounds, eps the unit roundoff of float64, r = rank_max:

  interpolation  |(L L^T)[p, i] - K0[p, i]| <= dK0[p, i] + (r + 8) eps sum_j |L_ij| |L_pj| + FLAT          at every pivot p
  residual       s - sum_j L_ij^2 >= -(dK0[i, i] + (r + 8) eps sum_j L_ij^2 + FLAT)                          at every row i
  greedy         at every step k the residual diagonal d of the long-double factor rebuilt from the pivots 0 .. k-1 has
                 d[p_k] >= max d - 2 max_i (dK0[i, i] + (r + 8) eps sum_{j<k} L_ij^2 + FLAT)
  FLAT = 4 (r + 2) eps s

dK0: the kernel evaluation. (r + 8) eps sum |L||L|: the k-term inner product of a step, the subtraction, the division by the root
and the root itself, as in the standard analysis of a Cholesky column. FLAT: the factor divides by the root of the RUNNING residual
d_p, which k updates d <- max(0, d - L^2) have rounded, each by eps times a partial value bounded by s, while the numerator of the
pivot's own entry is s - sum_j L_pj^2 summed afresh (k + 2 more roundings bounded by s); the two differ by at most 2 (k + 2) eps s,
so L_pk sqrt(d_p) = d_p + e with |e| <= 2 (k + 2) eps s, and column k of L L^T carries r_ip e / d_p with |r_ip| <= sqrt(d_i d_p) <=
d_p (the pivot holds the largest residual): at most |e| in absolute terms, however close d_p is to the early-stop threshold 64 eps s
- there it is NOT small relative to d_p, which is why the term is flat. The same difference, once per row, separates the running
residual the device compares from the freshly summed one (residual, greedy); doubled for safety. In the greedy check both the
pivot's row and the row of the maximum carry a bar, hence the factor 2.

Each case asserts first that every bar is at most 1e-9 s: passing a wider one would say nothing.
"""

import numpy as np

import _kernelop_ref as R

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps) / 2.0

## the issue's case table: (n, d, profile, lengthscale, s, sigma2, rank_max, note)
CASES = (
	(1, 1, "rbf", 1.0, 1.0, 1e-2, 1, ""),
	(17, 3, "rbf", 0.5, 2.0, 1e-3, 5, ""),
	(130, 2, "matern32", 0.3, 1.0, 1e-4, 16, ""),
	(300, 1, "rbf", 1.0, 1.0, 1e-6, 64, "early-stop"),
	(257, 17, "matern52", 2.0, 1.5, 1e-2, 33, "rpad>rank"),
	(200, 3, "matern12", 0.5, 1.0, 1e-3, 48, "duplicates"),
	(1000, 2, "rbf", 0.2, 1.0, 1e-4, 128, "slabs"),
)
EARLY_STOP = CASES[3]
COLUMN_COUNTS = (1, 16, 65, 260)


def case_id(c) -> str:
	return f"n{c[0]}-d{c[1]}-{c[2]}-r{c[6]}" + (f"-{c[7]}" if c[7] else "")


def case_points(c) -> np.ndarray:
	"""Uniform in [0, 1]^d, seeded; the duplicates case repeats its first 20 points as its last 20."""
	n, d = c[0], c[1]
	X = R.points(n, d, seed=n + d).copy()
	if c[7] == "duplicates":
		X[-20:] = X[:20]
	return X


def operator(c):
	from primate_amd.operators import KernelOperator

	n, d, name, ell, s, sigma2, rank, _ = c
	return KernelOperator(case_points(c), name, lengthscale=ell, outputscale=s, noise=sigma2)


_cache = {}


def k0_model(c):
	"""(z, K0, dK0): the rounded points, s phi(r2) in long double and its elementwise bound. Computed once, read-only."""
	if c not in _cache:
		n, d, name, ell, s, sigma2, rank, _ = c
		z = R.scaled_points(case_points(c), ell, np.float64)
		r2 = R.r2_exact(z)
		K0 = LD(s) * R.phi(name, r2)
		nrm = np.sqrt(np.sum(z.astype(LD) ** 2, axis=1))
		eps = LD(EPS)
		dr2 = LD(d + 3) * eps * (nrm[:, None] + nrm[None, :]) ** 2
		dK = LD(s) * np.abs(R.phi(name, np.maximum(r2 - dr2, LD(0))) - R.phi(name, r2 + dr2)) + LD(R.C_EXP) * eps * K0
		dK_product = dK.copy()  # §4.15's own: the diagonal rule alone (the product's MFMA dot product is not the norm's fma chain)
		dK_product[np.diag_indices(n)] = LD(R.C_EXP) * eps * K0[np.diag_indices(n)]
		same = r2 == 0  # the diagonal, and pairs of bitwise-equal rounded points (r2_exact sums squares of differences)
		dK[same] = LD(R.C_EXP) * eps * K0[same]
		for Z in (z, K0, dK, dK_product):
			Z.setflags(write=False)
		_cache[c] = (z, K0, dK, dK_product)
	return _cache[c][:3]


def k0_product_bound(c):
	"""dK0 as §4.15 has it, for the operator's product: exact zeros of r2 on the diagonal only."""
	k0_model(c)
	return _cache[c][3]


def emulate_k0(z: np.ndarray, name: str, s: float) -> np.ndarray:
	"""K0 by norms plus dot product entirely in float64, both summed over the coordinates in order: what the column kernel computes up to its fmas."""
	n = z.shape[0]
	nrm, g = np.zeros(n), np.zeros((n, n))
	for k in range(z.shape[1]):  # (norm and dot product in the same order: see the module docstring)
		nrm += z[:, k] * z[:, k]
		g += z[:, k][:, None] * z[:, k][None, :]
	r2 = np.maximum(nrm[:, None] + nrm[None, :] - 2.0 * g, 0.0)
	np.fill_diagonal(r2, 0.0)
	return s * R.phi(name, r2)


def factor(K0: np.ndarray, s: float, rank_max: int, tol: float = 0.0):
	"""(L, pivots, d) by the definition, in K0's dtype: L is n x rank_max with zero columns beyond the rank, pivots has -1 there."""
	T = K0.dtype.type
	n = K0.shape[0]
	rank_max = min(rank_max, n)
	d = np.full(n, T(s))
	L = np.zeros((n, rank_max), dtype=K0.dtype)
	piv = np.full(rank_max, -1, dtype=np.int64)
	stop = T(max(tol, 64.0 * np.finfo(np.float64).eps)) * T(s)
	for k in range(rank_max):
		p = int(np.argmax(d))  # (the first of equal maxima)
		if not d[p] > stop:
			break
		col = (K0[:, p] - L[:, :k] @ L[p, :k]) / np.sqrt(d[p])
		dead = d == 0
		dead[p] = False
		col[dead] = 0
		L[:, k] = col
		d = np.maximum(d - col * col, T(0))
		d[p] = 0
		piv[k] = p
	return L, piv, d


def check_factor(c, L: np.ndarray, pivots: np.ndarray, limit: float, tag: str) -> dict:
	"""Asserts the four properties of the module docstring at `limit` times their bars; returns the measured fractions and the rank."""
	n, d, name, ell, s, sigma2, rank_max, _ = c
	rank_max = min(rank_max, n)
	z, K0, dK = k0_model(c)
	assert L.shape == (n, rank_max) and pivots.shape == (rank_max,)
	r = int(np.sum(pivots >= 0))
	piv = pivots[:r].astype(np.int64)
	assert np.all(pivots[:r] >= 0) and np.all(pivots[r:] == -1), "the pivots are not a prefix"
	assert np.all(piv < n) and len(set(piv.tolist())) == r, "the pivots are not distinct"
	assert not L[:, r:].any(), "columns beyond the rank are not zero"
	eps, sl = LD(EPS), LD(s)
	flat = LD(4 * (rank_max + 2)) * eps * sl
	Ll = L.astype(LD)
	La = np.abs(Ll)
	S2 = np.sum(Ll * Ll, axis=1)
	dKd = np.diagonal(dK)
	res_bar = dKd + LD(rank_max + 8) * eps * S2 + flat
	worst_bar = float(np.max(res_bar) / sl)
	res_frac = float(np.max(np.maximum(S2 - sl, LD(0)) / res_bar))
	int_frac = 0.0
	for p in piv:
		bar = dK[p] + LD(rank_max + 8) * eps * (La @ La[p]) + flat
		worst_bar = max(worst_bar, float(np.max(bar) / sl))
		int_frac = max(int_frac, float(np.max(np.abs(Ll @ Ll[p] - K0[p]) / bar)))
	## greedy: the long-double factor rebuilt from the pivots, its residual diagonal at the start of every step
	dm = np.full(n, sl)
	Lm = np.zeros((n, max(r, 1)), dtype=LD)
	S2k = np.zeros(n, dtype=LD)
	greedy_frac = 0.0
	for k, p in enumerate(piv):
		gbar = LD(2) * np.max(dKd + LD(rank_max + 8) * eps * S2k + flat)
		worst_bar = max(worst_bar, float(gbar / sl))
		assert dm[p] > 0, f"step {k}: the model's residual at the pivot {p} is not positive"
		greedy_frac = max(greedy_frac, float((np.max(dm) - dm[p]) / gbar))
		col = (K0[:, p] - Lm[:, :k] @ Lm[p, :k]) / np.sqrt(dm[p])
		Lm[:, k] = col
		dm = np.maximum(dm - col * col, LD(0))
		dm[p] = LD(0)
		S2k = S2k + Ll[:, k] * Ll[:, k]
	out = dict(rank=r, bar_over_s=worst_bar, residual=res_frac, interpolation=int_frac, greedy=greedy_frac)
	print(f"[kernelprecond-factor] {tag} {case_id(c)}: rank {r}/{rank_max} bar/s {worst_bar:.2e} residual {res_frac:.3f} interpolation {int_frac:.3f} greedy {greedy_frac:.3f} (limit {limit})")
	assert worst_bar <= 1e-9, "the bar does not discriminate"
	assert res_frac <= limit and int_frac <= limit and greedy_frac <= limit
	return out


def dense_p(L: np.ndarray, sigma2: float):
	"""(P^{-1/2}, cond P, logdet P, P) of P = L L^T + sigma2 I by eigh, in float64."""
	P = L @ L.T
	P[np.diag_indices_from(P)] += sigma2
	lam, U = np.linalg.eigh(P)
	return (U / np.sqrt(lam)) @ U.T, float(lam[-1] / lam[0]), float(np.sum(np.log(lam))), P


def apply_bar(cond_p: float, ref: np.ndarray) -> float:
	"""16 eps cond(P) max |ref| (eps = 2^-52, as numpy.finfo has it)."""
	return 16.0 * float(np.finfo(np.float64).eps) * cond_p * float(np.max(np.abs(ref)))


def product_model(c, L: np.ndarray, X: np.ndarray):
	"""(Y, bar): Y = M A M X with M = eigh(P)^{-1/2} from the given L and A the long-double model of §4.15, and the scalar bar per
	column: the apply's bar on V = M X through |A| |M| (2-norms; sqrt(n) from the max norm of the error to its 2-norm), the product's
	own bar (§4.15's formula evaluated on V: dK0 |V| + (n + 2) eps K0 |V| + 2 eps sigma2 |V|) through |M|, and the apply's bar on the
	result. The product itself is long double; the bars are float64 arithmetic."""
	n, d, name, ell, s, sigma2, rank_max, _ = c
	z, K0, dK = k0_model(c)
	M, cond, _, _ = dense_p(L, sigma2)
	K64 = K0.astype(np.float64)
	A = K64.copy()
	A[np.diag_indices(n)] += sigma2
	V = M @ X
	T = (K0 @ V.astype(LD) + LD(sigma2) * V.astype(LD)).astype(np.float64)
	Va = np.abs(V)
	tbar = k0_product_bound(c).astype(np.float64) @ Va + (n + 2) * EPS * (K64 @ Va) + 2 * EPS * sigma2 * Va
	Y = M @ T
	nA, nM = float(np.linalg.norm(A, 2)), float(np.linalg.norm(M, 2))
	e = 16.0 * float(np.finfo(np.float64).eps) * cond
	bar = np.sqrt(n) * e * np.max(Va, axis=0) * nA * nM + nM * np.linalg.norm(tbar, axis=0) + e * np.max(np.abs(Y), axis=0)
	return Y, bar
