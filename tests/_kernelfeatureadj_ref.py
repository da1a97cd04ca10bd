"""The model of the adjoint feature product's tests, its bar, and the dense NumPy weight-space model of
`gp.feature_posterior`.

The model takes z and Omega ROUNDED TO THE OPERATOR'S DTYPE, as tests/_kernelfeature_ref.py does, and forms in long double

    Z = a [cos g | sin g]^T U,        g_ij = sum_k Omega_jk z_ik,        a = sqrt(s / F2)

The bar per output element reuses that module's terms with the sum now over the row points:

    dc_ij  = (d + 2) eps sum_k |Omega_jk| |z_ik| + C_TRIG eps
    bar_jc = a sum_i dc_ij |U_ic| + (nrows + 2) eps a sum_i |trig g_ij| |U_ic|        trig = cos for rows [0, F2), sin for [F2, 2 F2)

(nrows + 2) eps: the nrows-term sum of the second product, the square root and the product by a.
"""

import numpy as np

import _kernelcross_ref as X
import _kernelfeature_ref as Fr
import _kernelop_ref as R

LD = np.longdouble
PROFILES = R.PROFILES
C_TRIG = Fr.C_TRIG
S = Fr.S
FREQ_SEED = Fr.FREQ_SEED
## (n, d, lengthscale, F2, b): the six cells of the forward table and the adjoint's own seventh - one row block of frequencies and
## many slabs of points, the last one shorter
CASES = Fr.CASES + ((2000, 3, 0.2, 40, 3),)
CASE_IDS = tuple(f"n{n}_d{d}_F{f2}_b{b}" for n, d, _, f2, b in CASES)
CROSS_M = Fr.CROSS_M  # new points of the cross form, for the first six cells
N_CROSS_CASES = len(Fr.CASES)
MUTANT_CASE = 2  # (130, 17, 1.5, 33, 5): the cell the four faults are planted in


def rows_of(idx: int) -> tuple:
	"""The row sets of cell idx: None (the operator's points) and, for the first six cells, the new points of the cross form."""
	return (None, *CROSS_M) if idx < N_CROSS_CASES else (None,)


def model(z: np.ndarray, om: np.ndarray, s: float, U: np.ndarray):
	"""(Z, bar) in long double for z and Omega in the operator's dtype: Z = Phi^T U and the forward bound of the module docstring."""
	d, f2, nrows = z.shape[1], om.shape[0], z.shape[0]
	eps = LD(R.eps_of(z.dtype))
	g = Fr.phases(z, om)  # nrows x F2
	a = np.sqrt(LD(s) / LD(f2))
	cg, sg = np.cos(g), np.sin(g)
	Ul = U.astype(LD)
	Z = a * np.vstack([cg.T @ Ul, sg.T @ Ul])
	dc = LD(d + 2) * eps * (np.abs(z.astype(LD)) @ np.abs(om.astype(LD)).T) + LD(C_TRIG) * eps
	first = a * (dc.T @ np.abs(Ul))
	bar = np.vstack([first, first]) + LD(nrows + 2) * eps * a * np.vstack([np.abs(cg).T @ np.abs(Ul), np.abs(sg).T @ np.abs(Ul)])
	return Z, bar


def emulate(z: np.ndarray, om: np.ndarray, s: float, U: np.ndarray, fault: str = None) -> np.ndarray:
	"""The evaluation entirely in z's dtype (NumPy): what a device kernel computes up to summation order. fault, for the test that the
	bar sees them: "swap" - the cosine and sine row blocks exchanged; "no_scale" - a left out; "padding" - the padded points of the last
	tile of 16 (zero z: cos 0 = 1, sin 0 = 0) weighed against a non-zero U, as an unguarded fetch of a column-major U would (it reads
	on into the first rows of the next column); "drop_tail" - the remainder tile of points left out."""
	T = z.dtype.type
	f2, nrows = om.shape[0], z.shape[0]
	Ud = U.astype(z.dtype)
	zz = z
	if fault == "drop_tail":
		keep = nrows // 16 * 16
		zz, Ud = z[:keep], Ud[:keep]
	g = (zz @ om.T).astype(z.dtype)
	cg, sg = np.cos(g).astype(z.dtype), np.sin(g).astype(z.dtype)
	zc, zs = cg.T @ Ud, sg.T @ Ud
	if fault == "padding":
		pad = -nrows % 16
		zc = zc + np.sum(np.roll(U.astype(z.dtype), -1, axis=1)[:pad], axis=0)[None, :]
	a = T(1) if fault == "no_scale" else np.sqrt(T(s) / T(f2)).astype(z.dtype)
	out = (a * np.vstack([zs, zc] if fault == "swap" else [zc, zs])).astype(z.dtype)
	return out


def limit_of(name: str, dtype) -> float:
	"""What max bar / max |Z| may be at most: matern12 gets the wider limit because its frequencies are Cauchy (the largest bar sits in
	the row of the largest |Omega_j|, max |Z| is over all rows)."""
	f32 = np.dtype(dtype) == np.float32
	if name == "matern12":
		return 3e-2 if f32 else 1e-10
	return 3e-3 if f32 else 1e-11


def check_condition(Z, bar, name: str, dtype) -> float:
	"""The bar must stay a small fraction of the result, or passing it says nothing."""
	ratio = float(np.max(bar) / np.max(np.abs(Z)))
	limit = limit_of(name, dtype)
	assert ratio <= limit, f"the bar is {ratio:.3e} of max |Z| (limit {limit:g}): the case does not discriminate"
	return ratio


worst = R.worst
_CACHE = {}


def case_data(idx: int, name: str, dtype, m=None):
	"""Everything one cell of the table needs, computed once and shared (the arrays are read-only): X, Xnew (m new points offset by 0.5,
	or None: the rows are the operator's own points), the lengthscale, the row points' z, Omega in float64 and rounded, U, the model's
	Z and the bar."""
	key = (idx, name, np.dtype(dtype).str, m)
	if key not in _CACHE:
		n, d, ls, f2, b = CASES[idx]
		Xt = R.points(n, d, seed=11, dtype=dtype)
		Xn = None if m is None else R.points(m, d, seed=12, offset=0.5, dtype=dtype)
		z = R.scaled_points(Xt, ls, dtype) if m is None else X.scaled_new_points(Xt, Xn, ls, dtype)
		om64 = Fr.frequencies(name, f2, d, FREQ_SEED + idx)
		om = om64.astype(dtype)
		U = R.probes(z.shape[0], b, seed=100 + idx, dtype=dtype)
		Z, bar = model(z, om, S, U)
		arrays = [Xt, z, om64, om, U, Z, bar] + ([] if Xn is None else [Xn])
		for a in arrays:
			a.setflags(write=False)
		_CACHE[key] = dict(X=Xt, Xnew=Xn, ls=ls, z=z, omega64=om64, omega=om, U=U, Z=Z, bar=bar)
	return _CACHE[key]


def gram_model(z: np.ndarray, om: np.ndarray, s: float):
	"""(G, bar): Phi^T Phi in long double and the bar propagated through the two products that form it on the device: column c of G is
	the adjoint of T = Phi e_c. The forward product's bar on T (tests/_kernelfeature_ref.py with W = e_c) passes through the exact
	adjoint as |Phi|^T bar_T, and the adjoint's own bar is taken at U = |T| + bar_T."""
	f2 = om.shape[0]
	I = np.eye(2 * f2, dtype=z.dtype)
	T, bar_T = Fr.model(z, om, s, I)
	P = Fr.feature_matrix(z, om, s)
	_, bar_adj = model(z, om, s, (np.abs(T) + bar_T).astype(LD))
	return P.T @ P, np.abs(P).T @ bar_T + bar_adj


## ---- the weight-space model of gp.feature_posterior on the GP setting of tests/_kernelfeature_ref.py ---------------------------------
F2_GP = 256
FREQ_SEED_GP = 5


def weight_space_dense(G, om: np.ndarray) -> dict:
	"""The dense float64 weight-space model: M = Phi^T Phi + sigma2 I = L L^T, w_bar, the predictive mean and variance at the new
	points and the log marginal likelihood by the formula of the issue."""
	PX = Fr.feature_matrix(G["z"], om, Fr.S_GP).astype(np.float64)
	Ps = Fr.feature_matrix(G["zs"], om, Fr.S_GP).astype(np.float64)
	n, m2, s2, y = PX.shape[0], PX.shape[1], G["noise"], G["y"]
	h = PX.T @ y
	M = PX.T @ PX + s2 * np.eye(m2)
	L = np.linalg.cholesky(M)
	wbar = np.linalg.solve(M, h)
	B = np.linalg.solve(L, Ps.T)  # L^-1 phi*
	mll = -0.5 * ((y @ y - h @ wbar) / s2 + 2.0 * np.sum(np.log(np.diag(L))) + (n - m2) * np.log(s2) + n * np.log(2.0 * np.pi))
	return dict(PX=PX, Ps=Ps, L=L, wbar=wbar, mean=Ps @ wbar, var=s2 * np.sum(B * B, axis=0), mll=float(mll))


def function_space_dense(G, om: np.ndarray) -> dict:
	"""The same model in function space: A = Phi Phi^T + sigma2 I (n x n), mean = Phi* Phi^T A^-1 y, var = diag(Phi* Phi*^T - Phi* Phi^T
	A^-1 Phi Phi*^T), mll = -1/2 (y^T A^-1 y + log det A + n log 2 pi)."""
	PX = Fr.feature_matrix(G["z"], om, Fr.S_GP).astype(np.float64)
	Ps = Fr.feature_matrix(G["zs"], om, Fr.S_GP).astype(np.float64)
	n, y = PX.shape[0], G["y"]
	A = PX @ PX.T + G["noise"] * np.eye(n)
	Cs = Ps @ PX.T
	AinvCt = np.linalg.solve(A, Cs.T)
	_, logdet = np.linalg.slogdet(A)
	mll = -0.5 * (y @ np.linalg.solve(A, y) + logdet + n * np.log(2.0 * np.pi))
	return dict(mean=AinvCt.T @ y, var=np.sum(Ps * Ps, axis=1) - np.sum(Cs * AinvCt.T, axis=1), mll=float(mll))


def path_value_ld(G, om: np.ndarray, W: np.ndarray, Xq: np.ndarray):
	"""Phi(x) W at arbitrary points in long double (Fr.path_value_ld without a data term)."""
	return Fr.path_value_ld(G, "rbf", om, W, None, Xq)
