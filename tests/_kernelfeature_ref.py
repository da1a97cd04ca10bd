"""The model of the random-feature tests and its bar, and the NumPy pathwise model of `gp.sample_paths`.

The feature model takes z and Omega ROUNDED TO THE OPERATOR'S DTYPE (the map is defined on these), forms g_ij = sum_k Omega_jk z_ik,
cos g, sin g and Y = a (cos g W_c + sin g W_s), a = sqrt(s / F2), in long double.

The bar per output element is a forward bound on an evaluation in the operator's dtype, not a fitted number:

    dg_ij  = (d + 2) eps sum_k |Omega_jk| |z_ik|                                   eps = unit roundoff of the dtype
    dc_ij  = dg_ij + C_TRIG eps
    bar_ic = a sum_j dc_ij (|W_jc| + |W_{F2+j,c}|) + (2 F2 + 2) eps a sum_j (|cos g_ij| |W_jc| + |sin g_ij| |W_{F2+j,c}|)

dg: the d products and d - 1 additions of the dot product, each relative to a partial sum bounded by sum |Omega| |z|. dc: cos and sin
have slope at most 1, so the error of g passes through unamplified, and C_TRIG eps is the functions' own arithmetic (range reduction,
the polynomial): C_TRIG = 4 by the convention of _kernelop_ref.C_EXP. (2 F2 + 2) eps: the 2 F2-term sum of the second product, the
square root and the product by a.
"""

import numpy as np

import _kernelcross_ref as X
import _kernelop_ref as R

LD = np.longdouble
PROFILES = R.PROFILES
C_TRIG = 4.0
S = 1.5
## (n, d, lengthscale, F2, b): the issue's table
CASES = ((1, 1, 0.3, 1, 1), (17, 3, 0.5, 16, 1), (130, 17, 1.5, 33, 5), (257, 2, 0.3, 500, 260), (300, 8, 1.0, 1024, 16), (129, 64, 4.0, 100, 17))
CASE_IDS = tuple(f"n{n}_d{d}_F{f2}_b{b}" for n, d, _, f2, b in CASES)
CROSS_M = (1, 40, 130)  # new points of the cross form, offset by 0.5
DOF = {"matern12": 1.0, "matern32": 3.0, "matern52": 5.0}
## Case idx draws its frequencies with the seed FREQ_SEED + idx. The condition of a cell (check_condition) is a property of the model
## alone, and the one-row cells (m = 1: max |Y| over b values only) sit closest to it: 2.5e-3 of the 3e-3 allowed in fp32 at F2 = 1024.
## Some draws put such a cell just above (3.1e-3); these seeds keep every cell under, with max |g| = 1.0e3 from the Cauchy
## frequencies of matern12.
FREQ_SEED = 400


def frequencies(name: str, f2: int, d: int, seed) -> np.ndarray:
	"""The frequency law as the issue defines it (float64): G = standard_normal((F2, d)); rbf: G; matern: then u = chisquare(2 nu, F2),
	Omega_j = G_j sqrt(2 nu / u_j)."""
	rng = np.random.default_rng(seed)
	G = rng.standard_normal((f2, d))
	if name == "rbf":
		return G
	u = rng.chisquare(DOF[name], f2)
	return G * np.sqrt(DOF[name] / u)[:, None]


def phases(z: np.ndarray, om: np.ndarray):
	"""g = z Omega^T in long double (rows x F2)."""
	return z.astype(LD) @ om.astype(LD).T


def feature_matrix(z: np.ndarray, om: np.ndarray, s: float):
	"""Phi in long double: rows x 2 F2."""
	g = phases(z, om)
	return np.sqrt(LD(s) / LD(om.shape[0])) * np.hstack([np.cos(g), np.sin(g)])


def model(z: np.ndarray, om: np.ndarray, s: float, W: np.ndarray):
	"""(Y, bar) in long double for z and Omega in the operator's dtype: Y = Phi W and the forward bound of the module docstring."""
	d, f2 = z.shape[1], om.shape[0]
	eps = LD(R.eps_of(z.dtype))
	g = phases(z, om)
	a = np.sqrt(LD(s) / LD(f2))
	cg, sg = np.cos(g), np.sin(g)
	Wl = W.astype(LD)
	Wc, Ws = Wl[:f2], Wl[f2:]
	Y = a * (cg @ Wc + sg @ Ws)
	dc = LD(d + 2) * eps * (np.abs(z.astype(LD)) @ np.abs(om.astype(LD)).T) + LD(C_TRIG) * eps
	bar = a * (dc @ (np.abs(Wc) + np.abs(Ws))) + LD(2 * f2 + 2) * eps * a * (np.abs(cg) @ np.abs(Wc) + np.abs(sg) @ np.abs(Ws))
	return Y, bar


def emulate(z: np.ndarray, om: np.ndarray, s: float, W: np.ndarray, swap: bool = False, no_scale: bool = False) -> np.ndarray:
	"""The evaluation entirely in z's dtype (NumPy): what a device kernel computes up to summation order. swap: the sine rows weigh the
	cosines and the other way round; no_scale: a is left out - mutants, for the test that the bar sees them."""
	T = z.dtype.type
	f2 = om.shape[0]
	g = (z @ om.T).astype(z.dtype)
	cg, sg = np.cos(g).astype(z.dtype), np.sin(g).astype(z.dtype)
	Wd = W.astype(z.dtype)
	Wc, Ws = (Wd[f2:], Wd[:f2]) if swap else (Wd[:f2], Wd[f2:])
	a = T(1) if no_scale else np.sqrt(T(s) / T(f2)).astype(z.dtype)
	return (a * (cg @ Wc + sg @ Ws)).astype(z.dtype)


def check_condition(Y, bar, dtype) -> float:
	"""The bar must stay a small fraction of the result, or passing it says nothing: max bar / max |Y| <= 3e-3 (fp32), 1e-11 (fp64)."""
	ratio = float(np.max(bar) / np.max(np.abs(Y)))
	limit = 3e-3 if np.dtype(dtype) == np.float32 else 1e-11
	assert ratio <= limit, f"the bar is {ratio:.3e} of max |Y| (limit {limit:g}): the case does not discriminate"
	return ratio


worst = R.worst
_CACHE = {}


def case_data(idx: int, name: str, dtype, m=None):
	"""Everything one cell of the table needs, computed once and shared (the arrays are read-only): X, Xnew (m new points offset by 0.5,
	or None: the rows are the operator's own points), the lengthscale, the row points' z, Omega in float64 and rounded, W, the model's
	Y and the bar."""
	key = (idx, name, np.dtype(dtype).str, m)
	if key not in _CACHE:
		n, d, ls, f2, b = CASES[idx]
		Xt = R.points(n, d, seed=11, dtype=dtype)
		Xn = None if m is None else R.points(m, d, seed=12, offset=0.5, dtype=dtype)
		z = R.scaled_points(Xt, ls, dtype) if m is None else X.scaled_new_points(Xt, Xn, ls, dtype)
		om64 = frequencies(name, f2, d, FREQ_SEED + idx)
		om = om64.astype(dtype)
		W = R.probes(2 * f2, b, seed=idx, dtype=dtype)
		Y, bar = model(z, om, S, W)
		arrays = [Xt, z, om64, om, W, Y, bar] + ([] if Xn is None else [Xn])
		for a in arrays:
			a.setflags(write=False)
		_CACHE[key] = dict(X=Xt, Xnew=Xn, ls=ls, z=z, omega64=om64, omega=om, W=W, Y=Y, bar=bar)
	return _CACHE[key]


## ---- the pathwise model on the GP setting of tests/test_gpu_kernelcross.py (copied as data set-up) ------------------------------------
N_GP, M_GP, S_GP, NOISE_GP, LS_GP = 300, 40, 1.5, 0.1, 0.4
_gp_cache = {}


def gp_case(name: str, noise: float = NOISE_GP, ls: float = LS_GP):
	"""Points, one column of observations and the dense float64 pieces (A, C, the exact posterior mean and covariance), once per
	profile, noise and lengthscale, read-only."""
	key = (name, float(noise), float(ls))
	if key not in _gp_cache:
		rng = np.random.default_rng(77)
		Xt = R.points(N_GP, 2, seed=21)
		Xn = R.points(M_GP, 2, seed=22) + 0.5
		Xn[:5] = Xt[[3, 50, 120, 200, 299]]
		y = np.sin(6 * Xt[:, 0]) + np.sqrt(NOISE_GP) * rng.standard_normal(N_GP)
		z, zs = R.scaled_points(Xt, ls, np.float64), X.scaled_new_points(Xt, Xn, ls, np.float64)
		A = R.dense_matrix(z, name, S_GP, noise)
		Cm = X.cross_matrix(zs, z, name, S_GP).astype(np.float64)
		Kss = (LD(S_GP) * R.phi(name, X.r2_cross(zs, zs))).astype(np.float64)
		AinvCt = np.linalg.solve(A, Cm.T)
		mean = AinvCt.T @ y
		cov = Kss - Cm @ AinvCt
		out = dict(X=Xt, Xnew=Xn, y=y, z=z, zs=zs, A=A, C=Cm, AinvCt=AinvCt, mean=mean, cov=cov, noise=float(noise), ls=float(ls))
		for a in out.values():
			if isinstance(a, np.ndarray):
				a.setflags(write=False)
		_gp_cache[key] = out
	return _gp_cache[key]


def path_dense(G, om: np.ndarray, W: np.ndarray, E=None) -> tuple:
	"""(F, V): the dense float64 paths at the new points from the same Omega, W and eps: V = A^-1 (y - Phi_X W - sqrt(noise) E),
	F = Phi* W + C V."""
	PX = feature_matrix(G["z"], om, S_GP).astype(np.float64)
	Ps = feature_matrix(G["zs"], om, S_GP).astype(np.float64)
	rhs = G["y"][:, None] - PX @ W
	if E is not None:
		rhs = rhs - np.sqrt(G["noise"]) * E
	V = np.linalg.solve(G["A"], rhs)
	return Ps @ W + G["C"] @ V, V


def path_cov_given_omega(G, om: np.ndarray) -> np.ndarray:
	"""The covariance of the paths at the new points given Omega: (Phi* - C A^-1 Phi_X)(...)^T + noise C A^-2 C^T."""
	PX = feature_matrix(G["z"], om, S_GP).astype(np.float64)
	Ps = feature_matrix(G["zs"], om, S_GP).astype(np.float64)
	P = Ps - G["AinvCt"].T @ PX
	return P @ P.T + G["noise"] * (G["AinvCt"].T @ G["AinvCt"])


def moments_hold(F: np.ndarray, G, om: np.ndarray) -> tuple:
	"""The two derived bars of the moment test, shared with the GPU test: per new point the sample mean within 6 standard errors of the
	exact posterior mean (unbiased for any Omega; the standard error from the model's covariance given Omega) and the sample variance
	within 6 sqrt(2 / (count - 1)) relative of the model's variance given Omega. Returns the two worst ratios to their bars."""
	count = F.shape[1]
	var = np.diag(path_cov_given_omega(G, om))
	r_mean = float(np.max(np.abs(F.mean(axis=1) - G["mean"]) / (6.0 * np.sqrt(var / count))))
	r_var = float(np.max(np.abs(F.var(axis=1, ddof=1) / var - 1.0) / (6.0 * np.sqrt(2.0 / (count - 1)))))
	return r_mean, r_var


def path_value_ld(G, name: str, om: np.ndarray, W: np.ndarray, V, Xq: np.ndarray):
	"""f_c at arbitrary points Xq (q x d) in long double, V held fixed: the scaled points are NOT rounded here (the finite differences of
	the gradient test move x by 1e-5)."""
	mean = np.cumsum(G["X"], axis=0, dtype=np.float64)[-1] / np.float64(G["X"].shape[0])
	zq = (Xq.astype(LD) - mean.astype(LD)) / LD(G["ls"])
	g = zq @ om.astype(LD).T
	out = np.sqrt(LD(S_GP) / LD(om.shape[0])) * np.hstack([np.cos(g), np.sin(g)]) @ W.astype(LD)
	if V is not None:
		zl = G["z"].astype(LD)
		r2 = np.zeros((zq.shape[0], zl.shape[0]), dtype=LD)
		for k in range(zl.shape[1]):
			diff = zq[:, k][:, None] - zl[:, k][None, :]
			r2 += diff * diff
		out = out + (LD(S_GP) * R.phi(name, r2)) @ V.astype(LD)
	return out
