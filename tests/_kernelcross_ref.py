"""The model of the cross-covariance tests and its bar.

The model takes z* and z ROUNDED TO THE OPERATOR'S DTYPE (z* with the TRAINING centre), forms r2_ij = sum_k (z*_ik - z_jk)^2 in long
double - no cancellation -, C = s phi(r2), and computes Y = C W (forward) or Y = C^T U (adjoint) in long double.

The bar per output element is the forward bound of tests/_kernelop_ref.py without its diagonal and noise terms:

    dr2_ij = (d + 3) eps (|z*_i| + |z_j|)^2                                        eps = unit roundoff of the dtype
    dC_ij  = s |phi(max(r2 - dr2, 0)) - phi(r2 + dr2)| + C_EXP eps C_ij
    bar    = sum_j dC |W| + (nsum + 2) eps sum_j C |W|                             nsum = the points summed over (n forward, m adjoint)
"""

import numpy as np

import _kernelop_ref as R

LD = np.longdouble
PROFILES = R.PROFILES
C_EXP = R.C_EXP
S = 1.7
## (m, n, d, b, variant): the issue's table
CASES = (
	(1, 1, 1, 1, "plain"),
	(15, 17, 3, 3, "plain"),
	(129, 257, 3, 16, "plain"),
	(33, 1000, 8, 65, "plain"),
	(40, 130, 17, 5, "plain"),
	(64, 300, 2, 260, "plain"),
	(48, 200, 3, 8, "coincident"),
	(48, 200, 3, 8, "coincident_offset"),
)
CASE_IDS = tuple(f"m{m}_n{n}_d{d}_b{b}_{v}" for m, n, d, b, v in CASES)


def lengthscale_of(d: int):
	"""The pattern of _kernelop_ref.CPU_CASES: 0.3 at d = 1, 0.4 at d = 2, per dimension at d = 3, 1.0 at d = 8, 1.5 at d = 17."""
	return {1: 0.3, 2: 0.4, 3: np.array([0.5, 0.3, 0.8]), 8: 1.0, 17: 1.5}[d]


def case_points(m: int, n: int, d: int, variant: str, dtype):
	"""(X, Xnew): uniform in the unit cube; "coincident": the first 20 new points are training points 0, 7, 14, ...; "_offset": every
	point moved by 1e4."""
	off = 1e4 if variant.endswith("offset") else 0.0
	X = R.points(n, d, seed=11, offset=off, dtype=dtype)
	Xn = R.points(m, d, seed=12, offset=off, dtype=dtype)
	if variant.startswith("coincident"):
		Xn[:20] = X[np.arange(20) * 7]
	return X, Xn


def scaled_new_points(X: np.ndarray, Xnew: np.ndarray, lengthscale, dtype) -> np.ndarray:
	"""z* as the library defines it: the centre is the TRAINING points' (the float64 sum in row order over n), (x* - mean) / l is
	float64 arithmetic, and the result is rounded once to `dtype`."""
	X = np.asarray(X, dtype=dtype)
	X = X.reshape(-1, 1) if X.ndim == 1 else X
	Xnew = np.asarray(Xnew, dtype=dtype).reshape(-1, X.shape[1])
	mean = np.cumsum(X, axis=0, dtype=np.float64)[-1] / np.float64(X.shape[0])
	ls = np.broadcast_to(np.asarray(lengthscale, dtype=np.float64), (X.shape[1],))
	return ((Xnew.astype(np.float64) - mean) / ls).astype(dtype)


def r2_cross(zs: np.ndarray, z: np.ndarray) -> np.ndarray:
	"""sum_k (z*_ik - z_jk)^2 in long double, m x n."""
	a, b = zs.astype(LD), z.astype(LD)
	out = np.zeros((a.shape[0], b.shape[0]), dtype=LD)
	for k in range(a.shape[1]):
		diff = a[:, k][:, None] - b[:, k][None, :]
		out += diff * diff
	return out


def cross_matrix(zs: np.ndarray, z: np.ndarray, name: str, s: float) -> np.ndarray:
	"""C in long double."""
	return LD(s) * R.phi(name, r2_cross(zs, z))


def model(zs: np.ndarray, z: np.ndarray, name: str, s: float, W: np.ndarray, trans: bool = False):
	"""(Y, bar) in long double: Y = C W (trans False; W n x b) or C^T W (W m x b) on the rounded points, and the forward bound of
	the module docstring for an evaluation in their dtype."""
	d = z.shape[1]
	eps = LD(R.eps_of(z.dtype))
	r2 = r2_cross(zs, z)
	C = LD(s) * R.phi(name, r2)
	ns = np.sqrt(np.sum(zs.astype(LD) ** 2, axis=1))
	nz = np.sqrt(np.sum(z.astype(LD) ** 2, axis=1))
	dr2 = LD(d + 3) * eps * (ns[:, None] + nz[None, :]) ** 2
	dC = LD(s) * np.abs(R.phi(name, np.maximum(r2 - dr2, LD(0))) - R.phi(name, r2 + dr2)) + LD(C_EXP) * eps * C
	if trans:
		C, dC = C.T, dC.T
	nsum = C.shape[1]
	Wl, Wa = W.astype(LD), np.abs(W.astype(LD))
	return C @ Wl, dC @ Wa + LD(nsum + 2) * eps * (C @ Wa)


def emulate(zs: np.ndarray, z: np.ndarray, name: str, s: float, W: np.ndarray, trans: bool = False, diagonal_rule=None) -> np.ndarray:
	"""The norms-plus-dot evaluation entirely in the points' dtype (NumPy): what a device kernel computes up to summation order.
	diagonal_rule: pairs (i, j) whose r2 is forced to 0 - a mutant, for the test that the bar sees an applied diagonal rule."""
	T = z.dtype.type
	ns = np.sum(zs * zs, axis=1, dtype=z.dtype)
	nz = np.sum(z * z, axis=1, dtype=z.dtype)
	r2 = np.maximum(ns[:, None] + nz[None, :] - T(2) * (zs @ z.T), T(0))
	if diagonal_rule is not None:
		r2[diagonal_rule] = T(0)
	C = T(s) * R.phi(name, r2).astype(z.dtype)
	return ((C.T if trans else C) @ W.astype(z.dtype)).astype(z.dtype)


def condition_limit(name: str, variant: str, dtype) -> float:
	"""max bar / max |Y| a case must stay under, or passing the bar says nothing: 1e-3 (fp32), 1e-10 (fp64); matern12 on the
	coincident cases in fp64 alone 1e-6 (its cusp at r = 0; DESIGN.md §4.16 has the precedent)."""
	if np.dtype(dtype) == np.float32:
		return 1e-3
	return 1e-6 if (name == "matern12" and variant.startswith("coincident")) else 1e-10


def check_condition(Y, bar, name: str, variant: str, dtype) -> float:
	ratio = float(np.max(bar) / np.max(np.abs(Y)))
	limit = condition_limit(name, variant, dtype)
	assert ratio <= limit, f"the bar is {ratio:.3e} of max |Y| (limit {limit:g}): the case does not discriminate"
	return ratio


def worst(got: np.ndarray, Y, bar) -> float:
	"""max |got - Y| / bar."""
	return float(np.max(np.abs(got.astype(LD) - Y) / bar))


_CACHE = {}


def case_data(idx: int, name: str, dtype, trans: bool):
	"""Everything one cell of the table needs, computed once and shared (the arrays are read-only): X, Xnew, lengthscale, z, z*,
	the operand, the model's Y and the bar."""
	key = (idx, name, np.dtype(dtype).str, bool(trans))
	if key not in _CACHE:
		m, n, d, b, variant = CASES[idx]
		ls = lengthscale_of(d)
		X, Xn = case_points(m, n, d, variant, dtype)
		z = R.scaled_points(X, ls, dtype)
		zs = scaled_new_points(X, Xn, ls, dtype)
		W = R.probes(m if trans else n, b, seed=idx, dtype=dtype)
		Y, bar = model(zs, z, name, S, W, trans)
		for a in (X, Xn, z, zs, W, Y, bar):
			a.setflags(write=False)
		_CACHE[key] = dict(X=X, Xnew=Xn, ls=ls, z=z, zs=zs, W=W, Y=Y, bar=bar, variant=variant)
	return _CACHE[key]
