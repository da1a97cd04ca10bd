"""The model of the kernel-gradient tests and its bar.

For A = s phi(r2) + sigma2 I on the ROUNDED z of the operator (`_kernelop_ref`), two matrices Z, W (n x m) and C_ij = sum_c Z_ic W_jc,
D_ijk = z_ik - z_jk, the model computes in long double, with r2 = sum_k D^2 (`_kernelop_ref.r2_exact`: no cancellation),

    g_l[k]   = (s / l_k) sum_ij C_ij chi(r2_ij) D_ijk^2          chi = -2 dphi/dr2
    g_s      =           sum_ij C_ij phi(r2_ij)
    g_sigma2 =           sum_i  C_ii

chi: rbf exp(-r2/2); matern12 exp(-r)/r, DEFINED 0 where r2 = 0; matern32 3 exp(-sqrt3 r); matern52 (5/3)(1 + sqrt5 r) exp(-sqrt5 r).

The bar is a forward bound, not a fitted number. eps = 2^-53, |C|_ij = sum_c |Z_ic| |W_jc|; dr2, C_EXP = 4, lo = max(r2 - dr2, 0),
hi = r2 + dr2 as in `_kernelop_ref.model`; dphi = |phi(lo) - phi(hi)|, dchi = |chi(lo) - chi(hi)| - for matern12 where lo = 0,
dchi = chi(r2) + chi(hi): the term may be dropped whole - both 0 on the diagonal; S = (2 n + 64) eps:

    bar_s      = sum |C| dphi + ((m + 2 + C_EXP) eps + S) sum |C| phi
    bar_sigma2 = (m + 2 + n) eps sum_i |C|_ii
    bar_l[k]   = (s / l_k) [ sum |C| dchi D_k^2 + ((m + 5 + C_EXP) eps + S) sum |C| chi D_k^2 + 4 eps sum |C| chi (|z_ik| + |z_jk|)^2 ]
                 + 2 eps |g_l[k]|

in order: r2's error through the monotone profile; the m-term dot and the profile's arithmetic; any summation order in which no
term passes through more than 2 n + 64 additions; an expanded evaluation of D^2 (granted whether used or not); the final scale.
"""

import numpy as np

import _kernelop_ref as R

LD = np.longdouble
EPS = LD(2.0) ** -53
C_EXP = LD(R.C_EXP)
CONDITION = 1e-6


def chi(name: str, r2):
	"""-2 dphi/dr2 on an array of r2 (any float type); matern12 is 0 where r2 = 0."""
	r2 = np.asarray(r2)
	T = r2.dtype.type
	if name == "rbf":
		return np.exp(-r2 / T(2))
	r = np.sqrt(r2)
	if name == "matern12":
		out = np.zeros_like(r2)
		pos = r2 > 0
		out[pos] = np.exp(-r[pos]) / r[pos]
		return out
	if name == "matern32":
		return T(3) * np.exp(-np.sqrt(T(3)) * r)
	if name == "matern52":
		a = np.sqrt(T(5)) * r
		return T(5) / T(3) * (T(1) + a) * np.exp(-a)
	raise ValueError(name)


def _blocks(n: int, step: int = 256):
	return [(i, min(n, i + step)) for i in range(0, n, step)]


def model(z: np.ndarray, name: str, ls, s: float, Z: np.ndarray, W: np.ndarray, flip=None):
	"""(g, bar), d + 2 long doubles each: [0, d) the lengthscales per dimension, [d] the outputscale, [d + 1] the noise, for the
	rounded points z (n x d, float64), the lengthscales ls (scalar or d) and the factors Z, W (n x m). flip = (i, j, k): that one
	difference enters as z_ik + z_jk - a fault for the tests of the bar, not a feature."""
	n, d = z.shape
	ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (d,)).astype(LD)
	Zl, Wl = np.asarray(Z, dtype=np.float64).reshape(n, -1).astype(LD), np.asarray(W, dtype=np.float64).reshape(n, -1).astype(LD)
	m = Zl.shape[1]
	zl = z.astype(LD)
	nrm = np.sqrt(np.sum(zl * zl, axis=1))
	S = LD(2 * n + 64) * EPS
	g, bar = np.zeros(d + 2, dtype=LD), np.zeros(d + 2, dtype=LD)
	raw, t1, t2, t3 = (np.zeros(d, dtype=LD) for _ in range(4))
	cphi = dphi_sum = LD(0)
	for i0, i1 in _blocks(n):
		idx = np.arange(i0, i1)
		r2 = R.r2_exact(z, idx)
		Cm, Ca = Zl[idx] @ Wl.T, np.abs(Zl[idx]) @ np.abs(Wl).T
		dr2 = LD(d + 3) * EPS * (nrm[idx][:, None] + nrm[None, :]) ** 2
		lo, hi = np.maximum(r2 - dr2, LD(0)), r2 + dr2
		ph, ch = R.phi(name, r2), chi(name, r2)
		dph, dch = np.abs(R.phi(name, lo) - R.phi(name, hi)), np.abs(chi(name, lo) - chi(name, hi))
		if name == "matern12":
			dch = np.where(lo == 0, ch + chi(name, hi), dch)
		dph[np.arange(idx.size), idx] = 0
		dch[np.arange(idx.size), idx] = 0
		g[d] += np.sum(Cm * ph)
		cphi += np.sum(Ca * ph)
		dphi_sum += np.sum(Ca * dph)
		g[d + 1] += np.sum(Cm[np.arange(idx.size), idx])
		bar[d + 1] += np.sum(Ca[np.arange(idx.size), idx])
		for k in range(d):
			D = zl[idx, k][:, None] - zl[None, :, k]
			if flip is not None and flip[2] == k and i0 <= flip[0] < i1:
				D[flip[0] - i0, flip[1]] = zl[flip[0], k] + zl[flip[1], k]
			D2 = D * D
			raw[k] += np.sum(Cm * ch * D2)
			t1[k] += np.sum(Ca * dch * D2)
			t2[k] += np.sum(Ca * ch * D2)
			t3[k] += np.sum(Ca * ch * (np.abs(zl[idx, k])[:, None] + np.abs(zl[None, :, k])) ** 2)
	g[:d] = LD(s) / ls * raw
	bar[:d] = LD(s) / ls * (t1 + (LD(m + 5) * EPS + C_EXP * EPS + S) * t2 + LD(4) * EPS * t3) + LD(2) * EPS * np.abs(g[:d])
	bar[d] = dphi_sum + (LD(m + 2) * EPS + C_EXP * EPS + S) * cphi
	bar[d + 1] = LD(m + 2 + n) * EPS * bar[d + 1]
	return g, bar


def emulate(z: np.ndarray, name: str, ls, s: float, Z: np.ndarray, W: np.ndarray, jmax=None) -> np.ndarray:
	"""The device evaluation in float64 NumPy: norms plus dot for r2 (clamped, 0 on the diagonal), differences for D. jmax: only the
	points j < jmax enter (a dropped remainder tile, for the tests of the bar)."""
	n, d = z.shape
	ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (d,))
	Z, W = np.asarray(Z, dtype=np.float64).reshape(n, -1), np.asarray(W, dtype=np.float64).reshape(n, -1)
	if jmax is not None:
		W = W.copy()
		W[jmax:] = 0.0
	nrm = np.sum(z * z, axis=1)
	r2 = np.maximum(nrm[:, None] + nrm[None, :] - 2.0 * (z @ z.T), 0.0)
	np.fill_diagonal(r2, 0.0)
	Cm = Z @ W.T
	out = np.zeros(d + 2)
	B = Cm * chi(name, r2)
	for k in range(d):
		D = z[:, k][:, None] - z[None, :, k]
		out[k] = s / ls[k] * np.sum(B * D * D)
	out[d] = np.sum(Cm * R.phi(name, r2))
	out[d + 1] = np.trace(Cm)
	return out


def groups(d: int):
	return (("lengthscale", slice(0, d)), ("outputscale", slice(d, d + 1)), ("noise", slice(d + 1, d + 2)))


def check_condition(g, bar) -> float:
	"""The condition of every case: max bar <= 1e-6 max |g| for each of the three groups, or passing the bar says nothing. Returns
	the worst ratio."""
	d = g.size - 2
	worst_ratio = 0.0
	for what, sl in groups(d):
		top, b = float(np.max(np.abs(g[sl]))), float(np.max(bar[sl]))
		assert b <= CONDITION * top, f"{what}: the bar {b:.3e} is above {CONDITION:g} of max |g| = {top:.3e}: the case does not discriminate"
		worst_ratio = max(worst_ratio, b / top if top > 0 else 0.0)  # (one point: the lengthscale sums and their bar are exactly 0)
	return worst_ratio


def worst(got, g, bar) -> float:
	"""max |got - g| / bar over the d + 2 values; where the bar is 0 (an exactly known value) equality is asked: 0, else inf."""
	err = np.abs(np.asarray(got).astype(LD) - g)
	ratio = np.where(bar > 0, err / np.where(bar > 0, bar, LD(1)), np.where(err == 0, LD(0), LD(np.inf)))
	return float(np.max(ratio))


## ---- the cases of the GPU tests: (n, d, m, profile, lengthscale per dimension?, offset, duplicate rows?) -----------------------
GPU_CASES = [
	(1, 1, 1, "rbf", False, 0.0, False),
	(15, 3, 3, "matern12", False, 0.0, False),
	(17, 4, 4, "matern32", True, 0.0, False),
	(65, 5, 64, "matern52", True, 0.0, True),
	(129, 17, 33, "matern32", False, 0.0, False),
	(257, 3, 16, "matern12", False, 1e4, True),
	(257, 8, 65, "rbf", False, 0.0, False),
] + [(1000, 3, 32, p, False, 0.0, False) for p in R.PROFILES]  # fmt: skip


def case_id(c) -> str:
	n, d, m, name, per_dim, offset, dup = c
	return f"n{n}-d{d}-m{m}-{name}" + ("-perdim" if per_dim else "") + ("-offset" if offset else "") + ("-dup" if dup else "")


def case_inputs(c, seed: int = 0):
	"""(X, ls, s, noise, Z, W) of a case: points uniform in [0, 1]^d (+ offset; duplicate rows: every 7th point repeats its
	predecessor), lengthscale 0.3 sqrt(d) or 0.3 sqrt(d) (1 + k / d) per dimension, normal Z and W."""
	n, d, m, name, per_dim, offset, dup = c
	X = R.points(n, d, seed=seed + d, offset=offset)
	if dup:
		X[6::7] = X[5:-1:7][: X[6::7].shape[0]]
	base = 0.3 * np.sqrt(d)
	ls = base * (1.0 + np.arange(d) / d) if per_dim else base
	rng = np.random.default_rng(3000 + seed + n)
	Z = np.asfortranarray(rng.standard_normal((n, m)))
	W = np.asfortranarray(rng.standard_normal((n, m)))
	return X, ls, 1.3, 0.1, Z, W


_CACHE: dict = {}


def case_model(c):
	"""(inputs, z, g, bar) of a case, computed once per session and shared; the arrays are not to be changed."""
	if c not in _CACHE:
		inp = case_inputs(c)
		X, ls, s, noise, Z, W = inp
		z = R.scaled_points(X, ls, np.float64)
		g, bar = model(z, c[3], ls, s, Z, W)
		_CACHE[c] = (inp, z, g, bar)
	return _CACHE[c]
