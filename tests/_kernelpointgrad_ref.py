"""The model of the point-gradient tests and its bar.

On the ROUNDED z of the operator (`_kernelop_ref.scaled_points`; the new points z* by `_kernelcross_ref.scaled_new_points`), with
chi = -2 dphi/dr2 (`_kernelgrad_ref.chi`: matern12 is 0 where r2 = 0) and r2 = sum_k D^2 from differences in long double:

    training form   P[a,k] = -(s / l_k) sum_j (C_aj + C_ja) chi(r2_aj) (z_ak - z_jk),        C = Z W^T          n x d
    cross form      R[a,k] = -(s / l_k) sum_j  C_aj         chi(r2(z*_a, z_j)) (z*_ak - z_jk), C = U W^T          m x d

The bar is a forward bound, elementwise. eps = 2^-53, |C| = |Z||W|^T (+ |W||Z|^T); dr2, C_EXP, lo = max(r2 - dr2, 0), hi = r2 + dr2 and
dchi = |chi(lo) - chi(hi)| (matern12 where lo = 0: chi(r2) + chi(hi)) as in `_kernelgrad_ref`; dchi = 0 on the training diagonal;
S = (n_sum + 80) eps, m the number of factor columns, Delta_k = z_ak - z_jk:

    bar[a,k] = (s / l_k) [ sum_j |C| dchi |Delta_k| + ((m + 5 + C_EXP) eps + S) sum_j |C| chi |Delta_k|
                           + 2 eps sum_j |C| chi (|z_ak| + |z_jk|) ] + 2 eps |P[a,k]|

in order: r2's error through the monotone profile; the m-term dot and the profile's arithmetic; any summation order in which no term
passes through more than n_sum + 80 additions; an expanded evaluation of the difference (granted whether used or not); the final scale.
"""

import numpy as np

import _kernelgrad_ref as G
import _kernelop_ref as R

LD = np.longdouble
EPS = G.EPS
C_EXP = G.C_EXP
CONDITION = 1e-6


def _r2(za, zb):
	out = np.zeros((za.shape[0], zb.shape[0]), dtype=LD)
	for k in range(za.shape[1]):
		diff = za[:, k][:, None] - zb[None, :, k]
		out += diff * diff
	return out


def model(z: np.ndarray, name: str, ls, s: float, Z: np.ndarray, W: np.ndarray, znew=None, flip=None, one_sided: bool = False):
	"""(P, bar), long double. znew None: the training form on the rounded points z (n x d) with factors Z, W (n x m): n x d. znew (m* x d,
	rounded): the cross form with Z = U (m* x b) on the new points and W (n x b): m* x d. Two faults for the tests of the bar, not
	features: flip = (a, j, k): that one difference enters as z_ak + z_jk; one_sided: the training form without its C_ja term."""
	n, d = z.shape
	cross = znew is not None
	ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (d,)).astype(LD)
	zs = z.astype(LD)
	zr = znew.astype(LD) if cross else zs
	rows = zr.shape[0]
	## (float64 factors as the device holds them; a long-double factor - a dense inverse as Z against W = I - is taken as it is)
	Zl, Wl = (np.asarray(F, dtype=LD if np.asarray(F).dtype == LD else np.float64).reshape(r, -1).astype(LD) for F, r in ((Z, rows), (W, n)))
	m = Zl.shape[1]
	nr, ns = np.sqrt(np.sum(zr * zr, axis=1)), np.sqrt(np.sum(zs * zs, axis=1))
	S = LD(n + 80) * EPS
	P, bar = np.zeros((rows, d), dtype=LD), np.zeros((rows, d), dtype=LD)
	for i0, i1 in G._blocks(rows):
		idx = np.arange(i0, i1)
		r2 = _r2(zr[idx], zs)
		Cm, Ca = Zl[idx] @ Wl.T, np.abs(Zl[idx]) @ np.abs(Wl).T
		if not cross and not one_sided:
			Cm, Ca = Cm + Wl[idx] @ Zl.T, Ca + np.abs(Wl[idx]) @ np.abs(Zl).T
		dr2 = LD(d + 3) * EPS * (nr[idx][:, None] + ns[None, :]) ** 2
		lo, hi = np.maximum(r2 - dr2, LD(0)), r2 + dr2
		ch = G.chi(name, r2)
		dch = np.abs(G.chi(name, lo) - G.chi(name, hi))
		if name == "matern12":
			dch = np.where(lo == 0, ch + G.chi(name, hi), dch)
		if not cross:
			dch[np.arange(idx.size), idx] = 0
		for k in range(d):
			D = zr[idx, k][:, None] - zs[None, :, k]
			if flip is not None and flip[2] == k and i0 <= flip[0] < i1:
				D[flip[0] - i0, flip[1]] = zr[flip[0], k] + zs[flip[1], k]
			aD = np.abs(D)
			raw = np.sum(Cm * ch * D, axis=1)
			t1, t2 = np.sum(Ca * dch * aD, axis=1), np.sum(Ca * ch * aD, axis=1)
			t3 = np.sum(Ca * ch * (np.abs(zr[idx, k])[:, None] + np.abs(zs[None, :, k])), axis=1)
			P[idx, k] = -(LD(s) / ls[k]) * raw
			bar[idx, k] = LD(s) / ls[k] * (t1 + (LD(m + 5) * EPS + C_EXP * EPS + S) * t2 + LD(2) * EPS * t3) + LD(2) * EPS * np.abs(P[idx, k])
	return P, bar


def emulate(z: np.ndarray, name: str, ls, s: float, Z: np.ndarray, W: np.ndarray, znew=None, jmax=None, expanded: bool = False) -> np.ndarray:
	"""The device evaluation in float64 NumPy: norms plus dot for r2 (clamped; 0 on the training diagonal), DIFFERENCES for the
	coordinate term. jmax: only the summed points j < jmax enter (a dropped remainder tile, for the tests of the bar). expanded: the
	coordinate term as rowsum(B) z_a - B z_J instead (what the kernel must not do: it cancels where chi is huge)."""
	n, d = z.shape
	cross = znew is not None
	zr = znew if cross else z
	rows = zr.shape[0]
	ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (d,))
	Z, W = np.asarray(Z, dtype=np.float64).reshape(rows, -1), np.asarray(W, dtype=np.float64).reshape(n, -1)
	nr, ns = np.sum(zr * zr, axis=1), np.sum(z * z, axis=1)
	r2 = np.maximum(nr[:, None] + ns[None, :] - 2.0 * (zr @ z.T), 0.0)
	if not cross:
		np.fill_diagonal(r2, 0.0)
	ch = G.chi(name, r2)
	passes = [(Z, W)] if cross else [(Z, W), (W, Z)]
	out = np.zeros((rows, d))
	for U, V in passes:
		if jmax is not None:
			V = V.copy()
			V[jmax:] = 0.0
		B = (U @ V.T) * ch
		for k in range(d):
			if expanded:
				v = B.sum(axis=1) * zr[:, k] - B @ z[:, k]
			else:
				v = np.sum(B * (zr[:, k][:, None] - z[None, :, k]), axis=1)
			out[:, k] += -(s / ls[k]) * v
	return out


def check_condition(P, bar) -> float:
	"""The condition of every case: max bar <= 1e-6 max |P|, or passing the bar says nothing. Returns the ratio (0 where P is exactly 0:
	one point)."""
	top, b = float(np.max(np.abs(P))), float(np.max(bar))
	assert b <= CONDITION * top, f"the bar {b:.3e} is above {CONDITION:g} of max |P| = {top:.3e}: the case does not discriminate"
	return b / top if top > 0 else 0.0


def worst(got, P, bar) -> float:
	"""max |got - P| / bar over the elements; where the bar is 0 (an exactly known value) equality is asked: 0, else inf."""
	err = np.abs(np.asarray(got).astype(LD) - P)
	ratio = np.where(bar > 0, err / np.where(bar > 0, bar, LD(1)), np.where(err == 0, LD(0), LD(np.inf)))
	return float(np.max(ratio))


_CACHE: dict = {}


def case_model(c):
	"""(inputs, z, P, bar) of a case of `_kernelgrad_ref.GPU_CASES` with its inputs, computed once per session and shared; the arrays are
	not to be changed."""
	if c not in _CACHE:
		inp = G.case_inputs(c)
		X, ls, s, noise, Z, W = inp
		z = R.scaled_points(X, ls, np.float64)
		P, bar = model(z, c[3], ls, s, Z, W)
		_CACHE[c] = (inp, z, P, bar)
	return _CACHE[c]


## ---- the cross cases of the GPU tests: (m new points, n, d, b columns, profile) -------------------------------------------------
CROSS_CASES = [(1, 1, 1, 1, "rbf"), (5, 40, 3, 2, "matern12"), (130, 257, 17, 65, "matern32"), (1000, 33, 3, 16, "matern52"), (33, 1000, 2, 64, "matern12")]


def cross_id(c) -> str:
	return f"m{c[0]}-n{c[1]}-d{c[2]}-b{c[3]}-{c[4]}"


def cross_inputs(c, seed: int = 0):
	"""(X, Xnew, ls, s, noise, U, W, copies): points uniform in [0, 1]^d, lengthscale 0.3 sqrt(d); every 4th new point (from the first) is
	a bitwise copy of a training point - `copies` lists those rows (none where there is one new point: its gradient would be 0)."""
	m, n, d, b, name = c
	X, Xn = R.points(n, d, seed=seed + d), R.points(m, d, seed=seed + 50 + d)
	copies = np.arange(0, m if m > 1 else 0, 4)
	Xn[copies] = X[copies % n]
	rng = np.random.default_rng(4000 + seed + n + m)
	U = np.asfortranarray(rng.standard_normal((m, b)))
	W = np.asfortranarray(rng.standard_normal((n, b)))
	return X, Xn, 0.3 * np.sqrt(d), 1.3, 0.1, U, W, copies


def cross_model(c):
	"""(inputs, z, z*, R, bar) of a cross case, computed once per session and shared."""
	import _kernelcross_ref as X_

	if c not in _CACHE:
		inp = cross_inputs(c)
		X, Xn, ls, s, noise, U, W, copies = inp
		z, zn = R.scaled_points(X, ls, np.float64), X_.scaled_new_points(X, Xn, ls, np.float64)
		P, bar = model(z, c[4], ls, s, U, W, znew=zn)
		_CACHE[c] = (inp, z, zn, P, bar)
	return _CACHE[c]
