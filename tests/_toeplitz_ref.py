"""The model of the Toeplitz operator's tests: the exact product in np.longdouble from the ROUNDED c and r, the error
bar of a product, the check that the bar is a small fraction of the result, and the case list the CPU and the GPU test share.

The bar, for output column k in the complex pair q = k // 2 (columns 2q and 2q+1 travel through the transforms as one complex column):

    |got[:, k] - Y[:, k]|_2  <=  eps log2(L) |t|_1 |[x_2q, x_2q+1]|_2,      |t|_1 = sum|c| + sum|r[1:]|,  eps = 2^-53 / 2^-24.

The worst-case theory for two transforms and the symbol gives about 16 x this (Higham, Accuracy and Stability, Thm 24.2); pocketfft at the
operator's dtype attains 0.05 - 0.33 of it on the inputs below, so the bar admits a hand-written transform about 3 x pocketfft's worst case
and rejects anything systematically worse than rounding."""

import ctypes as C
import functools

import numpy as np

LD = np.longdouble
DENSE_MAX = 8192
BS = (1, 2, 3, 16, 17, 33)
## two panels (NP = 2: the panel loop, the column offset of the mask, the reuse of the one workspace), an odd count in the second panel
BS_TWO_PANELS = {np.float64: 131, np.float32: 259}


def eps_of(dtype) -> float:
	return 2.0**-53 if np.dtype(dtype) == np.float64 else 2.0**-24


def values(n: int, symmetric: bool, dtype, rho: float = 0.5):
	"""c = rho^k (the Kac-Murdock-Szego matrix, spectrum in [(1-rho)/(1+rho), (1+rho)/(1-rho)]), r = c or 0.3^k; as rounded to dtype."""
	k = np.arange(n, dtype=np.float64)
	c = (rho**k).astype(dtype)
	r = c.copy() if symmetric else (0.3**k).astype(dtype)
	r[0] = c[0]
	return c, r


def plan(n: int, dtype, pw: int = 0) -> dict:
	"""slq_debug_toeplitz_plan (no device)."""
	from primate_amd import _capi

	out = (C.c_int64 * 10)()
	dt = np.dtype(dtype)
	pw = pw or (16 if dt == np.float64 else 32)
	_capi.check(_capi.lib().slq_debug_toeplitz_plan(n, _capi.dtype_id(dt), pw, out, 10))
	v = [int(x) for x in out]
	return {"L": v[0], "levels": v[1], "lengths": v[2:5], "lds": v[5], "cg": v[6], "ws": v[7], "launches": v[8], "max_n": v[9]}


@functools.lru_cache(maxsize=None)
def structure_sizes() -> tuple:
	"""(largest n of the one-kernel path, the smallest n of every further pass structure), from the debug entry."""
	max_n = plan(1, np.float64)["max_n"]
	## (L changes only between n = 2^k and 2^k + 1: scan those)
	first = {}
	k = 0
	while (1 << k) <= max_n:
		for n in ((1 << k), (1 << k) + 1):
			if n <= max_n:
				first.setdefault(plan(n, np.float64)["levels"], n)
		k += 1
	single_max = first[2] - 1 if 2 in first else max_n
	return single_max, tuple(first[lv] for lv in sorted(first) if lv > 1)


def sizes() -> tuple:
	single_max, further = structure_sizes()
	return tuple(sorted(set((1, 2, 3, 17, 64, 1000, single_max) + further)))


def inputs(n: int, b: int, dtype, seed: int = 0) -> np.ndarray:
	"""n x b, column-major. n <= DENSE_MAX: Rademacher signs, the probes the estimators draw (with standard normals the host path itself
	reaches 0.85 of the bar in one column of the n = 2, b = 33, fp32, non-symmetric case - at L = 4 the bar is two roundings wide - and
	the condition of test_toeplitz_cpu.py, host path <= half the bar, would not hold on the whole list). Above: at most 64 nonzero rows per column - unit vectors at 0, n-1 and the
	middle, a prefix of 64 ones, 64 random rows - so that the model stays O(64 n) per column."""
	rng = np.random.default_rng(1000 * seed + n % 997 + b)
	if n <= DENSE_MAX:
		return np.asfortranarray((2.0 * rng.integers(0, 2, (n, b)) - 1.0).astype(dtype))
	X = np.zeros((n, b), dtype=dtype, order="F")
	for k in range(b):
		kind = k % 5
		if kind < 3:
			X[(0, n - 1, n // 2)[kind], k] = 1.0 + k
		elif kind == 3:
			X[:64, k] = 1.0
		else:
			X[rng.choice(n, 64, replace=False), k] = rng.standard_normal(64).astype(dtype)
	return X


def model(c, r, X) -> np.ndarray:
	"""The exact product in long double, from the rounded c and r."""
	n = c.size
	cl, rl, Xl = c.astype(LD), r.astype(LD), X.astype(LD)
	if n <= DENSE_MAX:
		i, j = np.indices((n, n))
		A = np.where(i >= j, cl[np.abs(i - j)], rl[np.abs(i - j)])
		return A @ Xl
	Y = np.zeros(X.shape, dtype=LD)
	kc, kr = (int(np.flatnonzero(v)[-1]) + 1 if np.any(v) else 1 for v in (c, r))  # (entries behind them are exact zeros: skipped, which is exact)
	for k in range(X.shape[1]):
		for j in np.flatnonzero(X[:, k]):
			lo, hi = max(0, j - kr + 1), min(n, j + kc)
			Y[lo:hi, k] += Xl[j, k] * np.concatenate((rl[j - lo : 0 : -1], cl[: hi - j]))  # column j of A, rows lo .. hi - 1
	return Y


def bar(c, r, X, dtype) -> np.ndarray:
	"""Per column: eps log2(L) |t|_1 |pair|_2 (long double)."""
	n, b = X.shape
	L = plan(n, dtype)["L"]
	t1 = np.sum(np.abs(c.astype(LD))) + np.sum(np.abs(r[1:].astype(LD)))
	Xl = X.astype(LD)
	n2 = np.sum(Xl * Xl, axis=0)
	pair = np.array([np.sqrt(n2[2 * (k // 2) : 2 * (k // 2) + 2].sum()) for k in range(b)], dtype=LD)
	return LD(eps_of(dtype)) * LD(np.log2(L)) * t1 * pair


def ratios(got, Y, bars) -> np.ndarray:
	err = np.sqrt(np.sum((got.astype(LD) - Y) ** 2, axis=0))
	return (err / bars).astype(np.float64)


def check_condition(Y, bars, dtype) -> float:
	"""The bar must be a small fraction of the result (<= 1e-3 in fp32, 1e-11 in fp64, per column), or passing it proves nothing."""
	yn = np.sqrt(np.sum(Y * Y, axis=0))
	frac = float(np.max(bars / yn))
	assert frac <= (1e-11 if np.dtype(dtype) == np.float64 else 1e-3), f"the bar is {frac:.3g} of the result"
	return frac


def host_path(c, r, X, dtype) -> np.ndarray:
	"""scipy.fft at the operator's dtype with the device's pairing: probes 2q and 2q+1 as one complex column (four complex columns at a
	time: the transforms of a large L stay small in memory)."""
	import scipy.fft as sf

	n, b = X.shape
	cd = np.complex128 if np.dtype(dtype) == np.float64 else np.complex64
	L = plan(n, dtype)["L"]
	e = np.zeros(L)
	e[:n] = c
	e[L - n + 1 :] = r[:0:-1]
	sym = sf.fft(e).astype(cd)
	out = np.empty((n, b), dtype=dtype)
	for q0 in range(0, (b + 1) // 2, 4):
		cols = range(2 * q0, min(b, 2 * q0 + 8))
		Xp = np.zeros((L, (len(cols) + 1) // 2), dtype=cd)
		Xp[:n].real = X[:, cols[0::2]]
		Xp[:n, : len(cols) // 2].imag = X[:, cols[1::2]]
		Z = sf.ifft(sym[:, None] * sf.fft(Xp, axis=0, workers=4), axis=0, workers=4)[:n]
		assert Z.dtype == cd
		out[:, cols[0::2]] = Z.real
		out[:, cols[1::2]] = Z.imag[:, : len(cols) // 2]
	return out


def two_panel_cases() -> list:
	n = structure_sizes()[1][0]
	return [(n, BS_TWO_PANELS[dtype], False, dtype) for dtype in (np.float64, np.float32)]


def cases() -> list:
	"""(n, b, symmetric, dtype) of every product the GPU test runs."""
	out = []
	for n in sizes():
		for b in BS:
			for symmetric in (True, False):
				for dtype in (np.float64, np.float32):
					out.append((n, b, symmetric, dtype))
	return out + two_panel_cases()


def _case_data(n: int, b: int, symmetric: bool, dtype):
	c, r = values(n, symmetric, dtype)
	X = inputs(n, b, dtype)
	Y = model(c, r, X)
	return c, r, X, Y, bar(c, r, X, dtype)


_cached_case_data = functools.lru_cache(maxsize=None)(_case_data)


def case_data(n: int, b: int, symmetric: bool, dtype):
	"""c, r, X, the model and the bars of a case: computed once and shared for n <= DENSE_MAX (a few MB in all), computed anew above (a
	case there is hundreds of MB in long double, and cheap: the model walks the nonzero band of c and r only)."""
	return (_cached_case_data if n <= DENSE_MAX else _case_data)(n, b, symmetric, dtype)
