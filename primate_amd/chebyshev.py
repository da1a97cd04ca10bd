"""The kernel polynomial method (Weisse, Wellein, Alvermann, Fehske, Rev. Mod. Phys. 78, 2006; Lin, Saad, Yang, SIAM Review 2016):
traces v^T f(A) v and spectral densities from the Chebyshev moments mu_k = v^T T_k(A~) v, A~ = (A - c) / h, of a batch of
probes (engine.ChebyshevPlan: one update pass of the orth-0 Lanczos step per two moments, no orthogonality, no eigensolve,
no cap at 512 steps), and the action f(A) X ~= sum_k c_k T_k(A~) X of the same expansion: one fixed polynomial for every
column, so `ChebyshevFunction @ X` is exactly linear and symmetric (what hutchpp and xtrace assume), at any degree up to
16384 and in memory that does not depend on the degree.

What runs where: the recurrence, the moments, their sums against coefficients, the sum of the action and the density on a
grid are libslq kernels; the Chebyshev coefficients of f, the damping factors and the spectral bounds are small host
computations.
"""

from __future__ import annotations

from typing import Callable, Optional, Union

import numpy as np
from scipy.sparse.linalg import LinearOperator

from . import engine
from .lanczos import _as_device_operator
from .operators import is_linear_op

DAMPINGS = ("none", "jackson", "lanczos")
BOUNDS_METHODS = ("auto", "gershgorin", "lanczos")
## ChebyshevFunction with automatic bounds: an `outside` flag doubles the margin and runs again, this many times at most
BOUNDS_RETRIES = 3
## spectral_bounds(method="lanczos"): steps of the Lanczos run whose extreme Ritz values are taken
BOUNDS_LANCZOS_DEG = 30


def _check_bounds(bounds) -> tuple:
	try:
		a, b = (float(v) for v in bounds)
	except (TypeError, ValueError):
		raise ValueError(f"bounds must be a pair (a, b), got {bounds!r}") from None
	if not (np.isfinite(a) and np.isfinite(b) and a < b):
		raise ValueError(f"bounds must be finite with a < b, got {bounds!r}")
	return a, b


def _check_count(name: str, v, lo: int = 1) -> int:
	if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
		raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
	return int(v)


def damping_factors(kind: Optional[str], ncoef: int) -> np.ndarray:
	"""g_0 .. g_{ncoef-1} of the kernel polynomial method (Weisse et al. 2006, eqs. 71 and 78), g_0 = 1:
	"jackson": [(N - k + 1) cos(pi k / (N + 1)) + sin(pi k / (N + 1)) cot(pi / (N + 1))] / (N + 1), N = ncoef - the positive
	kernel (a damped density is >= 0);
	"lanczos": sigma factors sinc(k / N)^3; "none" / None: ones."""
	ncoef = _check_count("ncoef", ncoef)
	kind = "none" if kind is None else kind
	if kind not in DAMPINGS:
		raise ValueError(f"unknown damping '{kind}' (one of {', '.join(DAMPINGS)})")
	k = np.arange(ncoef, dtype=np.float64)
	if kind == "none":
		return np.ones(ncoef)
	if kind == "jackson":
		q = np.pi / (ncoef + 1)
		return ((ncoef - k + 1) * np.cos(q * k) + np.sin(q * k) / np.tan(q)) / (ncoef + 1)
	return np.sinc(k / ncoef) ** 3  # (np.sinc(x) = sin(pi x) / (pi x))


def _host_function(f, **kwargs) -> Callable:
	"""A built-in name (checked by engine.fun_spec, evaluated with the registry's defaults) or any callable."""
	if isinstance(f, str) or f is None:
		from .special import param_callable

		engine.fun_spec(f, **kwargs)
		return param_callable(f, **kwargs)
	if not callable(f):
		raise ValueError("f must be a built-in function name or a callable")
	return f


def chebyshev_coefficients(f, ncoef: int, bounds, damping: Optional[str] = "none", nquad: Optional[int] = None, **kwargs) -> np.ndarray:
	"""c_0 .. c_{ncoef-1} with f(x) ~= sum_k c_k T_k((x - c) / h) on [a, b] = bounds, by Chebyshev-Gauss quadrature on
	nquad >= ncoef nodes (a type-2 DCT; default 2 ncoef, and nquad = ncoef gives the interpolant of
	numpy.polynomial.chebyshev.chebinterpolate), multiplied by the damping factors. f: a built-in name (kwargs: its
	parameters, e.g. t=) or a callable on arrays. So that v^T f(A) v ~= sum_k c_k mu_k."""
	from scipy.fft import dct

	ncoef = _check_count("ncoef", ncoef)
	a, b = _check_bounds(bounds)
	g = damping_factors(damping, ncoef)
	nquad = 2 * ncoef if nquad is None else _check_count("nquad", nquad)
	if nquad < ncoef:
		raise ValueError(f"nquad = {nquad} < ncoef = {ncoef}")
	fun = _host_function(f, **kwargs)
	x = np.cos(np.pi * (np.arange(nquad) + 0.5) / nquad)
	fx = np.asarray(fun(0.5 * (a + b) + 0.5 * (b - a) * x), dtype=np.float64)
	if fx.shape != x.shape or not np.all(np.isfinite(fx)):
		raise ValueError("f must map an array of points inside the bounds to finite values of the same shape")
	c = dct(fx, type=2)[:ncoef] / nquad
	c[0] *= 0.5
	return c * g


def spectral_bounds(A, method: str = "auto", margin: float = 0.01, seed=None) -> tuple:
	"""(a, b) with the spectrum of the symmetric A inside.
	"gershgorin": the union of the Gershgorin discs of a sparse or dense matrix - guaranteed, and tight for Laplacians;
	"lanczos" (operators known by their product only): a short `lanczos()` run, the extreme Ritz values -/+ their residual
	norms, widened by `margin` of the width on each side - an estimate, which is why a ChebyshevFunction checks the
	`outside` flags of every run; "auto": gershgorin where A has entries, lanczos otherwise."""
	import scipy.sparse as sp

	if method not in BOUNDS_METHODS:
		raise ValueError(f"unknown method '{method}' (one of {', '.join(BOUNDS_METHODS)})")
	margin = float(margin)
	if not (np.isfinite(margin) and margin >= 0.0):
		raise ValueError(f"margin must be >= 0, got {margin!r}")
	if not is_linear_op(A):
		raise ValueError("A must be a square operator with a product")
	has_entries = sp.issparse(A) or isinstance(A, np.ndarray)
	if method == "auto":
		method = "gershgorin" if has_entries else "lanczos"
	if method == "gershgorin":
		if not has_entries:
			raise ValueError("Gershgorin discs need the entries of A (a SciPy sparse matrix or an ndarray): use method='lanczos'")
		if sp.issparse(A):
			M = sp.csr_matrix(A)
			d = np.asarray(M.diagonal(), dtype=np.float64)
			r = np.asarray(abs(M).sum(axis=1), dtype=np.float64).ravel() - np.abs(d)
		else:
			M = np.asarray(A, dtype=np.float64)
			d = np.diag(M).copy()
			r = np.abs(M).sum(axis=1) - np.abs(d)
		a, b = float(np.min(d - r)), float(np.max(d + r))
		pad = 0.0
	else:
		from scipy.linalg import eigh_tridiagonal

		from .lanczos import lanczos

		n = A.shape[0]
		deg = min(BOUNDS_LANCZOS_DEG, n)
		dt = np.dtype(getattr(A, "dtype", np.float64))
		alpha, beta = np.zeros(deg + 1, dtype=dt), np.zeros(deg + 1, dtype=dt)
		lanczos(A, deg=deg, orth=deg, seed=seed, alpha=alpha, beta=beta, dtype=dt)
		al, be = alpha[:deg].astype(np.float64), beta[1:deg].astype(np.float64)
		theta, Y = eigh_tridiagonal(al, be) if deg > 1 else (al.copy(), np.ones((1, 1)))
		res = abs(float(beta[deg])) * np.abs(Y[-1, :])  # ||A y - theta y|| of every Ritz pair
		a, b = float(theta[0] - res[0]), float(theta[-1] + res[-1])
		pad = margin
	w = b - a
	if not w > 0.0:  # (a multiple of the identity: any interval around the one eigenvalue)
		w = max(abs(a), 1.0)
		pad = max(pad, 0.01)
	return a - pad * w, b + pad * w


def _widen(raw: tuple, extra: float) -> tuple:
	w = raw[1] - raw[0]
	return raw[0] - extra * w, raw[1] + extra * w


def _steps_of(deg: int) -> int:
	return (int(deg) + 1) // 2  # ceil(deg / 2) steps give the moments 0 .. 2 ceil(deg / 2) >= deg


class ChebyshevFunction(LinearOperator):
	"""p(A), the degree-`deg` Chebyshev expansion of f on `bounds`, as a linear operator (the kernel polynomial method).
	`M @ x` / `M @ X` is sum_k c_k T_k(A~) X: `deg` steps of the recurrence in ONE run, the same polynomial for every column -
	exactly linear and symmetric, so `hutchpp(M)`, `xtrace(M)` and `diag(M)` work on it as on a matrix -, in device memory that
	does not depend on deg (the action: deg <= 16384); the columns go in batches of `batch`.
	`quad(x)` and `quad_generated(...)` as MatrixFunction has them, so `hutch(ChebyshevFunction(A, "log", deg=80))` estimates a
	trace with `trace.py` as it is: there ceil(deg / 2) steps run and the moments 0 .. deg are summed against the (damped)
	coefficients of f.
	fun: a built-in name (kwargs: its parameters) or a callable on arrays. bounds=None: `spectral_bounds(A)`; an `outside`
	flag then doubles the margin and runs again, BOUNDS_RETRIES times at most. With bounds given, the flag raises ValueError."""

	def __init__(self, A, fun: Union[str, Callable, None] = None, deg: int = 40, bounds: Optional[tuple] = None, damping: Optional[str] = "none",
				 dtype=np.float64, bounds_method: str = "auto", margin: float = 0.01, batch: int = 128, **kwargs):  # fmt: skip
		self._batch = _check_count("batch", batch)
		if not is_linear_op(A):
			raise ValueError("Invalid operator `A`; must be a square symmetric operator with a product")
		self._deg = _check_count("deg", deg)
		self._steps = _steps_of(self._deg)
		if self._steps > 16384:
			raise ValueError(f"deg = {deg} needs {self._steps} steps: at most 16384")
		damping_factors(damping, 1)  # (checks the name)
		self._fun = _host_function(fun, **kwargs)
		self._damping = damping
		self._given = None if bounds is None else _check_bounds(bounds)
		if bounds_method not in BOUNDS_METHODS:
			raise ValueError(f"unknown method '{bounds_method}' (one of {', '.join(BOUNDS_METHODS)})")
		self._margin = float(margin)
		if not (np.isfinite(self._margin) and self._margin > 0.0):
			raise ValueError(f"margin must be > 0, got {margin!r}")
		self.shape = A.shape
		self.dtype = np.dtype(dtype)
		self._A = A
		self._op = _as_device_operator(A, dtype=self.dtype)
		self._bounds_method = bounds_method
		self._raw = None     # automatic bounds before any widening
		self._extra = 0.0    # what the retries have added to them, as a fraction of their width
		self.bounds = self._given
		self._coef = None
		self._plans: dict = {}
		self._action_plans: dict = {}

	@property
	def degree(self) -> int:
		return self._deg

	def _adjoint(self):
		return self

	def _matvec(self, x):
		x = np.asarray(x)
		return self._matmat(x.reshape(-1, 1)).reshape(x.shape)

	def _matmat(self, X):
		"""p(A) X in batches of `batch` columns, every batch one run of deg steps (engine.ChebyshevPlan.action)."""
		X = np.asarray(X)
		if X.ndim != 2 or X.shape[0] != self.shape[1]:
			raise ValueError(f"dimension mismatch: {X.shape} against {self.shape}")
		Xd = X.astype(self.dtype, copy=False)
		Y = np.empty((self.shape[0], X.shape[1]), dtype=self.dtype, order="F")
		for c0 in range(0, X.shape[1], self._batch):
			Y[:, c0 : c0 + self._batch] = self._action(Xd[:, c0 : c0 + self._batch])
		return Y

	def _action_plan(self, nprobes: int) -> engine.ChebyshevPlan:
		if self._deg > 16384:
			raise ValueError(f"deg = {self._deg}: the action runs deg steps, at most 16384 (quad runs ceil(deg / 2))")
		if nprobes not in self._action_plans:
			for k in list(self._action_plans):  # (one cached action plan beside the cached quad plan)
				self._action_plans.pop(k).close()
			self._action_plans[nprobes] = engine.ChebyshevPlan(self._op, nprobes, self._deg, action=True)
		return self._action_plans[nprobes]

	def _action(self, X: np.ndarray) -> np.ndarray:
		"""The bounds logic of `_quad` around one action run."""
		plan = self._action_plan(X.shape[1])
		if self._coef is None:
			self._set_bounds()
		for attempt in range(BOUNDS_RETRIES + 1):
			plan.set_probes(X)
			try:
				return plan.action(self.bounds, self._coef)
			except ValueError:
				if plan.bounds != self.bounds:  # (refused before the run)
					raise
				_, flags = plan.moments(return_outside=True)
				if not flags.any():
					raise
				if self._given is not None:
					raise ValueError(f"the spectrum of A is not inside bounds = {self.bounds}: {int(flags.sum())} of {X.shape[1]} columns saw a moment above mu_0") from None
				if attempt == BOUNDS_RETRIES:
					raise ValueError(f"the spectrum of A is not inside the automatic bounds {self.bounds} after {BOUNDS_RETRIES} widenings: give bounds=") from None
				self._extra = max(2.0 * self._extra, 2.0 * self._margin)
				self._set_bounds()
		raise AssertionError("unreachable")

	def _set_bounds(self):
		if self._given is None:
			if self._raw is None:
				self._raw = spectral_bounds(self._A, self._bounds_method, self._margin)
			self.bounds = _widen(self._raw, self._extra)
		self._coef = chebyshev_coefficients(self._fun, self._deg + 1, self.bounds, self._damping)

	def _plan(self, nprobes: int) -> engine.ChebyshevPlan:
		if nprobes not in self._plans:
			for k in list(self._plans):  # (one cached plan: older ones are released to bound device memory)
				self._plans.pop(k).close()
			self._plans[nprobes] = engine.ChebyshevPlan(self._op, nprobes, self._steps)
		return self._plans[nprobes]

	def _quad(self, nprobes: int, load: Callable) -> np.ndarray:
		plan = self._plan(nprobes)
		if self._coef is None:
			self._set_bounds()
		for attempt in range(BOUNDS_RETRIES + 1):
			load(plan)
			plan.run(self.bounds)
			try:
				return plan.moment_sum(self._coef)
			except ValueError:
				_, flags = plan.moments(return_outside=True)
				if not flags.any():
					raise
				if self._given is not None:
					raise ValueError(f"the spectrum of A is not inside bounds = {self.bounds}: {int(flags.sum())} of {nprobes} probes saw a moment above mu_0") from None
				if attempt == BOUNDS_RETRIES:
					raise ValueError(f"the spectrum of A is not inside the automatic bounds {self.bounds} after {BOUNDS_RETRIES} widenings: give bounds=") from None
				self._extra = max(2.0 * self._extra, 2.0 * self._margin)
				self._set_bounds()
		raise AssertionError("unreachable")

	def quad(self, x: np.ndarray) -> np.ndarray:
		"""x^T f(A) x for every column of x."""
		x = np.asarray(x).astype(self.dtype, copy=False)
		x = np.atleast_2d(x).T if x.ndim == 1 else x
		return self._quad(x.shape[1], lambda plan: plan.set_probes(x))

	def quad_generated(self, nprobes: int, pdf: str = "rademacher", seed: int = 0, probe_offset: int = 0) -> np.ndarray:
		"""v_i^T f(A) v_i for `nprobes` probes drawn on the device (Philox probe ids probe_offset ..)."""
		return self._quad(int(nprobes), lambda plan: plan.generate_probes(pdf, seed=int(seed), probe_offset=int(probe_offset)))

	def close(self):
		for k in list(self._plans):
			self._plans.pop(k).close()
		for k in list(self._action_plans):
			self._action_plans.pop(k).close()


def _probe_stream(pdf: str, seed, n: int, dtype):
	"""load(plan, done, m): probe ids [done, done + m) of the stream (pdf, seed) into `plan` - host draws are the columns
	`hutch` draws for the same seed, "device:<name>" the Philox ids on the GPU. Raises ValueError for an unknown pdf."""
	from ._capi import PDF_IDS
	from .random import _ISO_DISTRIBUTIONS, isotropic

	if not isinstance(pdf, str):
		raise ValueError("pdf must be a distribution name or 'device:<name>'")
	dev = pdf.startswith("device:")
	name = pdf[len("device:"):] if dev else pdf
	if name not in (PDF_IDS if dev else _ISO_DISTRIBUTIONS):
		raise ValueError(f"Invalid distribution '{pdf}' supplied.")
	rng = np.random.default_rng(seed)
	if dev:
		dev_seed = int(seed) if isinstance(seed, (int, np.integer)) else int(rng.integers(0, 2**62))
		return lambda plan, done, m: plan.generate_probes(name, seed=dev_seed, probe_offset=done)
	draw = isotropic(pdf=pdf, seed=rng)
	return lambda plan, done, m: plan.set_probes(draw(size=(n, m)).astype(dtype, copy=False))


def _moment_args(A, deg, bounds, nprobes, batch) -> tuple:
	if not is_linear_op(A):
		raise ValueError("A must be a square symmetric operator with a product")
	deg = _check_count("deg", deg)
	if _steps_of(deg) > 16384:
		raise ValueError(f"deg = {deg} needs {_steps_of(deg)} steps: at most 16384")
	return deg, (None if bounds is None else _check_bounds(bounds)), _check_count("nprobes", nprobes), _check_count("batch", batch)


def chebyshev_moments(A, deg: int, bounds: Optional[tuple] = None, nprobes: int = 256, batch: int = 256, pdf: str = "rademacher", seed=None,
					  dtype=np.float64) -> tuple:  # fmt: skip
	"""(mu, bounds): mu[i, k] = v_i^T T_k(A~) v_i for k = 0 .. deg and `nprobes` probes of the stream (pdf, seed), in lock-step
	batches of `batch`; bounds=None: `spectral_bounds(A)`. ValueError if the bounds miss part of the spectrum."""
	deg, bounds, nprobes, batch = _moment_args(A, deg, bounds, nprobes, batch)
	load = _probe_stream(pdf, seed, A.shape[0], np.dtype(dtype))
	bounds = spectral_bounds(A) if bounds is None else bounds
	op = _as_device_operator(A, dtype=np.dtype(dtype))
	out, plans = np.zeros((nprobes, deg + 1)), {}
	try:
		done = 0
		while done < nprobes:
			m = min(batch, nprobes - done)
			if m not in plans:
				plans[m] = engine.ChebyshevPlan(op, m, _steps_of(deg))
			load(plans[m], done, m)
			plans[m].run(bounds)
			mu, flags = plans[m].moments(return_outside=True)
			if flags.any():
				raise ValueError(f"the spectrum of A is not inside bounds = {bounds}: {int(flags.sum())} of {m} probes saw a moment above mu_0")
			out[done : done + m] = mu[:, : deg + 1]
			done += m
	finally:
		for pl in plans.values():
			pl.close()
	return out, bounds


def density_grid(bins: int, a: float, b: float) -> np.ndarray:
	"""`bins` points strictly inside (a, b): the midpoints of `bins` equal cells (the density has 1 / sqrt(1 - x~^2) at the ends)."""
	return a + (np.arange(bins) + 0.5) * ((b - a) / bins)


def kpm_density(A, bins: int, interval: Optional[tuple], deg: int, damping: Optional[str], nprobes: int, batch: int, pdf: str, seed, dtype=np.float64) -> tuple:
	"""What integrate.spectral_density(method="kpm") runs: (mean, M2, outside, count, grid, bounds). interval=None: the
	spectral bounds, sampled at the midpoints of `bins` cells; an interval given: `bins` points from end to end of it, inside
	bounds that contain both it and the spectrum."""
	deg, interval, nprobes, batch = _moment_args(A, deg, interval, nprobes, batch)
	bins = _check_count("bins", bins)
	g = damping_factors(damping, deg + 1)
	load = _probe_stream(pdf, seed, A.shape[0], np.dtype(dtype))
	sb = spectral_bounds(A)
	if interval is None:
		bounds, grid = sb, density_grid(bins, *sb)
	else:
		pad = 1e-6 * (interval[1] - interval[0])
		bounds, grid = (min(sb[0], interval[0] - pad), max(sb[1], interval[1] + pad)), np.linspace(interval[0], interval[1], bins)
	op = _as_device_operator(A, dtype=np.dtype(dtype))
	acc, plans = engine.DensityAccumulator("chebyshev", grid, ctx=op.ctx), {}
	try:
		done = 0
		while done < nprobes:
			m = min(batch, nprobes - done)
			if m not in plans:
				plans[m] = engine.ChebyshevPlan(op, m, _steps_of(deg))
			load(plans[m], done, m)
			plans[m].run(bounds)
			acc.update(plans[m], damping=g, nweights=deg + 1)
			done += m
		mean, m2, outside, cnt = acc.get()
	finally:
		acc.close()
		for pl in plans.values():
			pl.close()
	return mean, m2, outside, cnt, grid, bounds
