"""`MatrixFunction`: the SLQ operator x -> f(A) x / x^T f(A) x with the reference's interface
(src/primate/operators.py:36-161), evaluated by libslq on the MI355X.

What changes under the hood:
  * `.quad(X)` advances ALL columns of X in lock-step in one device run (the reference loops over
    columns in Python and crosses its FFI once per probe, operators.py:145-150);
  * the operator is uploaded once and stays resident (the reference copies it >= 3 times per probe,
    SURVEY.md §8a a6);
  * built-in spectral functions are reduced on the device; Python callables are applied on the
    host to the (P, deg) nodes.
"""

from __future__ import annotations

from typing import Any, Callable, Optional, Union

import numpy as np
from scipy.sparse.linalg import LinearOperator

from . import engine
from .lanczos import _as_device_operator
from .special import builtin_spec, param_callable

F64: np.dtype = np.dtype("float64")


def _has_product(A: Any) -> bool:
	return any(hasattr(A, a) for a in ("__matmul__", "matmul", "dot", "matvec"))


def is_valid_operator(A: Union[np.ndarray, LinearOperator]) -> np.dtype:
	"""Checks of operators.py:15-23; returns the floating dtype."""
	assert _has_product(A), "Invalid operator; must have an overloaded 'matvec' or 'matmul' method"
	assert hasattr(A, "shape") and len(A.shape) >= 2, "Operator must be at least two dimensional."
	assert A.shape[0] == A.shape[1], "This function only works with square, symmetric matrices!"
	f_dtype = (A @ np.zeros(A.shape[1])).dtype if not hasattr(A, "dtype") else A.dtype
	assert np.dtype(f_dtype).type in {np.float32, np.float64}, "Only 32- or 64-bit floats are supported."
	return np.dtype(f_dtype)


def is_linear_op(A: Any) -> bool:
	"""operators.py:26-33."""
	return bool(_has_product(A) and hasattr(A, "shape") and len(A.shape) >= 2 and A.shape[0] == A.shape[1])


class MatrixFunction(LinearOperator):
	"""Linear operator approximating f(A) by degree-`deg` Lanczos (operators.py:36-151).

	Parameters match the reference: A (ndarray / sparse / LinearOperator), fun (name or callable),
	deg, orth (number of most recent Lanczos vectors to re-orthogonalise against; <0 or >deg means
	deg), dtype, and **kwargs for the named function (e.g. t=, a=, b=, threshold=).

	stale_ring (extra, default False): reproduce the reference's `quad` bit of history — it never
	clears its Lanczos ring `_Q` between probes (operators.py:138-148), so with orth > 0 probe j's
	first orth-1 reorthogonalisation sweeps also project against probe j-1's last Lanczos vectors.
	True runs `quad` one probe at a time through the single-vector drop-in entry with a persistent
	ring, exactly like the reference (and as slowly: one device run per probe). The default False is
	the lock-step batched path, which starts every probe from a clean ring — what the reference's own
	`_matvec` enforces (operators.py:116) and what its first probe always sees.

	Adaptive degree (extra; `deg_max=None`, the default, changes nothing): with `deg_max`, `quad` / `quad_generated` -
	and so `hutch(M)` - run a resumable Lanczos run of capacity deg_max in stages deg, deg + deg_step, ... (deg_step
	defaults to engine.DEG_STEP) and stop at the first stage that meets `deg_rtol` (required: it has no default), by the
	change of the batch sum between stages or, with `endpoint` <= lambda_min(A), by the width of the Gauss / Gauss-Radau
	bracket (engine.quad_adaptive). The values are those of a fixed deg = `M.deg_used` run; `M.deg_used` and
	`M.quad_bounds` (per-probe (lower, upper) of the bracket, None without endpoint) record the last call, `M.deg_history`
	its stages and their statistics. Built-in
	function names only. `_matvec` (f(A) v), `diag`, `xtrace`, `hutchpp` and `spectral_density` keep the fixed `deg`, and
	the `distributed` entries refuse an adaptive MatrixFunction: a degree chosen per rank would make the result depend on
	the sharding.

	`basis` (extra, default "keep": nothing changes): what the f(A)v action - `_matvec` / `_matmat`, and through them `diag`,
	`xdiag`, `xtrace`, `hutchpp` - runs on. "keep" retains the deg + 1 Lanczos panels; "recompute" is two-pass Lanczos
	(engine.LanczosPlan): a footprint independent of deg for one more run per action; "auto" takes the kept basis when its
	plan for the requested column count fits the free device memory (its bytes + 1 GiB) and recompute otherwise.
	`M.basis_used` records what the last action ran on. A Python callable `fun` needs the basis on the host: "keep" (and
	"auto", which then means "keep") only.
	"""

	def __init__(
		self, A, fun: Union[str, Callable, None] = None, deg: int = 20, orth: int = 3, dtype: np.dtype = F64,
		stale_ring: bool = False, deg_max: Optional[int] = None, deg_rtol: Optional[float] = None, deg_step: Optional[int] = None,
		endpoint: Optional[float] = None, basis: str = "keep", **kwargs,
	) -> None:  # fmt: skip
		assert is_linear_op(A), "Invalid operator `A`; must be dim=2 symmetric operator with defined matvec"
		assert deg >= 2, "Degree must be >= 2"
		self._basis = engine._basis_arg(False, basis, auto=True)
		if self._basis is None:
			raise ValueError("basis must be 'keep', 'recompute' or 'auto'")
		if self._basis == "recompute" and fun is not None and not isinstance(fun, str):
			raise ValueError("a callable `fun` combines the Lanczos basis on the host: basis='recompute' takes built-in function names")
		self.basis_used = None
		self._adaptive = None
		self.deg_used, self.quad_bounds, self.deg_history = None, None, None
		if deg_max is not None:
			if stale_ring:
				raise ValueError("an adaptive degree needs the clean ring of the batched path (stale_ring=False)")
			if not isinstance(fun, str):
				raise ValueError("an adaptive degree takes built-in function names (the stage statistics are reduced on the device)")
			n_cap = min(int(deg_max), A.shape[0]) if isinstance(deg_max, (int, np.integer)) and not isinstance(deg_max, bool) else deg_max
			dm, stages, rt, ep = engine._adaptive_args(n_cap, None, deg_rtol, endpoint, deg_step, first=min(deg, A.shape[0]))
			self._adaptive = dict(deg_max=dm, stages=stages, deg_rtol=rt, endpoint=ep)
		elif deg_rtol is not None or deg_step is not None or endpoint is not None:
			raise ValueError("deg_rtol, deg_step and endpoint belong to an adaptive degree: give deg_max")
		self.shape = A.shape
		self.dtype = np.dtype(dtype)
		fun = (lambda x: x) if fun is None else fun
		self._builtin = builtin_spec(fun, **kwargs) if isinstance(fun, str) else None
		self.fun = param_callable(fun, **kwargs) if isinstance(fun, str) else fun
		self._deg = min(deg, A.shape[0])
		self._rtol = 1e-8
		self._orth = self._deg if orth < 0 or orth > self._deg else orth
		self._orth_given = orth  # (the adaptive plan has capacity deg_max: out-of-range means ITS deg)
		self._A = A
		self._op = _as_device_operator(A, dtype=self.dtype)
		self._plans: dict = {}
		self._stale_ring = bool(stale_ring)
		if self._stale_ring:  # the reference's persistent buffers (operators.py:69-77)
			self._alpha = np.zeros(self._deg + 1, dtype=self.dtype)
			self._beta = np.zeros(self._deg + 1, dtype=self.dtype)
			self._Q = np.zeros((A.shape[0], self._deg), dtype=self.dtype, order="F")
		self._nodes = np.zeros(self._deg, dtype=self.dtype)
		self._weights = np.zeros(self._deg, dtype=self.dtype)

	@property
	def degree(self) -> int:
		return self._deg

	@property
	def fun(self) -> Callable:
		return self._fun

	@fun.setter
	def fun(self, value: Callable) -> None:
		assert callable(value), "Function must be callable."
		out = value(np.ones(self.shape[1]))
		assert isinstance(out, np.ndarray), "Function must return array-like"
		assert out.shape[-1] == self.shape[0], "Last dimension of output must match number of rows."
		self._fun = value
		spec = getattr(value, "_slq_builtin", None)
		if spec is not None:
			self._builtin = spec
		elif getattr(self, "_fun_initialised", False):
			self._builtin = None
		self._fun_initialised = True

	def _adjoint(self):
		return self

	def _action_basis(self, nprobes: int) -> str:
		"""The plan kind an action over `nprobes` columns runs on: the mode given, "auto" resolved by the memory rule of
		slq_fAv_batch_mode (a callable `fun` needs the basis on the host: "keep")."""
		basis = getattr(self, "_basis", "keep")
		if basis != "auto":
			return basis
		if self._builtin is None:
			return "keep"
		for k, plan in self._plans.items():  # (a plan this size already exists: it fits)
			if k[0] == nprobes and k[1] in ("keep", "recompute") and not k[2]:
				return k[1]
		for k in [k for k in self._plans if k[1] in ("keep", "recompute")]:  # (their memory is free for the choice)
			self._plans.pop(k).close()
		need = engine.plan_query_bytes(self.dtype, self.shape[0], nprobes, self._deg, self._orth, "keep")
		free, _ = self._op.ctx.meminfo()
		return "keep" if need + (1 << 30) <= free else "recompute"

	def _plan(self, nprobes: int, keep_basis: bool, adaptive: bool = False) -> engine.LanczosPlan:
		kind = self._action_basis(nprobes) if keep_basis else False
		key = (nprobes, kind, adaptive)
		if keep_basis:
			self.basis_used = kind
		if key not in self._plans:
			## one cached plan per shape class; older ones are released to bound device memory
			for k in [k for k in self._plans if bool(k[1]) == bool(kind) and k[2] == adaptive]:
				self._plans.pop(k).close()
			deg = self._adaptive["deg_max"] if adaptive else self._deg
			self._plans[key] = engine.LanczosPlan(self._op, nprobes, deg, self._orth_given if adaptive else self._orth, basis=kind or None)
		return self._plans[key]

	def _quad_adaptive(self, X, nprobes: int) -> np.ndarray:
		"""`quad` through engine.quad_adaptive on a cached plan of capacity deg_max; records deg_used / quad_bounds."""
		a = self._adaptive
		if self._builtin is None:
			raise ValueError("an adaptive degree takes built-in function names (the stage statistics are reduced on the device)")
		name, kw = self._builtin
		q, used, hist = engine.quad_adaptive(
			self._op, X, a["deg_max"], self._orth_given, name, stages=a["stages"], deg_rtol=a["deg_rtol"], endpoint=a["endpoint"],
			rtol=self._rtol, nprobes=nprobes, plan=self._plan(nprobes, False, adaptive=True), **kw,
		)  # fmt: skip
		self.deg_used, self.deg_history = used, hist
		if a["endpoint"] is not None:
			self.quad_bounds = (np.minimum(q[:, 0], q[:, 1]), np.maximum(q[:, 0], q[:, 1]))
			q = np.ascontiguousarray(q[:, 0])
		return q

	def quad(self, x: np.ndarray) -> np.ndarray:
		"""x^T f(A) x for every column of x by Lanczos quadrature (operators.py:126-151)."""
		x = np.asarray(x).astype(self.dtype, copy=False)
		x = np.atleast_2d(x).T if x.ndim == 1 else x
		if self._stale_ring:
			return self._quad_reference_ring(x)
		if self._adaptive is not None:
			return self._quad_adaptive(x, x.shape[1])
		plan = self._plan(x.shape[1], False)
		plan.set_probes(x)
		plan.run(self._rtol)
		if self._builtin is not None:
			name, kw = self._builtin
			y, nodes, weights = plan.quadrature(name, return_rule=True, **kw)
		else:
			y, nodes, weights = plan.quadrature(self._fun, return_rule=True)
		## the reference leaves the last probe's rule in self._nodes/_weights (operators.py:149)
		self._nodes[:], self._weights[:] = nodes[-1], weights[-1]
		return y

	def quad_generated(self, nprobes: int, pdf: str = "rademacher", seed: int = 0, probe_offset: int = 0) -> np.ndarray:
		"""v_i^T f(A) v_i for `nprobes` probes DRAWN ON THE DEVICE (Philox stream of probe ids probe_offset..;
		slq_plan_generate_probes): the throughput form of `quad`, with no n x nprobes host array at all."""
		assert not self._stale_ring, "device-drawn probes start from a clean ring"
		if self._adaptive is not None:
			return self._quad_adaptive((pdf, int(seed), int(probe_offset)), int(nprobes))
		plan = self._plan(int(nprobes), False)
		plan.generate_probes(pdf, seed=int(seed), probe_offset=int(probe_offset))
		plan.run(self._rtol)
		if self._builtin is not None:
			name, kw = self._builtin
			y, nodes, weights = plan.quadrature(name, return_rule=True, **kw)
		else:
			y, nodes, weights = plan.quadrature(self._fun, return_rule=True)
		self._nodes[:], self._weights[:] = nodes[-1], weights[-1]
		return y

	def _quad_reference_ring(self, x: np.ndarray) -> np.ndarray:
		"""The reference loop verbatim in structure (operators.py:145-150): per column, the native
		single-vector Lanczos on the persistent alpha/beta/Q, then the Gauss rule, then the sum."""
		from .integrate import quadrature
		from .lanczos import _native_lanczos

		y = np.zeros(x.shape[1])
		for j in range(x.shape[1]):
			xc = np.ascontiguousarray(x[:, j])
			_native_lanczos(self._op, xc, self._deg, self._rtol, self._orth, self._alpha, self._beta, self._Q)
			quadrature(self._alpha[: self._deg], self._beta[: self._deg], deg=self._deg, nodes=self._nodes, weights=self._weights)
			y[j] = np.sum(self._fun(self._nodes) * self._weights, axis=-1) * np.linalg.norm(xc) ** 2
		return y

	def _matvec(self, x: np.ndarray) -> np.ndarray:
		"""f(A) x ~= ||x|| Q Y (f(theta) * Y[0,:]) with the full Lanczos basis (operators.py:102-124)."""
		return self._matmat(np.asarray(x).reshape(-1, 1))

	def _matmat(self, X: np.ndarray) -> np.ndarray:
		X = np.asarray(X).astype(self.dtype, copy=False)
		plan = self._plan(X.shape[1], True)
		plan.set_probes(X)
		plan.run(self._rtol)
		if self._builtin is not None:
			name, kw = self._builtin
			return plan.fun_action(name, **kw)
		if plan.basis_kind != "keep":
			raise ValueError("a callable `fun` combines the Lanczos basis on the host: it needs basis='keep'")
		## Python callable: it can only be evaluated on the host, so the k x k eigenvectors of every probe's T come
		## back from the device eigensolver (one batched call) and the basis combination is done per probe
		a, b, _ = plan.tridiag()
		rws, Ys = engine.eigh_tridiag_batch(a[:, : self._deg], b[:, : self._deg], vectors=True, ctx=self._op.ctx)
		out = np.zeros((self.shape[0], X.shape[1]), dtype=self.dtype, order="F")
		for i in range(X.shape[1]):
			rw, Y = rws[i], Ys[i]
			coef = Y @ (np.ravel(self._fun(rw)) * Y[0, :])
			out[:, i] = np.linalg.norm(X[:, i]) * (plan.basis(i) @ coef)
		return out


def matrix_function(A, fun: Optional[Callable] = None, v: Optional[np.ndarray] = None, deg: int = 20):
	"""operators.py:155-161."""
	M = MatrixFunction(A, fun=fun, deg=deg)
	return M if v is None else M._matvec(v)


class GramOperator(LinearOperator):
	"""x -> A^T (A x) for a rectangular (sparse) A: the symmetric positive semidefinite operator behind the singular
	values of A (rank by `numrank`, nuclear / Schatten norms by `sqrt` of its spectrum, ...). The reference's native
	`SparseEigenLinearOperator<F, true>` (src/primate/include/eigen_operators.h:57-72), which its Python module never binds
	(`_lanczos.cpp:104-111`). On the device it is two panel SpMMs per Lanczos step (`slq_csr_gram_create`); the host
	methods are the plugin surface of every other operator."""

	_slq_kind = "gram"

	def __init__(self, A, dtype=None):
		import scipy.sparse as sp

		self.A = sp.csr_matrix(A)
		self.dtype = np.dtype(dtype if dtype is not None else (self.A.dtype if self.A.dtype in (np.float32, np.float64) else np.float64))
		self.A = self.A.astype(self.dtype)
		self.shape = (self.A.shape[1], self.A.shape[1])

	def _matvec(self, x: np.ndarray) -> np.ndarray:
		return self.A.T @ (self.A @ np.asarray(x).ravel())

	def _matmat(self, X: np.ndarray) -> np.ndarray:
		return self.A.T @ (self.A @ X)

	def _adjoint(self):
		return self


class AffineOperator(LinearOperator):
	"""A + t B for two sparse n x n matrices and a scalar t that changes between solves: the reference's native
	`SparseEigenAffineOperator` (src/primate/include/eigen_operators.h:106-137; unbound in its Python module). On the device
	both live on their union pattern as ONE CSR operator - every fused pass applies - and `set_parameter(t)` rewrites its
	values in place (`slq_csr_affine_create`, `slq_operator_set_parameter`), also for operators already wrapped in a
	`MatrixFunction`."""

	_slq_kind = "affine"

	def __init__(self, A, B, t: float = 0.0, dtype=None):
		import scipy.sparse as sp

		self.A, self.B = sp.csr_matrix(A), sp.csr_matrix(B)
		assert self.A.shape == self.B.shape and self.A.shape[0] == self.A.shape[1], "A and B must be square and of equal shape"
		self.dtype = np.dtype(dtype if dtype is not None else (self.A.dtype if self.A.dtype in (np.float32, np.float64) else np.float64))
		self.shape = self.A.shape
		self.t = float(t)

	def set_parameter(self, t: float) -> None:
		self.t = float(t)
		for ref in getattr(self, "_device_ops", []):
			op = ref()
			if op is not None and getattr(op, "_h", None):
				op.set_parameter(self.t)

	def _matvec(self, x: np.ndarray) -> np.ndarray:
		x = np.asarray(x).ravel()
		return (self.A @ x + self.t * (self.B @ x)).astype(self.dtype, copy=False)

	def _matmat(self, X: np.ndarray) -> np.ndarray:
		return (self.A @ X + self.t * (self.B @ X)).astype(self.dtype, copy=False)

	def _adjoint(self):
		return self


KERNEL_PROFILES = ("rbf", "matern12", "matern32", "matern52")
KERNEL_MAX_DIM = 64


def _kernel_profile(name: str, r2: np.ndarray) -> np.ndarray:
	"""phi(r2) of the four stationary profiles (r = sqrt(r2))."""
	if name == "rbf":
		return np.exp(-0.5 * r2)
	r = np.sqrt(r2)
	if name == "matern12":
		return np.exp(-r)
	if name == "matern32":
		a = np.sqrt(3.0) * r
		return (1.0 + a) * np.exp(-a)
	a = np.sqrt(5.0) * r
	return (1.0 + a + (5.0 / 3.0) * r2) * np.exp(-a)


def _kernel_chi(name: str, r2: np.ndarray) -> np.ndarray:
	"""chi = -2 dphi/dr2 of the four profiles; matern12's exp(-r) / r is DEFINED 0 at r2 = 0, as on the device."""
	if name == "rbf":
		return np.exp(-0.5 * r2)
	r = np.sqrt(r2)
	if name == "matern12":
		out = np.zeros_like(r2)
		pos = r2 > 0
		out[pos] = np.exp(-r[pos]) / r[pos]
		return out
	if name == "matern32":
		return 3.0 * np.exp(-np.sqrt(3.0) * r)
	a = np.sqrt(5.0) * r
	return (5.0 / 3.0) * (1.0 + a) * np.exp(-a)


class KernelOperator(LinearOperator):
	"""The kernel matrix of n points in d dimensions, never formed: with z_i = (x_i - mean(x)) / lengthscale rounded to `dtype`
	(the operator is DEFINED on these z), r2_ij = max(0, |z_i|^2 + |z_j|^2 - 2 z_i.z_j) (0 on the diagonal) and phi the profile
	("rbf": exp(-r2/2); "matern12": exp(-r); "matern32": (1 + sqrt3 r) exp(-sqrt3 r); "matern52": (1 + sqrt5 r + 5 r2/3) exp(-sqrt5 r)),

	    A = outputscale * phi(r2) + noise * I.

	The operator of a Gaussian process: `hutch(MatrixFunction(KernelOperator(X, "rbf", lengthscale=0.3, noise=1e-2), fun="log"))` is
	the log-determinant of its marginal likelihood. On the device (`slq_kernel_create`) a product evaluates tiles of A on the matrix
	cores and consumes them out of registers: the operator holds O(n d) words, whatever n. `X`: an (n, d) NumPy array (or (n,) for
	d = 1), or a torch tensor on the context's GPU (`slq_kernel_create_device`; the host methods below then work on a host copy).
	`lengthscale`: a scalar or one per dimension. mean(x) is fixed at construction: per dimension the sum over the points in row
	order in float64, divided by n. `set_parameters` changes lengthscale / outputscale / noise, also on operators already wrapped in
	a `MatrixFunction` - live plans compute with the new values from their next run. The host `_matvec` / `_matmat` are blocked
	NumPy in float64 from the definition: the plugin surface, and the model of the tests.

	`diag_scale`: an optional vector c of n entries, finite and >= 0, rounded once to `dtype` (the operator is defined
	on the rounded c, `self.diag_scale`), with which

	    A = outputscale * diag(c) phi(r2) diag(c) + noise * I.

	Fixed per-point noise K0 + diag(e) is E^{1/2} (D K0 D + I) E^{1/2} with c = e^{-1/2}; the B of a Laplace approximation is this
	operator with c = W^{1/2} and noise = 1 (`gp.fixed_noise_posterior`, `gp.laplace`). `set_diag_scale(c_or_None)` changes or clears
	it, on live device operators too. `cross()` and `features()` are defined on K0's points and profile and ignore the scale;
	`preconditioned()`, the gradients and the Gaussian-likelihood entries of `gp` refuse a scaled operator."""

	_slq_kind = "kernel"

	def __init__(self, X, kernel: str = "rbf", lengthscale=1.0, outputscale: float = 1.0, noise: float = 0.0, dtype=None, diag_scale=None):
		self._X_device = None
		if type(X).__module__.split(".")[0] == "torch":
			if dtype is None:
				dtype = {"torch.float64": np.float64, "torch.float32": np.float32}.get(str(X.dtype), np.float64)
			if X.is_cuda:
				self._X_device = X
			X = X.detach().cpu().numpy()
		X = np.asarray(X)
		if dtype is None:
			dtype = X.dtype if X.dtype in (np.float32, np.float64) else np.float64
		self.dtype = np.dtype(dtype)
		if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
			raise ValueError("Only 32- or 64-bit floats are supported.")
		if X.ndim == 1:
			X = X.reshape(-1, 1)
		if X.ndim != 2 or X.shape[0] < 1:
			raise ValueError(f"the points must be an (n, d) array, got shape {X.shape}")
		n, d = X.shape
		if not 1 <= d <= KERNEL_MAX_DIM:
			raise ValueError(f"kernel operator: d = {d} dimensions (1 <= d <= {KERNEL_MAX_DIM})")
		if not isinstance(kernel, str) or kernel not in KERNEL_PROFILES:
			raise ValueError(f"kernel operator: unknown profile {kernel!r} (one of {', '.join(KERNEL_PROFILES)})")
		self.X = np.ascontiguousarray(X, dtype=self.dtype)
		bad = np.argwhere(~np.isfinite(self.X))
		if bad.size:
			i, k = (int(v) for v in bad[0])
			raise ValueError(f"kernel operator: point {i}, coordinate {k} is {self.X[i, k]} (points must be finite)")
		self.kernel = kernel
		self.shape = (n, n)
		## the centre: sequential float64 sums in row order (cumsum adds in order; np.sum is pairwise), as the library takes it
		self.mean = np.cumsum(self.X, axis=0, dtype=np.float64)[-1] / np.float64(n)
		self.lengthscale, self.outputscale, self.noise = self._check_parameters(lengthscale, outputscale, noise)
		self._z = None
		self.diag_scale = self._check_diag_scale(diag_scale)

	def _check_diag_scale(self, c):
		"""None, or c as the operator holds it: n entries, finite and >= 0, rounded once to the operator's dtype."""
		if c is None:
			return None
		n = self.shape[0]
		c = np.asarray(c, dtype=np.float64).ravel()
		if c.size != n:
			raise ValueError(f"kernel operator: the diagonal scale has {c.size} entries, the operator n = {n} points")
		with np.errstate(over="ignore"):
			cr = c.astype(self.dtype)
		bad = np.flatnonzero(~(np.isfinite(c) & (c >= 0) & np.isfinite(cr)))
		if bad.size:
			raise ValueError(f"kernel operator: diag_scale[{int(bad[0])}] = {c[bad[0]]} is not a finite number >= 0 in the operator's dtype")
		return cr

	def set_diag_scale(self, c) -> None:
		"""A new diagonal scale (None: clear it), forwarded to every live device operator built from this object."""
		self.diag_scale = self._check_diag_scale(c)
		for ref in getattr(self, "_device_ops", []):
			op = ref()
			if op is not None and getattr(op, "_h", None):
				op.set_kernel_diag_scale(self.diag_scale)

	def _check_parameters(self, lengthscale, outputscale, noise):
		d = self.X.shape[1]
		ls = np.atleast_1d(np.asarray(lengthscale, dtype=np.float64)).ravel()
		if ls.size not in (1, d):
			raise ValueError(f"kernel operator: {ls.size} lengthscales (1 or d = {d})")
		badl = np.flatnonzero(~(np.isfinite(ls) & (ls > 0)))
		if badl.size:
			raise ValueError(f"kernel operator: lengthscale[{int(badl[0])}] = {ls[badl[0]]} is not a positive finite number")
		s, v = float(outputscale), float(noise)
		if not (np.isfinite(s) and s > 0):
			raise ValueError(f"kernel operator: outputscale = {s} is not a positive finite number")
		if not (np.isfinite(v) and v >= 0):
			raise ValueError(f"kernel operator: noise = {v} is not a finite number >= 0")
		return ls.copy(), s, v

	def set_parameters(self, lengthscale=None, outputscale=None, noise=None) -> None:
		"""New hyperparameters (None: unchanged), forwarded to every live device operator built from this object."""
		self.lengthscale, self.outputscale, self.noise = self._check_parameters(
			self.lengthscale if lengthscale is None else lengthscale,
			self.outputscale if outputscale is None else outputscale,
			self.noise if noise is None else noise,
		)
		self._z = None
		for ref in getattr(self, "_device_ops", []):
			op = ref()
			if op is not None and getattr(op, "_h", None):
				op.set_kernel_parameters(self.lengthscale, self.outputscale, self.noise)

	def scaled_points(self) -> np.ndarray:
		"""z = (x - mean) / lengthscale, computed in float64 and rounded once to the operator's dtype: what the operator is defined on."""
		if self._z is None:
			ls = np.broadcast_to(self.lengthscale, (self.X.shape[1],))
			self._z = ((self.X.astype(np.float64) - self.mean) / ls).astype(self.dtype)
		return self._z

	def rows(self, idx) -> np.ndarray:
		"""Rows `idx` of A in float64, from the definition (norms plus dot product, clamped, exact zeros on the diagonal)."""
		idx = np.asarray(idx, dtype=np.int64).ravel()
		z = self.scaled_points().astype(np.float64)
		nrm = np.einsum("ij,ij->i", z, z)
		r2 = np.maximum(nrm[idx, None] + nrm[None, :] - 2.0 * (z[idx] @ z.T), 0.0)
		r2[np.arange(idx.size), idx] = 0.0
		K = self.outputscale * _kernel_profile(self.kernel, r2)
		if self.diag_scale is not None:
			c = self.diag_scale.astype(np.float64)
			K = K * (c[idx, None] * c[None, :])
		K[np.arange(idx.size), idx] += self.noise
		return K

	def _matmat(self, X: np.ndarray) -> np.ndarray:
		X = np.asarray(X)
		if X.ndim != 2 or X.shape[0] != self.shape[1]:
			raise ValueError(f"dimension mismatch: the operator is {self.shape[0]} x {self.shape[1]}, the operand has {X.shape[0]} rows")
		n = self.shape[0]
		Y = np.empty((n, X.shape[1]), dtype=np.float64)
		X64 = X.astype(np.float64, copy=False)
		for i0 in range(0, n, 1024):
			i1 = min(n, i0 + 1024)
			Y[i0:i1] = self.rows(np.arange(i0, i1)) @ X64
		return Y.astype(self.dtype, copy=False)

	def _matvec(self, x: np.ndarray) -> np.ndarray:
		x = np.asarray(x)
		if x.size != self.shape[1]:
			raise ValueError(f"dimension mismatch: the operator is {self.shape[0]} x {self.shape[1]}, the operand has {x.size} entries")
		return self._matmat(x.reshape(-1, 1)).ravel()

	def _adjoint(self):
		return self

	def preconditioned(self, rank: int = 100, tol: float = 0.0) -> "PreconditionedKernelOperator":
		"""B = M A M with M = P^{-1/2} of a rank-`rank` pivoted-Cholesky factor of this operator without its noise (DESIGN.md
		§4.18): the operator to run Lanczos on when the noise is small. It follows this operator's hyperparameters. Not built for an
		operator with a diagonal scale."""
		return PreconditionedKernelOperator(self, rank, tol)

	def cross(self, Xnew) -> "KernelCrossOperator":
		"""The cross-covariance between the new points `Xnew` (m x d) and this operator's points: a `KernelCrossOperator` of shape
		(m, n). It follows this operator's hyperparameters, whenever they are set."""
		return KernelCrossOperator(self, Xnew)

	def features(self, num_features: int = 2048, seed=None, frequencies=None) -> "KernelFeatures":
		"""Random Fourier features of this operator's profile: a host value `KernelFeatures` with `num_features`
		frequencies drawn from the profile's spectral measure by `numpy.random.default_rng(seed)` - or the explicit `frequencies`
		(F2 x d) instead of the draw. Host-only: no GPU, no library. `.device(op)` is the product on the GPU."""
		if frequencies is not None:
			return KernelFeatures(self, frequencies)
		return KernelFeatures(self, draw_kernel_frequencies(self.kernel, int(num_features), self.X.shape[1], np.random.default_rng(seed)))


def refuse_diag_scale(K, what: str) -> None:
	"""ValueError where `K` is a KernelOperator with a diagonal scale: `what` is not built for one. Host-only: called
	before the library is touched."""
	if getattr(K, "_slq_kind", None) == "kernel_precond":
		K = K.base
	if getattr(K, "diag_scale", None) is not None:
		raise ValueError(
			f"{what} is not built for a KernelOperator with a diagonal scale (diag_scale / set_diag_scale): "
			"use gp.fixed_noise_posterior for per-point noise and gp.laplace for a non-Gaussian likelihood"
		)


def draw_kernel_frequencies(kernel: str, num_features: int, d: int, rng) -> np.ndarray:
	"""F2 x d frequencies of the profile's spectral measure in the scaled coordinates, float64, in ONE defined order of draws from
	`rng`: G = standard_normal((F2, d)); rbf: Omega = G; matern with 2 nu in {1, 3, 5}: then u = chisquare(2 nu, F2) and
	Omega_j = G_j sqrt(2 nu / u_j) - the multivariate Student-t with 2 nu degrees of freedom."""
	if kernel not in KERNEL_PROFILES:
		raise ValueError(f"unknown profile {kernel!r} (one of {', '.join(KERNEL_PROFILES)})")
	if num_features < 1:
		raise ValueError(f"num_features = {num_features} must be >= 1")
	G = rng.standard_normal((num_features, d))
	if kernel == "rbf":
		return G
	dof = {"matern12": 1.0, "matern32": 3.0, "matern52": 5.0}[kernel]
	u = rng.chisquare(dof, num_features)
	return G * np.sqrt(dof / u)[:, None]


class KernelFeatures:
	"""The feature map Phi(z) = sqrt(s / F2) [cos(Omega z) | sin(Omega z)] of a KernelOperator `K` as a host value:
	`omega` (float64, F2 x d), the profile's name, and K itself for its scaled points and outputscale of now. Paired features, no random
	phase: Phi(z) Phi(z')^T = (s / F2) sum_j cos(omega_j.(z - z')) is exactly stationary, its diagonal exactly s. The map is DEFINED on
	`rounded()`, Omega rounded once to K's dtype. `matrix(Xnew)` is the host model in float64; `device(op)` the product on the GPU
	(engine.KernelFeatureMap)."""

	def __init__(self, K: "KernelOperator", omega):
		if getattr(K, "_slq_kind", None) != "kernel":
			raise ValueError("KernelFeatures needs a KernelOperator")
		d = K.X.shape[1]
		om = np.array(omega, dtype=np.float64)
		om = om.reshape(-1, 1) if om.ndim == 1 else om
		if om.ndim != 2 or om.shape[1] != d or om.shape[0] < 1:
			raise ValueError(f"the frequencies must be an (F2, {d}) array with F2 >= 1, got shape {om.shape}")
		if not np.all(np.isfinite(om)):
			j, k = (int(v) for v in np.argwhere(~np.isfinite(om))[0])
			raise ValueError(f"kernel features: frequency {j}, coordinate {k} is {om[j, k]} (frequencies must be finite)")
		self.K, self.kernel, self.omega = K, K.kernel, om
		self.num_features = int(om.shape[0])
		self.dtype = np.dtype(K.dtype)

	def rounded(self) -> np.ndarray:
		"""Omega rounded once to the operator's dtype: what the device holds."""
		return self.omega.astype(self.dtype)

	def matrix(self, Xnew=None) -> np.ndarray:
		"""Phi in float64 from the definition, rows x 2 F2, at K's points (None) or at new points (K's centre and lengthscales of now)."""
		z = (self.K.scaled_points() if Xnew is None else self.K.cross(Xnew).scaled_points()).astype(np.float64)
		g = z @ self.rounded().astype(np.float64).T
		return np.sqrt(self.K.outputscale / self.num_features) * np.hstack([np.cos(g), np.sin(g)])

	def device(self, op=None) -> "engine.KernelFeatureMap":
		"""The product on the GPU: an engine.KernelFeatureMap over `op` (default: K's cached device operator)."""
		op = _as_device_operator(self.K, dtype=self.dtype) if op is None else op
		return engine.KernelFeatureMap(op, self.omega)


KERNEL_PRECOND_MAX_RANK = 256


def precond_g(t: np.ndarray, sigma2: float) -> np.ndarray:
	"""g(t) = (1 - (1 + t / sigma2)^{-1/2}) / t, smooth at 0 where it is 1 / (2 sigma2); negative t count as 0."""
	x = np.maximum(np.asarray(t, dtype=np.float64), 0.0) / sigma2
	small = ~(x > 2.0**-60)
	xs = np.where(small, 1.0, x)
	h = np.where(small, 0.5, np.minimum(-np.expm1(-0.5 * np.log1p(xs)) / xs, 0.5))
	return h / sigma2


class PreconditionedKernelOperator(LinearOperator):
	"""B = M A M for the KernelOperator `base` (A = K0 + noise I, noise > 0), M = P^{-1/2}, P = L L^T + noise I with L the greedy
	partial pivoted Cholesky factor of K0 of rank at most `rank`: the residual diagonal starts as d = s; step k
	takes p = argmax d (ties: the smallest index), L[:, k] = (K0[:, p] - L[:, :k] L[p, :k]^T) / sqrt(d_p), d <- max(0, d - L[:, k]^2),
	d_p <- 0; rows with d_i = 0 already get 0; it stops when d_p <= max(tol, 64 eps) s. B is symmetric positive definite,
	logdet A = tr log B + logdet P and A^-1 y = M B^-1 M y for any L. On the device (`slq_kernel_precond_create`) the factor, the
	applies of M and the product run in HIP kernels. The host side here is the model of the tests, O(n^2) NumPy in float64 from the
	definition, for small n: `_matmat`, `inv_sqrt`, and the attributes `rank`, `pivots`, `logdet_precond`, `residual_trace`."""

	_slq_kind = "kernel_precond"

	def __init__(self, base: KernelOperator, rank: int = 100, tol: float = 0.0):
		if getattr(base, "_slq_kind", None) != "kernel":
			raise ValueError("PreconditionedKernelOperator needs a KernelOperator")
		refuse_diag_scale(base, "the pivoted-Cholesky preconditioner")
		if np.dtype(base.dtype) != np.float64:
			raise ValueError(f"the preconditioner is fp64 only: the KernelOperator is {np.dtype(base.dtype)}")
		if not base.noise > 0:
			raise ValueError("the preconditioner needs noise > 0 (P^{-1/2} = (L L^T + noise I)^{-1/2})")
		rank = int(rank)
		if not 1 <= rank <= KERNEL_PRECOND_MAX_RANK:
			raise ValueError(f"rank = {rank} (1 <= rank <= {KERNEL_PRECOND_MAX_RANK})")
		tol = float(tol)
		if not (np.isfinite(tol) and tol >= 0):
			raise ValueError(f"tol = {tol} is not a finite number >= 0")
		self.base, self.tol = base, tol
		self.rank_max = min(rank, base.shape[0])
		self.shape, self.dtype = base.shape, np.dtype(np.float64)
		self._model, self._model_key = None, None

	def _key(self):
		K = self.base
		return (tuple(np.atleast_1d(K.lengthscale).tolist()), float(K.outputscale), float(K.noise))

	def k0(self) -> np.ndarray:
		"""s phi(r2) of the base's points, dense, without the noise term (exact zeros of r2 on the diagonal)."""
		K = self.base
		z = K.scaled_points().astype(np.float64)
		nrm = np.einsum("ij,ij->i", z, z)
		r2 = np.maximum(nrm[:, None] + nrm[None, :] - 2.0 * (z @ z.T), 0.0)
		np.fill_diagonal(r2, 0.0)
		return K.outputscale * _kernel_profile(K.kernel, r2)

	def host_model(self) -> dict:
		"""{L, pivots, d, t, V, G, H, logdet_p} by the definition, for the base's parameters of now (cached per parameter set)."""
		if self._model is not None and self._model_key == self._key():
			return self._model
		K = self.base
		n, r, s, sigma2 = self.shape[0], self.rank_max, float(K.outputscale), float(K.noise)
		K0 = self.k0()
		d = np.full(n, s)
		L = np.zeros((n, r))
		piv = []
		stop = max(self.tol, 64.0 * np.finfo(np.float64).eps) * s
		for k in range(r):
			p = int(np.argmax(d))
			if not d[p] > stop:
				break
			col = (K0[:, p] - L[:, :k] @ L[p, :k]) / np.sqrt(d[p])
			dead = d == 0.0
			dead[p] = False
			col[dead] = 0.0
			L[:, k] = col
			d = np.maximum(d - col * col, 0.0)
			d[p] = 0.0
			piv.append(p)
		t, V = np.linalg.eigh(L.T @ L)
		t = np.maximum(t, 0.0)
		G = (V * precond_g(t, sigma2)) @ V.T
		H = (V / (t + sigma2)) @ V.T  # (L^T L + sigma2 I)^-1: P^-1 = (I - L H L^T) / sigma2 (§4.19)
		self._model = dict(L=L, pivots=np.array(piv, dtype=np.int64), d=d, t=t, V=V, G=G, H=H, logdet_p=float(np.sum(np.log1p(t / sigma2)) + n * np.log(sigma2)))
		self._model_key = self._key()
		return self._model

	@property
	def rank(self) -> int:
		return int(self.host_model()["pivots"].size)

	@property
	def pivots(self) -> np.ndarray:
		return self.host_model()["pivots"]

	@property
	def logdet_precond(self) -> float:
		return self.host_model()["logdet_p"]

	@property
	def residual_trace(self) -> float:
		return float(np.sum(self.host_model()["d"]))

	def trace_grad_exact(self, L: Optional[np.ndarray] = None, H: Optional[np.ndarray] = None) -> np.ndarray:
		"""tr(P^-1 dA/dtheta) as d + 2 values - the lengthscales per dimension, the outputscale, the noise, as a
		KernelGradAccumulator holds them - in float64 NumPy from the definition: with C = (L H) L^T

		    sigma^-2 [tr D - sum_ij C_ij D_ij],   D_lk = (s / l_k) chi(r2) (z_ik - z_jk)^2,  D_s = phi(r2),  D_sigma2 = I,

		tr D = 0, n, n. L, H: the host model's (None), or another factor's - the device's, for the tests. This is the exact part of
		the gradient of logdet A that `gp.logdet_grad` adds its sampled remainder to; P itself is not differentiated."""
		m = self.host_model() if L is None or H is None else None
		L = m["L"] if L is None else np.asarray(L, dtype=np.float64)
		H = m["H"] if H is None else np.asarray(H, dtype=np.float64)
		K = self.base
		n, d = K.X.shape
		s, sigma2 = float(K.outputscale), float(K.noise)
		ls = np.broadcast_to(np.asarray(K.lengthscale, dtype=np.float64), (d,))
		z = K.scaled_points().astype(np.float64)
		nrm = np.einsum("ij,ij->i", z, z)
		r2 = np.maximum(nrm[:, None] + nrm[None, :] - 2.0 * (z @ z.T), 0.0)
		np.fill_diagonal(r2, 0.0)
		Cm = (L @ H) @ L.T
		Bm = Cm * _kernel_chi(K.kernel, r2)
		out = np.zeros(d + 2)
		for k in range(d):
			D = z[:, k][:, None] - z[None, :, k]
			out[k] = -(s / ls[k]) * np.sum(Bm * D * D) / sigma2
		out[d] = (n - np.sum(Cm * _kernel_profile(K.kernel, r2))) / sigma2
		out[d + 1] = (n - np.trace(Cm)) / sigma2
		return out

	def inv_sqrt(self, X: np.ndarray) -> np.ndarray:
		"""P^{-1/2} X = (X - L G L^T X) / sigma."""
		m = self.host_model()
		X = np.asarray(X, dtype=np.float64)
		X2 = X.reshape(self.shape[0], -1)
		Y = (X2 - m["L"] @ (m["G"] @ (m["L"].T @ X2))) / np.sqrt(float(self.base.noise))
		return Y.reshape(X.shape)

	def _matmat(self, X: np.ndarray) -> np.ndarray:
		X = np.asarray(X)
		if X.ndim != 2 or X.shape[0] != self.shape[1]:
			raise ValueError(f"dimension mismatch: the operator is {self.shape[0]} x {self.shape[1]}, the operand has {X.shape[0]} rows")
		return self.inv_sqrt(self.base._matmat(self.inv_sqrt(X)))

	def _matvec(self, x: np.ndarray) -> np.ndarray:
		x = np.asarray(x)
		if x.size != self.shape[1]:
			raise ValueError(f"dimension mismatch: the operator is {self.shape[0]} x {self.shape[1]}, the operand has {x.size} entries")
		return self._matmat(x.reshape(-1, 1)).ravel()

	def _adjoint(self):
		return self


class KernelCrossOperator(LinearOperator):
	"""C = outputscale * phi(r2(X*, X)), m x n, between new points X* and the n points of the KernelOperator `K`, never formed
	(DESIGN.md §4.17): z* = (x* - mean(X)) / lengthscale with K's centre - the TRAINING centre, never the new points' own -
	computed in float64 and rounded once to K's dtype; r2_ij = max(0, |z*_i|^2 + |z_j|^2 - 2 z*_i.z_j) with no diagonal rule
	(a new point equal to a training point gets what the arithmetic gives); no noise term. `C @ W` is the forward product,
	`C.T @ U` (or `rmatmat`) the adjoint. It reads K's lengthscale and outputscale at every product, so `K.set_parameters` needs
	no forwarding. `Xnew`: an (m, d) NumPy array ((m,) for d = 1), or a torch tensor on the context's GPU (`device()` then hands
	the library the device pointer; the host methods work on a host copy). The host `_matmat` / `_rmatmat` are blocked NumPy in
	float64 from the definition: the plugin surface, and the model of the tests. `device(op)` is the product on the GPU
	(engine.KernelCross)."""

	def __init__(self, K: KernelOperator, Xnew, _transposed: bool = False):
		if getattr(K, "_slq_kind", None) != "kernel":
			raise ValueError("KernelCrossOperator needs a KernelOperator")
		self.K = K
		self._X_device = None
		self._Xnew_arg = Xnew
		if type(Xnew).__module__.split(".")[0] == "torch":
			if Xnew.is_cuda:
				self._X_device = Xnew
			Xnew = Xnew.detach().cpu().numpy()
		X = np.asarray(Xnew)
		d = K.X.shape[1]
		if X.ndim == 1:
			X = X.reshape(-1, 1)
		if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] != d:
			raise ValueError(f"the new points must be an (m, {d}) array with m >= 1, got shape {X.shape}")
		self.Xnew = np.ascontiguousarray(X, dtype=K.dtype)
		bad = np.argwhere(~np.isfinite(self.Xnew))
		if bad.size:
			i, k = (int(v) for v in bad[0])
			raise ValueError(f"kernel cross: new point {i}, coordinate {k} is {self.Xnew[i, k]} (points must be finite)")
		self.dtype = np.dtype(K.dtype)
		self.transposed = bool(_transposed)
		m, n = self.Xnew.shape[0], K.shape[0]
		self.shape = (n, m) if self.transposed else (m, n)

	def scaled_points(self) -> np.ndarray:
		"""z* = (x* - mean(X)) / lengthscale in float64, rounded once to the operator's dtype, with K's parameters of now."""
		ls = np.broadcast_to(self.K.lengthscale, (self.Xnew.shape[1],))
		return ((self.Xnew.astype(np.float64) - self.K.mean) / ls).astype(self.dtype)

	def rows(self, idx) -> np.ndarray:
		"""Rows `idx` of the m x n matrix C in float64, from the definition (norms plus dot product, clamped)."""
		idx = np.asarray(idx, dtype=np.int64).ravel()
		zs = self.scaled_points().astype(np.float64)[idx]
		z = self.K.scaled_points().astype(np.float64)
		r2 = np.maximum(np.einsum("ij,ij->i", zs, zs)[:, None] + np.einsum("ij,ij->i", z, z)[None, :] - 2.0 * (zs @ z.T), 0.0)
		return self.K.outputscale * _kernel_profile(self.K.kernel, r2)

	def _product(self, X: np.ndarray, trans: bool) -> np.ndarray:
		m, n = self.Xnew.shape[0], self.K.shape[0]
		rin, rout = (m, n) if trans else (n, m)
		X = np.asarray(X)
		if X.ndim != 2 or X.shape[0] != rin:
			raise ValueError(f"dimension mismatch: the product reads {rin} rows, the operand has shape {X.shape}")
		X64 = X.astype(np.float64, copy=False)
		Y = np.zeros((rout, X.shape[1]), dtype=np.float64)
		for i0 in range(0, m, 1024):
			i1 = min(m, i0 + 1024)
			Cb = self.rows(np.arange(i0, i1))
			if trans:
				Y += Cb.T @ X64[i0:i1]
			else:
				Y[i0:i1] = Cb @ X64
		return Y.astype(self.dtype, copy=False)

	def _matmat(self, X: np.ndarray) -> np.ndarray:
		return self._product(X, self.transposed)

	def _rmatmat(self, X: np.ndarray) -> np.ndarray:
		return self._product(X, not self.transposed)

	def _matvec(self, x: np.ndarray) -> np.ndarray:
		x = np.asarray(x)
		if x.size != self.shape[1]:
			raise ValueError(f"dimension mismatch: the operator is {self.shape[0]} x {self.shape[1]}, the operand has {x.size} entries")
		return self._matmat(x.reshape(-1, 1)).ravel()

	def _rmatvec(self, x: np.ndarray) -> np.ndarray:
		return self._rmatmat(np.asarray(x).reshape(-1, 1)).ravel()

	def _adjoint(self):
		return KernelCrossOperator(self.K, self._Xnew_arg, _transposed=not self.transposed)

	def _transpose(self):
		return self._adjoint()

	def device(self, op=None) -> "engine.KernelCross":
		"""The products on the GPU: an engine.KernelCross over `op` (default: K's cached device operator). Its `matmat(X, trans)`
		is that of the m x n matrix, whatever `transposed` says."""
		op = _as_device_operator(self.K, dtype=self.dtype) if op is None else op
		return engine.KernelCross(op, self._X_device if self._X_device is not None else self.Xnew)


class Toeplitz(LinearOperator):
	"""Matrix-free symmetric-or-not Toeplitz operator with first column `c` and first row `r` (default r = c),
	applied by circulant embedding and two FFTs of length 2n (src/primate/operators.py:165-183). A host-side
	plugin: `lanczos`/`MatrixFunction` reach it through the callback operator (`slq_callback_create`)."""

	def __init__(self, c: np.ndarray, r: Optional[np.ndarray] = None, dtype: np.dtype = np.float64):
		self.c = np.array(c)
		self.r = np.array(c if r is None else r)
		n = len(self.c)
		## first column of the 2n x 2n circulant that contains T in its leading block: [c, 0, r_{n-1}, ..., r_1]
		self._symbol = np.fft.fft(np.concatenate((self.c, [0], self.r[:0:-1])))
		self._pad = np.zeros(2 * n)
		self.shape = (n, n)
		self.dtype = np.dtype(dtype)

	def _matvec(self, x: np.ndarray) -> np.ndarray:
		n = self.shape[0]
		assert np.size(x) == n, f"Invalid shape of input vector 'x'; must have length {n}"
		self._pad[:n] = np.ravel(x)
		y = np.fft.ifft(self._symbol * np.fft.fft(self._pad))
		return np.real(y[:n]).astype(self.dtype)


class ToeplitzOperator(Toeplitz):
	"""The Toeplitz matrix A_ij = c[i-j] (i >= j), r[j-i] (j > i) as a DEVICE operator (`slq_toeplitz_create`): a
	product is three FFT passes of length L = 2^ceil(log2 2n) along the rows of the probe panel as it stands in memory - two probes per
	complex column, O(n log n) per probe, n up to 2^22. `c` and `r` (default r = c; r[0] is ignored, as in SciPy) are rounded once to
	`dtype`: the operator is defined on the rounded values (`self.c`, `self.r`), and is `symmetric` iff the rounded r[1:] equals c[1:].
	A stationary kernel on a regular 1-D grid is such a matrix: `ToeplitzOperator.from_kernel("rbf", n, spacing, ...)`.

	`lanczos`, `MatrixFunction`, `ChebyshevFunction`, `hutch`, `xtrace` and `spectral_density` take a symmetric one like any other
	operator; a non-symmetric one has products (`engine.DeviceOperator(T).matmat`) and no plans. `set_values(c, r)` rewrites the values,
	also on operators already wrapped in a `MatrixFunction` - live plans compute with them from their next run; it may not change the
	symmetry. The host `_matvec` / `_matmat` (NumPy FFTs in double on the rounded values) are the plugin surface inherited from `Toeplitz`,
	which itself stays the host plugin it was."""

	_slq_kind = "toeplitz"
	MAX_N = 1 << 22

	def __init__(self, c, r=None, dtype=np.float64):
		self.dtype = np.dtype(dtype)
		if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
			raise ValueError("Only 32- or 64-bit floats are supported.")
		self._set(*self._check_values(c, r, None))

	def _check_values(self, c, r, n):
		c = np.asarray(c, dtype=np.float64)
		if c.ndim != 1:
			raise ValueError(f"Toeplitz operator: c must be a vector, got shape {c.shape}")
		if n is not None and c.size != n:
			raise ValueError(f"Toeplitz operator: c has {c.size} entries, the operator n = {n}")
		if c.size < 1:
			raise ValueError("Toeplitz operator: n = 0 must be at least 1")
		if c.size > self.MAX_N:
			raise ValueError(f"Toeplitz operator: n = {c.size} exceeds the supported maximum {self.MAX_N}")
		r = c if r is None else np.asarray(r, dtype=np.float64)
		if r.shape != c.shape:
			raise ValueError(f"Toeplitz operator: r has shape {r.shape}, c has {c.size} entries")
		with np.errstate(over="ignore"):
			cr, rr = c.astype(self.dtype), r.astype(self.dtype)
		rr[0] = cr[0]  # (r[0] is ignored)
		for name, given, rounded in (("c", c, cr), ("r", r, rr)):
			bad = np.flatnonzero(~np.isfinite(rounded))
			if bad.size:
				raise ValueError(f"Toeplitz operator: {name}[{int(bad[0])}] = {given[bad[0]]} is not finite in the operator's dtype")
		return cr, rr

	def _set(self, cr, rr):
		n = cr.size
		self.c, self.r = cr, rr
		self.symmetric = bool(cr[1:].tobytes() == rr[1:].tobytes())
		self.shape = (n, n)
		self._symbol = np.fft.fft(np.concatenate((cr.astype(np.float64), [0.0], rr[:0:-1].astype(np.float64))))
		self._pad = np.zeros(2 * n)

	def set_values(self, c, r=None) -> None:
		"""New c and r of the same n (and the same symmetry), forwarded to every live device operator built from this object."""
		cr, rr = self._check_values(c, r, self.shape[0])
		if bool(cr[1:].tobytes() == rr[1:].tobytes()) != self.symmetric:
			raise ValueError("Toeplitz operator: set_values may not change the symmetry of the operator (create a new one)")
		## the live device operators first, the host state after: a refused or failed device call leaves the host object as it was, and
		## the device operators already changed are put back
		live = [op for op in (ref() for ref in getattr(self, "_device_ops", [])) if op is not None and getattr(op, "_h", None)]
		done = []
		try:
			for op in live:
				op.set_toeplitz_values(cr, rr)
				done.append(op)
		except Exception:
			for op in done:
				op.set_toeplitz_values(self.c, self.r)
			raise
		self._set(cr, rr)

	def _matmat(self, X: np.ndarray) -> np.ndarray:
		n = self.shape[0]
		X = np.asarray(X, dtype=np.float64).reshape(n, -1)
		F = np.fft.fft(np.concatenate((X, np.zeros((self._symbol.size - n, X.shape[1]))), axis=0), axis=0)
		return np.real(np.fft.ifft(self._symbol[:, None] * F, axis=0)[:n]).astype(self.dtype)

	def _adjoint(self):
		return ToeplitzOperator(self.r, self.c, dtype=self.dtype)

	@classmethod
	def from_kernel(cls, kernel: str, n: int, spacing: float, lengthscale: float = 1.0, outputscale: float = 1.0, noise: float = 0.0, dtype=np.float64):
		"""The kernel matrix of `KernelOperator`'s profiles on the grid spacing * arange(n): first column
		outputscale * phi((k spacing / lengthscale)^2) + noise [k = 0]."""
		if not isinstance(kernel, str) or kernel not in KERNEL_PROFILES:
			raise ValueError(f"Toeplitz operator: unknown profile {kernel!r} (one of {', '.join(KERNEL_PROFILES)})")
		for name, v, ok in (("spacing", spacing, spacing > 0), ("lengthscale", lengthscale, lengthscale > 0), ("outputscale", outputscale, outputscale > 0), ("noise", noise, noise >= 0)):
			if not (np.isfinite(v) and ok):
				raise ValueError(f"Toeplitz operator: {name} = {v} is out of range")
		if int(n) < 1:
			raise ValueError(f"Toeplitz operator: n = {n} must be at least 1")
		k = np.arange(int(n), dtype=np.float64)
		c = float(outputscale) * _kernel_profile(kernel, (k * float(spacing) / float(lengthscale)) ** 2)
		c[0] += float(noise)
		return cls(c, dtype=dtype)


class TorchOperator(LinearOperator):
	"""A symmetric operator given as a function on GPU-resident torch tensors, `fn(X) -> A X` for X of shape
	(n, b) on this process's GPU. Used as `A` in `lanczos` / `MatrixFunction` / `hutch`, its products run inside
	the device Lanczos loop on libslq's stream without a host round trip (`slq_device_callback_create`): the
	GPU-native form of the reference's `LinearOperator` plugin surface (src/primate/operators.py:15-33)."""

	def __init__(self, fn: Callable, n: int, dtype=np.float64, device: Optional[int] = None):
		self.fn, self.shape, self.dtype = fn, (int(n), int(n)), np.dtype(dtype)
		## the GPU `fn` computes on: LOCAL_RANK under torchrun (what `engine.Context` picks too), else torch's current
		## device at construction time. The device products below do NOT consult torch.cuda.current_device().
		self.device = device

	def _device(self):
		import os

		import torch

		if self.device is None:
			self.device = int(os.environ["LOCAL_RANK"]) if "LOCAL_RANK" in os.environ else torch.cuda.current_device()
		return torch.device("cuda", int(self.device))

	def matmat_device(self, X, Y, stream) -> None:
		import torch

		## X, Y and the stream belong to the GPU of the DeviceOperator's Context, which the views carry
		owner = getattr(X, "device_index", None)
		dev = torch.device("cuda", int(owner)) if owner is not None else self._device()
		if self.device is not None and owner is not None:
			assert int(self.device) == int(owner), f"TorchOperator on cuda:{self.device} driven by a Context on cuda:{owner}"
		with torch.cuda.device(dev), torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=dev)):
			x, y = torch.as_tensor(X, device=dev), torch.as_tensor(Y, device=dev)  # (b, n) views of column-major n x b
			y.copy_(self.fn(x.T).T)

	def _matmat(self, X: np.ndarray) -> np.ndarray:
		import torch

		dev = self._device()
		return self.fn(torch.as_tensor(np.ascontiguousarray(X), device=dev).to(torch.float64 if self.dtype == np.float64 else torch.float32)).cpu().numpy()

	def _matvec(self, x: np.ndarray) -> np.ndarray:
		return self._matmat(np.asarray(x).reshape(-1, 1)).ravel()
