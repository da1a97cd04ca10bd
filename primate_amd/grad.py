"""The gradient of tr f(A) with the value: for symmetric A, d tr f(A) / dA = f'(A), and its Girard-Hutchinson estimate on the
stored nonzeros e = (row, col) of a pattern is

    G[e] = (1/N) sum_i (f'(A) v_i)[row(e)] v_i[col(e)]

Both factors are already on the device after a run - the probes (`plan.get_probes_into`) and f'(A) V (`plan.fun_action_into`, or
one Chebyshev action) - and engine.SddmmAccumulator contracts them on the pattern (slq_sddmm_update): nothing of size n leaves
the GPU, and one run per batch yields the value and the gradient. `primate_amd.autograd.trace_fun` puts a torch
`autograd.Function` on top.

A KernelOperator has hyperparameters instead of stored entries: `kernel_trace_grad` runs the same batches and contracts the same two
factors against tiles of dA/dtheta (engine.KernelGradAccumulator, slq_kernel_grad_update) into d + 2 numbers - the lengthscales,
the outputscale, the noise; `kernel_quadratic_grad` is the same contraction for host vectors, the data-fit term of a marginal
likelihood. `primate_amd.autograd.kernel_trace_fun` is the torch function on top.
"""

from __future__ import annotations

from typing import Callable, Optional, Union

import numpy as np

from . import engine
from .special import param_callable

_EPS64 = np.finfo(np.float64).eps


def lanczos_derivative(name: str, kwargs: Optional[dict] = None) -> Optional[tuple]:
	"""(name', kwargs', scale) with f' = scale * name'(.; kwargs') among the built-in spectral functions, for the built-in f =
	`name`: the Lanczos route evaluates f'(A) V with the function ids the library already has. None for "identity" (f' = 1: the
	gradient is exact). ValueError for a built-in whose derivative is no built-in."""
	kwargs = dict(kwargs or {})
	if name == "identity":
		return None
	if name == "log":
		return "inv", {}, 1.0
	if name == "exp":
		t = float(kwargs.get("t", 1.0))
		return "exp", {"t": t}, t
	raise ValueError(
		f"the derivative of '{name}' is not a built-in spectral function: use the Chebyshev route, "
		f"trace_grad(ChebyshevFunction(A, '{name}', deg=...), dfun=...)"
	)


def derivative_callable(name: str, **kwargs) -> Callable:
	"""The derivative of the built-in spectral function `name` (special.param_callable, same parameters and defaults) as a
	callable on arrays: what the Chebyshev route expands when `dfun` is not given. ValueError for the built-ins that have no
	derivative worth expanding (abs, numrank, softsign: give `dfun`)."""
	if name == "identity":
		return lambda x: np.ones_like(np.asarray(x, dtype=np.float64))
	if name == "sqrt":
		return lambda x: 0.5 / np.sqrt(x)
	if name == "log":  # (log is evaluated as log(max(x, eps)): flat below eps)
		return lambda x: np.where(np.asarray(x) > _EPS64, 1.0 / np.maximum(x, _EPS64), 0.0)
	if name == "inv":
		return lambda x: -1.0 / np.square(x)
	if name == "exp":
		t = float(kwargs.get("t", 1.0))
		return lambda x: t * np.exp(t * np.asarray(x))
	if name == "smoothstep":
		a, b = float(kwargs.get("a", 0.0)), float(kwargs.get("b", 1.0))
		width = (b - a) if a != b else 1.0

		def d(x):
			y = (np.asarray(x, dtype=np.float64) - a) / width
			return np.where((y > 0.0) & (y < 1.0), 6.0 * y * (1.0 - y) / width, 0.0)

		return d
	if name in ("abs", "numrank", "step", "softsign"):
		raise ValueError(f"'{name}' has no derivative in the table: give dfun= (a callable, or the built-in name of the derivative)")
	raise ValueError(f"Unknown function: {name}.")


DERIVATIVE_NAMES = ("identity", "sqrt", "log", "inv", "exp", "smoothstep")


def _probe_loader(pdf, seed, probes, n: int, count: int, chebyshev: bool):
	"""load(plan, done, m): probes [done, done + m) into `plan`; calling it again for the same `done` loads the same probes
	(the Chebyshev route runs a batch again after widening automatic bounds)."""
	from ._capi import PDF_IDS
	from .random import _ISO_DISTRIBUTIONS, isotropic

	if probes is not None:
		V = np.asarray(probes, dtype=np.float64)
		if V.ndim != 2 or V.shape != (n, count):
			raise ValueError(f"probes must be an n x count = {n} x {count} matrix, got {V.shape}")
		return lambda plan, done, m: plan.set_probes(np.asfortranarray(V[:, done : done + m]))
	if not isinstance(pdf, str):
		raise ValueError("pdf must be a distribution name or 'device:<name>' (or give probes=)")
	dev = pdf.startswith("device:")
	name = pdf[len("device:"):] if dev else pdf
	if name not in (PDF_IDS if dev else _ISO_DISTRIBUTIONS):
		raise ValueError(f"Invalid distribution '{pdf}' supplied.")
	rng = np.random.default_rng(seed)
	if dev:
		if chebyshev and name == "sphere":
			raise ValueError(
				"device:sphere probes are stored as the normal draw g and used as sqrt(n) g / ||g||: the Chebyshev action reads the "
				"stored vectors (slq_plan_chebyshev_action). Use pdf='sphere' (a host draw) or another device pdf"
			)
		dev_seed = int(seed) if isinstance(seed, (int, np.integer)) else int(rng.integers(0, 2**62))
		return lambda plan, done, m: plan.generate_probes(name, seed=dev_seed, probe_offset=done)
	draw = isotropic(pdf=pdf, seed=rng)
	last = {}

	def load(plan, done, m):
		if last.get("done") != done:
			last["done"], last["X"] = done, draw(size=(n, m)).astype(np.float64, copy=False)
		plan.set_probes(last["X"])

	return load


def _own_pattern(M):
	import scipy.sparse as sp

	A = getattr(M, "_A", None)
	if sp.issparse(A) or engine._is_torch_csr(A):
		return A
	raise ValueError("pattern= is required: the operator of M has no sparse entries of its own (give the sparsity pattern the gradient is wanted on)")


def _pattern_rows_cols(pattern) -> tuple:
	if engine._is_torch_csr(pattern):
		indptr, indices = pattern.crow_indices().cpu().numpy(), pattern.col_indices().cpu().numpy()
	else:
		indptr, indices = pattern.indptr, pattern.indices
	return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)), np.asarray(indices)


def trace_grad(M, pdf: Union[str, None] = "rademacher", count: int = 256, batch: int = 64, seed=None, probes=None, pattern=None,
			   symmetric: bool = True, dfun=None, keep_device: bool = False, **dfun_kwargs) -> tuple:  # fmt: skip
	"""(est, grad, info): the Girard-Hutchinson estimate of tr f(A) over `count` probes and, from the same runs, of its gradient
	f'(A) on the stored entries of `pattern`, aligned with `pattern.data` (`pattern.values()` for a torch CSR tensor) entry for
	entry. M: a MatrixFunction with a built-in `fun` (log, exp, identity; fp64) or a ChebyshevFunction.
	pattern=None: the sparse matrix M was built on, as given when it is CSR (any other SciPy format: its `.tocsr()`). A dense,
	plugin or callback operator needs `pattern`.
	probes: an explicit n x count host matrix instead of a pdf (E[v v^T] = I is the caller's business). pdf "device:<name>" draws
	on the GPU as in `hutch`.
	symmetric (default): the symmetric part 0.5 (G + G^T) on the pattern - what a symmetric A can see, at the same cost in
	launches and twice the panel traffic.
	dfun (ChebyshevFunction only): the derivative of M's function, a callable on arrays or a built-in name (dfun_kwargs: its
	parameters); default: the table `derivative_callable` for M's built-in function. Its coefficients on M.bounds, at M's degree
	and damping, drive ONE action run per batch; the value comes from the moments that run leaves behind.
	info: count, quad (the per-probe quadratic forms v_i^T f(A) v_i), acc_count (columns the accumulator folded in; 0 where the
	gradient needed no sampling), and with keep_device=True and a sampled gradient `accumulator` (the open
	engine.SddmmAccumulator that holds `grad` on the device; the caller closes it)."""
	from .chebyshev import ChebyshevFunction
	from .operators import MatrixFunction

	if not isinstance(M, (MatrixFunction, ChebyshevFunction)):
		raise ValueError("trace_grad takes a MatrixFunction or a ChebyshevFunction")
	if getattr(getattr(M, "_A", None), "_slq_kind", None) == "kernel_precond" or getattr(getattr(M, "_op", None), "kind", None) == "kernel_precond":
		raise ValueError("trace_grad: a preconditioned kernel operator has no stored entries: the hyperparameter gradients through the preconditioner are gp.logdet_grad's")
	if getattr(getattr(M, "_A", None), "_slq_kind", None) == "kernel" or getattr(getattr(M, "_op", None), "kind", None) == "kernel":
		raise ValueError("trace_grad: a KernelOperator has no stored entries; its hyperparameter gradients come from kernel_trace_grad")
	if np.dtype(M.dtype) != np.float64:
		raise ValueError("trace_grad is fp64 only (the device matrices are fp64): build M with dtype=np.float64")
	count, batch = int(count), int(batch)
	if count < 1 or batch < 1:
		raise ValueError(f"count = {count} and batch = {batch} must be >= 1")
	n = int(M.shape[0])
	cheb = isinstance(M, ChebyshevFunction)
	if probes is not None:
		count = int(np.asarray(probes).shape[1]) if np.asarray(probes).ndim == 2 else count
	exact = False
	if cheb:
		spec = getattr(M._fun, "_slq_builtin", None)
		if dfun is None:
			if spec is None:
				raise ValueError("M's function is a callable: give its derivative as dfun=")
			dcall = derivative_callable(spec[0], **spec[1])
		elif isinstance(dfun, str):
			engine.fun_spec(dfun, **dfun_kwargs)
			dcall = param_callable(dfun, **dfun_kwargs)
		elif callable(dfun):
			dcall = dfun
		else:
			raise ValueError("dfun must be a callable or a built-in function name")
	else:
		if dfun is not None or dfun_kwargs:
			raise ValueError("dfun belongs to the Chebyshev route: a MatrixFunction's derivative comes from the built-in table")
		if M._builtin is None:
			raise ValueError("trace_grad needs a built-in `fun` on the Lanczos route: for a callable use ChebyshevFunction(A, f, ...) with dfun=")
		if M._stale_ring or M._adaptive is not None:
			raise ValueError("trace_grad runs fixed-degree lock-step batches: no stale_ring, no adaptive degree")
		name, kw = M._builtin
		der = lanczos_derivative(name, kw)
		exact = der is None
	load = _probe_loader(pdf, seed, probes, n, count, cheb)
	if pattern is None:
		pattern = _own_pattern(M)
	if not engine._is_torch_csr(pattern):
		import scipy.sparse as sp

		if not sp.issparse(pattern):
			raise ValueError("pattern must be a SciPy sparse matrix or a torch sparse-CSR tensor on the GPU")
		pattern = pattern if pattern.format == "csr" else pattern.tocsr()
	if tuple(pattern.shape) != (n, n):
		raise ValueError(f"the pattern is {tuple(pattern.shape)}, the operator {n} x {n}")

	ctx = M._op.ctx
	acc = engine.SddmmAccumulator(pattern, ctx=ctx)
	W = Z = None
	quad = np.empty(count)
	try:
		cols = min(batch, count)
		if not exact:
			W, Z = engine.DeviceMatrix(n, cols, ctx=ctx), engine.DeviceMatrix(n, cols, ctx=ctx)
		done = 0
		while done < count:
			m = min(batch, count - done)
			if cheb:
				quad[done : done + m] = _chebyshev_batch(M, dcall, load, done, m, W, Z)
				scale = 1.0
			else:
				plan = M._plan(m, not exact)
				load(plan, done, m)
				if not exact:
					plan.get_probes_into(W, 0)
				plan.run(M._rtol)
				quad[done : done + m] = plan.quadrature(name, **kw)
				if not exact:
					plan.fun_action_into(Z, 0, der[0], **der[1])
					scale = der[2]
			if not exact:
				acc.update(Z, 0, W, 0, m, alpha=scale / count, beta=1.0, symmetric=symmetric)
			done += m
		info = dict(count=count, quad=quad)
		if exact:  # f' = 1: the gradient is the identity on the pattern
			rows, cols_ = _pattern_rows_cols(pattern)
			grad = (rows == cols_).astype(np.float64)
			info["acc_count"] = 0
		else:
			grad, info["acc_count"] = acc.get()
			if keep_device:
				info["accumulator"], acc = acc, None
		return float(np.mean(quad)), grad, info
	finally:
		for d in (W, Z, acc):
			if d is not None:
				d.close()


def _kernel_grads(K, vals: np.ndarray) -> dict:
	"""The d + 2 values of a KernelGradAccumulator as a dict shaped like K's parameters (a scalar lengthscale's gradient is the sum
	over the dimensions, taken on the host)."""
	d = K.X.shape[1]
	ls = np.array(vals[:d], dtype=np.float64)
	if np.size(K.lengthscale) == 1:
		ls = np.array([ls.sum()])
	return dict(lengthscale=ls.reshape(np.shape(K.lengthscale)), outputscale=float(vals[d]), noise=float(vals[d + 1]))


def kernel_trace_grad(M, pdf: Union[str, None] = "rademacher", count: int = 256, batch: int = 64, seed=None, probes=None, points: bool = False) -> tuple:
	"""(est, grads, info): the Girard-Hutchinson estimate of tr f(A) over `count` probes for A = the KernelOperator under M and, from
	the same runs, of its gradient with respect to the hyperparameters:

	    grads = dict(lengthscale=array shaped like K.lengthscale, outputscale=float, noise=float),

	the estimate (1/N) sum_i (f'(A) v_i)^T (dA/dtheta) v_i, contracted on the device against tiles of dA/dtheta that are never held
	(engine.KernelGradAccumulator). The gradient is that of the smooth formula at the operator's rounded points z. points=True: a
	second accumulator (engine.KernelPointGradAccumulator) is updated at the same places with the same factors and
	weights and grads["points"] is the n x d gradient with respect to the points X; with False every number keeps its bits. The
	Chebyshev route has no point gradient and refuses points=True. M: a MatrixFunction with a built-in `fun` among log, exp, identity (fp64), or a ChebyshevFunction
	with a built-in function of the table `derivative_callable`. The batch loop is `trace_grad`'s. identity is exact and runs
	nothing: tr A = n (outputscale + noise), gradients 0, n, n.
	info: count, quad (the per-probe quadratic forms; for identity the exact trace in every entry), acc_count (columns the
	accumulator folded in; 0 where nothing was sampled)."""
	from .chebyshev import ChebyshevFunction
	from .operators import MatrixFunction

	if not isinstance(M, (MatrixFunction, ChebyshevFunction)):
		raise ValueError("kernel_trace_grad takes a MatrixFunction or a ChebyshevFunction")
	K = getattr(M, "_A", None)
	if getattr(K, "_slq_kind", None) == "kernel_precond":
		raise ValueError("kernel_trace_grad: the function of a preconditioned operator is not differentiated here: the gradient of logdet A through the pivoted-Cholesky preconditioner is gp.logdet_grad (gp.mll for the marginal likelihood)")
	if getattr(K, "_slq_kind", None) != "kernel":
		raise ValueError("kernel_trace_grad needs a function of a KernelOperator (for the gradient on a sparsity pattern use trace_grad)")
	from .operators import refuse_diag_scale

	refuse_diag_scale(K, "kernel_trace_grad")
	if np.dtype(M.dtype) != np.float64 or np.dtype(K.dtype) != np.float64:
		raise ValueError("kernel_trace_grad is fp64 only (the device matrices are fp64): build the KernelOperator and M with dtype=np.float64")
	count, batch = int(count), int(batch)
	if count < 1 or batch < 1:
		raise ValueError(f"count = {count} and batch = {batch} must be >= 1")
	n = int(M.shape[0])
	cheb = isinstance(M, ChebyshevFunction)
	if points and cheb:
		raise ValueError("kernel_trace_grad: points=True is not built on the Chebyshev route: use a MatrixFunction (Lanczos) for the gradient with respect to the points")
	if probes is not None:
		count = int(np.asarray(probes).shape[1]) if np.asarray(probes).ndim == 2 else count
	exact = False
	if cheb:
		spec = getattr(M._fun, "_slq_builtin", None)
		if spec is None:
			raise ValueError("kernel_trace_grad needs a built-in function on the Chebyshev route (its derivative comes from the table)")
		dcall = derivative_callable(spec[0], **spec[1])
	else:
		if M._builtin is None:
			raise ValueError("kernel_trace_grad needs a built-in `fun` on the Lanczos route (log, exp, identity)")
		if M._stale_ring or M._adaptive is not None:
			raise ValueError("kernel_trace_grad runs fixed-degree lock-step batches: no stale_ring, no adaptive degree")
		name, kw = M._builtin
		der = lanczos_derivative(name, kw)
		exact = der is None
	load = _probe_loader(pdf, seed, probes, n, count, cheb)
	if exact:
		d = K.X.shape[1]
		tr = float(n) * (K.outputscale + K.noise)
		grads = _kernel_grads(K, np.concatenate([np.zeros(d), [float(n), float(n)]]))
		if points:  # (tr A does not depend on the points)
			grads["points"] = np.zeros((n, d))
		return tr, grads, dict(count=count, quad=np.full(count, tr), acc_count=0)

	ctx = M._op.ctx
	acc = engine.KernelGradAccumulator(M._op)
	W = Z = pacc = None
	quad = np.empty(count)
	try:
		if points:
			pacc = engine.KernelPointGradAccumulator(M._op)
		cols = min(batch, count)
		W, Z = engine.DeviceMatrix(n, cols, ctx=ctx), engine.DeviceMatrix(n, cols, ctx=ctx)
		done = 0
		while done < count:
			m = min(batch, count - done)
			if cheb:
				quad[done : done + m] = _chebyshev_batch(M, dcall, load, done, m, W, Z)
				scale = 1.0
			else:
				plan = M._plan(m, True)
				load(plan, done, m)
				plan.get_probes_into(W, 0)
				plan.run(M._rtol)
				quad[done : done + m] = plan.quadrature(name, **kw)
				plan.fun_action_into(Z, 0, der[0], **der[1])
				scale = der[2]
			acc.update(Z, 0, W, 0, m, alpha=scale / count, beta=1.0)
			if pacc is not None:
				pacc.update(Z, 0, W, 0, m, alpha=scale / count, beta=1.0)
			done += m
		vals, acc_count = acc.get()
		grads = _kernel_grads(K, vals)
		if pacc is not None:
			grads["points"] = pacc.get()[0]
		return float(np.mean(quad)), grads, dict(count=count, quad=quad, acc_count=acc_count)
	finally:
		for dm in (W, Z, acc, pacc):
			if dm is not None:
				dm.close()


def kernel_quadratic_grad(K, U, V=None) -> dict:
	"""The gradient of sum_c u_c^T A v_c with respect to the hyperparameters of the KernelOperator K (fp64), for host arrays U, V
	(n x m or n; V=None: V = U), shaped as `kernel_trace_grad`'s: with U = V = A^-1 y and a factor -1 the data-fit term y^T A^-1 y of
	a marginal likelihood. One KernelGradAccumulator update on K's device operator."""
	from .lanczos import _as_device_operator

	if getattr(K, "_slq_kind", None) == "kernel_precond":
		raise ValueError("kernel_quadratic_grad: pass the base KernelOperator, not its preconditioner (the data-fit gradient of a marginal likelihood through the preconditioner is part of gp.mll; gp.logdet_grad has the log-determinant's)")
	if getattr(K, "_slq_kind", None) != "kernel":
		raise ValueError("kernel_quadratic_grad needs a KernelOperator")
	from .operators import refuse_diag_scale

	refuse_diag_scale(K, "kernel_quadratic_grad")
	if np.dtype(K.dtype) != np.float64:
		raise ValueError("kernel_quadratic_grad is fp64 only (the device matrices are fp64): build the KernelOperator with dtype=np.float64")
	n = int(K.shape[0])
	U = np.asarray(U, dtype=np.float64)
	U = U.reshape(-1, 1) if U.ndim == 1 else U
	Vh = U if V is None else np.asarray(V, dtype=np.float64)
	Vh = Vh.reshape(-1, 1) if Vh.ndim == 1 else Vh
	if U.ndim != 2 or U.shape[0] != n or Vh.shape != U.shape or U.shape[1] < 1:
		raise ValueError(f"U and V must be n x m = {n} x m arrays of one shape, got {U.shape} and {Vh.shape}")
	op = _as_device_operator(K, dtype=np.float64)
	m = U.shape[1]
	acc = Ud = Vd = None
	try:
		acc = engine.KernelGradAccumulator(op)
		Ud = engine.DeviceMatrix(n, m, ctx=op.ctx)
		Ud.set(0, U)
		if V is None:
			Vd = Ud
		else:
			Vd = engine.DeviceMatrix(n, m, ctx=op.ctx)
			Vd.set(0, Vh)
		acc.update(Ud, 0, Vd, 0, m, alpha=1.0, beta=0.0)
		return _kernel_grads(K, acc.get()[0])
	finally:
		for dm in {id(x): x for x in (Ud, Vd, acc) if x is not None}.values():
			dm.close()


def kernel_point_grad(K, U, V=None, Xnew=None) -> np.ndarray:
	"""The gradient of sum_c u_c^T A v_c with respect to the points of the KernelOperator K (fp64): n x d, shaped like K.X, for host
	arrays U, V (n x m or n; V=None: V = U). With `Xnew` (m* x d): the gradient of sum_c u_c^T K(Xnew, X) v_c with respect to the NEW
	points, m* x d - U (m* x b) on the new points, V (n x b, required) on the training points. The smooth formula at the operator's
	rounded points. One KernelPointGradAccumulator update on K's device operator."""
	from .lanczos import _as_device_operator

	if getattr(K, "_slq_kind", None) == "kernel_precond":
		raise ValueError("kernel_point_grad: pass the base KernelOperator, not its preconditioner")
	if getattr(K, "_slq_kind", None) != "kernel":
		raise ValueError("kernel_point_grad needs a KernelOperator")
	from .operators import refuse_diag_scale

	if Xnew is None:  # (the cross form is defined on K0's points and profile, as a cross product is: it ignores the scale)
		refuse_diag_scale(K, "kernel_point_grad")
	if np.dtype(K.dtype) != np.float64:
		raise ValueError("kernel_point_grad is fp64 only (the device matrices are fp64): build the KernelOperator with dtype=np.float64")
	n = int(K.shape[0])
	U = np.asarray(U, dtype=np.float64)
	U = U.reshape(-1, 1) if U.ndim == 1 else U
	if Xnew is not None and V is None:
		raise ValueError("kernel_point_grad: with Xnew, U is on the new points and V on the training points: V is required")
	Vh = U if V is None else np.asarray(V, dtype=np.float64)
	Vh = Vh.reshape(-1, 1) if Vh.ndim == 1 else Vh
	op = _as_device_operator(K, dtype=np.float64)
	acc = Ud = Vd = cross = None
	try:
		if Xnew is not None:
			cross = engine.KernelCross(op, Xnew)
			rows = cross.m
		else:
			rows = n
		if U.ndim != 2 or Vh.ndim != 2 or U.shape[0] != rows or Vh.shape[0] != n or U.shape[1] != Vh.shape[1] or U.shape[1] < 1:
			raise ValueError(f"U must be {rows} x m and V {n} x m, got {U.shape} and {Vh.shape}")
		m = U.shape[1]
		acc = engine.KernelPointGradAccumulator(cross if cross is not None else op)
		Ud = engine.DeviceMatrix(rows, m, ctx=op.ctx)
		Ud.set(0, U)
		if V is None:
			Vd = Ud
		else:
			Vd = engine.DeviceMatrix(n, m, ctx=op.ctx)
			Vd.set(0, Vh)
		acc.update(Ud, 0, Vd, 0, m, alpha=1.0, beta=0.0)
		return acc.get()[0]
	finally:
		for dm in {id(x): x for x in (acc, Ud, Vd, cross) if x is not None}.values():
			dm.close()


def _chebyshev_batch(M, dcall: Callable, load: Callable, done: int, m: int, W, Z) -> np.ndarray:
	"""One action run for the batch: Z = p'(A) V with the coefficients of f' on M.bounds, the probes in W, and the quadratic forms
	from the moments that run leaves; the automatic-bounds retry of ChebyshevFunction._action."""
	from .chebyshev import BOUNDS_RETRIES, chebyshev_coefficients

	plan = M._action_plan(m)
	if M._coef is None:
		M._set_bounds()
	for attempt in range(BOUNDS_RETRIES + 1):
		dcoef = chebyshev_coefficients(dcall, M._deg + 1, M.bounds, M._damping)
		load(plan, done, m)
		plan.get_probes_into(W, 0)
		try:
			plan.action_into(M.bounds, dcoef, Z, 0)
			return plan.moment_sum(M._coef)
		except ValueError:
			if plan.bounds != M.bounds:  # (refused before the run)
				raise
			_, flags = plan.moments(return_outside=True)
			if not flags.any():
				raise
			if M._given is not None:
				raise ValueError(f"the spectrum of A is not inside bounds = {M.bounds}: {int(flags.sum())} of {m} columns saw a moment above mu_0") from None
			if attempt == BOUNDS_RETRIES:
				raise ValueError(f"the spectrum of A is not inside the automatic bounds {M.bounds} after {BOUNDS_RETRIES} widenings: give bounds=") from None
			M._extra = max(2.0 * M._extra, 2.0 * M._margin)
			M._set_bounds()
	raise AssertionError("unreachable")
