"""Gaussian-process prediction, log-determinants, the marginal likelihood with its gradients and posterior function samples on the
matrix-free kernel operator, fixed per-point noise and the Laplace approximation (§4.23).

With A = K + noise I the operator of a `KernelOperator` on the training points X, C = outputscale * phi(r2(X*, X)) the
cross-covariance to new points X* (`KernelOperator.cross`, engine.KernelCross) and s the outputscale,

    mean = C A^-1 y,        var_i = s - (C A^-1 C^T)_ii.

With a pivoted-Cholesky preconditioner (`KernelOperator.preconditioned`, §4.18) M = P^{-1/2} and B = M A M,

    logdet A = tr log B + logdet P,        A^-1 y = M B^-1 M y,

which is what `logdet` computes and what `posterior(precond_rank > 0)` solves with: the path for small noise, where Lanczos on A
itself does not converge in any affordable number of steps.

`logdet_grad` and `mll` (§4.19) differentiate through the same split: tr(A^-1 dA/dtheta) = tr(P^-1 dA/dtheta), exact from the factor,
plus a sampled remainder on B. What they return is the gradient of logdet A and of the marginal likelihood themselves - an unbiased
estimate for any factor - NOT the derivative of the sampled value; the factor is never differentiated.

`fixed_noise_posterior` and `laplace` (§4.23) leave the single model A = K0 + noise I: known per-point noise K0 + diag(e) and the
B = I + W^{1/2} K0 W^{1/2} of a Laplace approximation (logit, poisson) are both the diagonally scaled operator s D K0 D + I
(`KernelOperator(diag_scale=)`), whose scale sits inside the matrix-free product. Every other entry here refuses a scaled operator.

Neither A nor C is ever formed: A^-1 is the Lanczos action `fun_action_into(..., "inv")` of a kept-basis plan over the device
operator, C and C^T are the cross-covariance products, and the contraction C A^-1 C^T of a batch is `DeviceMatrix.tn`.
"""

from __future__ import annotations

import contextlib
import time
from typing import Optional

import numpy as np

from . import engine
from .lanczos import _as_device_operator
from .operators import _kernel_profile, refuse_diag_scale


def _prior_block(K, zs: np.ndarray) -> np.ndarray:
	"""outputscale * phi(r2) among the scaled new points zs (m x d, float64): differences, exact zeros and so exactly s on the diagonal."""
	r2 = np.zeros((zs.shape[0], zs.shape[0]))
	for k in range(zs.shape[1]):
		diff = zs[:, k][:, None] - zs[:, k][None, :]
		r2 += diff * diff
	return K.outputscale * _kernel_profile(K.kernel, r2)


def _finite(a: np.ndarray, what: str, rtol: float) -> None:
	if not np.all(np.isfinite(a)):
		raise FloatingPointError(f"posterior: {what} is not finite" + (f" (rtol = {rtol} > 0 lets probes stop early, which the 'inv' action does not survive: use rtol = 0)" if rtol > 0 else ""))


def _solve_into(pop, plan, RHS, OUT, b: int, tmp, rtol: float = 0.0) -> None:
	"""OUT[:, :b] = A^-1 RHS[:, :b] by the kept-basis `plan`: on A's own operator (pop None), or on the preconditioned operator `pop`
	as M B^-1 M - M applied on the device to the right-hand sides before they become the plan's probes and to the action's result.
	tmp: two n x b DeviceMatrix of scratch for the preconditioned path."""
	if pop is None:
		plan.set_probes_device(RHS.col_ptr(0))
		plan.run(rtol)
		plan.fun_action_into(OUT, 0, "inv")
		return
	pop.inv_sqrt_dmat(RHS, 0, tmp[0], 0, b)
	plan.set_probes_device(tmp[0].col_ptr(0))
	plan.run(rtol)
	plan.fun_action_into(tmp[1], 0, "inv")
	pop.inv_sqrt_dmat(tmp[1], 0, OUT, 0, b)


def logdet(K, rank: int = 100, deg: int = 20, count: int = 64, batch: int = 64, pdf: str = "device:rademacher", seed=None) -> tuple:
	"""(estimate, info): log det A of the KernelOperator `K` (A = K0 + noise I, float64) by stochastic Lanczos quadrature on the
	preconditioned operator: `hutch` over `MatrixFunction(K.preconditioned(rank), "log", deg)` with `count` probes in equal batches
	of at most `batch` (whole batches are drawn: `count` is rounded up to ceil(count / batch) of them, info says how many), plus logdet P of the factor (exact, from its r x r Gram matrix). rank = 0: the plain estimate on A itself.
	info: rank (the factor's; 0 for the plain estimate), logdet_precond, trace (the stochastic part), std_error (of the estimate:
	the sample standard deviation of the per-probe values over sqrt(count)), count, deg."""
	from .operators import MatrixFunction
	from .trace import hutch

	if getattr(K, "_slq_kind", None) != "kernel":
		raise ValueError("logdet needs a KernelOperator")
	refuse_diag_scale(K, "gp.logdet")
	if np.dtype(K.dtype) != np.float64:
		raise ValueError(f"logdet is fp64 only: the KernelOperator is {np.dtype(K.dtype)}")
	rank, deg, count, batch = int(rank), int(deg), int(count), int(batch)
	if rank < 0 or deg < 1 or count < 2 or batch < 1:
		raise ValueError(f"rank = {rank} must be >= 0, deg = {deg} and batch = {batch} >= 1, count = {count} >= 2")
	B = K.preconditioned(rank) if rank > 0 else K
	M = MatrixFunction(B, fun="log", deg=deg, dtype=np.float64)
	pinfo = dict(rank=0, logdet_p=0.0)
	if rank > 0:
		pinfo = _as_device_operator(B, dtype=np.float64).info()
	nb = -(-count // batch)
	batch = -(-count // nb)  # whole batches of equal size: nb * batch probes, count rounded up by less than nb
	est, res = hutch(M, batch=batch, pdf=pdf, converge="count", count=count, seed=seed, full=True, record=True)
	vals = np.asarray(res.estimator.values, dtype=np.float64).ravel()
	info = dict(rank=int(pinfo["rank"]), logdet_precond=float(pinfo["logdet_p"]), trace=float(est), count=int(vals.size), deg=deg,
				std_error=float(np.std(vals, ddof=1) / np.sqrt(vals.size)))  # fmt: skip
	return float(est) + float(pinfo["logdet_p"]), info


def posterior(K, y, Xnew, deg: int = 60, orth: Optional[int] = None, rtol: float = 0.0, variance: bool = True, batch: int = 128,
			  covariance: bool = False, include_noise: bool = False, precond_rank: int = 0) -> tuple:  # fmt: skip
	"""(mean, var, info): the posterior of a Gaussian process with the kernel operator `K` (a `KernelOperator` in float64; its
	noise is the observation noise) and zero prior mean, given observations `y` ((n,) or (n, q)) at K's points, at the new points
	`Xnew` (m x d; NumPy, or a torch tensor on the context's GPU).

	mean: (m,) or (m, q), C A^-1 y. alpha = A^-1 y comes from ONE kept-basis Lanczos plan of `deg` steps (`orth` vectors of
	re-orthogonalisation, None: all) over K's device operator, written by `fun_action_into(..., "inv")` into a DeviceMatrix; the
	mean is the forward cross product of it. `rtol` is the early-stop threshold of `LanczosPlan.run`, 0 by default: every probe
	takes all `deg` steps. The "inv" action has no value for a probe that stopped early - the Ritz values of the steps it did not
	take are 0 - and a smooth kernel with noise exhausts its Krylov space in a few dozen steps, so a positive rtol is for operators
	known not to; a result that is not finite raises FloatingPointError and says so.
	var: (m,), s - diag(C A^-1 C^T) (None with variance=False), the variance of the latent function; include_noise=True adds K.noise,
	the variance of a new observation. It is computed per batch of at most `batch` new points: B = C^T I (the adjoint product on a
	cross object of the batch's points) is the probe block of a plan, `fun_action_into(Cv, "inv")` its solve, `B.tn(Cv)` the batch's
	m_b x m_b block on the host. covariance=True (only for m <= batch) returns instead of var the m x m posterior covariance
	s phi(X*, X*) - block, the block symmetrised (it is symmetric up to rounding); its diagonal is `var`.
	Nothing of size n leaves the device: only the mean's m x q and the m_b x m_b blocks do.

	Columns of norm 0. A new point so far from the data that its column of B is exactly zero (phi has underflowed against every
	training point) has no information: mean = 0 and var = s, exactly. A Lanczos run cannot start from a zero vector, so such
	columns never reach the plan: the batch's Gram matrix B^T B (one more m_b x m_b product) names them, each is overwritten on the
	device with a copy of a non-zero column of the batch (a batch with none runs no plan at all), and their rows and columns of the
	block are set to 0 afterwards - no other column can see a NaN from them. A zero column of `y` is treated the same way and has
	mean 0.

	precond_rank > 0: every solve is M B^-1 M on the preconditioned operator B = M A M of `K.preconditioned(precond_rank)` (§4.18) -
	M is applied on the device to the right-hand sides before they become a plan's probes and to the action's result - so that
	`deg` steps suffice at small noise. 0 (the default) is the plain path on A.

	info: deg, batches (variance batches run), steps (the Lanczos steps each plan took: first the solve for alpha, then one entry
	per batch), zero_columns (indices of the new points whose column of B was zero)."""
	return _posterior(K, y, Xnew, deg, orth, rtol, variance, batch, covariance, include_noise, precond_rank, False)[:3]


def _posterior(K, y, Xnew, deg, orth, rtol, variance, batch, covariance, include_noise, precond_rank, grad: bool, who: str = "posterior") -> tuple:
	"""(mean, var, info, dmean, dvar): `posterior` behind its docstring; with `grad` also `posterior_grad`'s two arrays, from point-gradient
	updates placed after the solves they read. Without it not one device call is added or moved: posterior's bits are what they were."""
	if getattr(K, "_slq_kind", None) != "kernel":
		raise ValueError(f"{who} needs a KernelOperator")
	refuse_diag_scale(K, f"gp.{who}")
	if np.dtype(K.dtype) != np.float64:
		raise ValueError(f"{who} is fp64 only (the device matrices are fp64): the KernelOperator is {np.dtype(K.dtype)}")
	n, d = K.X.shape
	deg, batch = int(deg), int(batch)
	if deg < 1 or batch < 1:
		raise ValueError(f"deg = {deg} and batch = {batch} must be >= 1")
	yh = np.asarray(y, dtype=np.float64)
	vector = yh.ndim == 1
	yh = yh.reshape(-1, 1) if vector else yh
	if yh.ndim != 2 or yh.shape[0] != n or yh.shape[1] < 1:
		raise ValueError(f"y must be ({n},) or ({n}, q), got shape {np.asarray(y).shape}")
	if not np.all(np.isfinite(yh)):
		raise ValueError("y must be finite")
	Cop = K.cross(Xnew)  # (checks the shape and the values of the new points)
	m = Cop.Xnew.shape[0]
	if covariance and not variance:
		raise ValueError("covariance=True needs variance=True")
	if covariance and m > batch:
		raise ValueError(f"covariance=True needs all m = {m} new points in one batch (batch = {batch})")
	orth_arg = -1 if orth is None else int(orth)
	s = float(K.outputscale)

	op = _as_device_operator(K, dtype=np.float64)
	ctx = op.ctx
	q = yh.shape[1]
	live = []  # device objects, closed in reverse order whatever happens
	precond_rank = int(precond_rank)
	if precond_rank < 0:
		raise ValueError(f"precond_rank = {precond_rank} must be >= 0")
	## the operator the plans run on: A itself, or B = M A M (the cross products stay on A's operator)
	pop = _as_device_operator(K.preconditioned(precond_rank), dtype=np.float64) if precond_rank > 0 else None
	solve_op = op if pop is None else pop

	def solve_into(plan, RHS, OUT, b, tmp):
		_solve_into(pop, plan, RHS, OUT, b, tmp, rtol)

	def keep(obj):
		live.append(obj)
		return obj

	info = dict(deg=min(deg, n), batches=0, steps=[], zero_columns=[])
	try:
		## alpha = A^-1 y over the non-zero columns of y, mean = C alpha
		nz = np.flatnonzero(np.any(yh != 0.0, axis=0))
		mean = np.zeros((m, q))
		dmean = np.zeros((m, d, q)) if grad else None
		dvar = np.zeros((m, d)) if grad and variance else None
		if nz.size:
			plan = keep(engine.LanczosPlan(solve_op, int(nz.size), deg, orth_arg, basis="keep"))
			Alpha = keep(engine.DeviceMatrix(n, int(nz.size), ctx=ctx))
			if pop is None:
				plan.set_probes(np.asfortranarray(yh[:, nz]))
				plan.run(rtol)
				plan.fun_action_into(Alpha, 0, "inv")
			else:
				Yd, t0, t1 = (keep(engine.DeviceMatrix(n, int(nz.size), ctx=ctx)) for _ in range(3))
				Yd.set(0, np.asfortranarray(yh[:, nz]))
				solve_into(plan, Yd, Alpha, int(nz.size), (t0, t1))
			info["steps"].append(plan.steps_done)
			cross = keep(Cop.device(op))
			Mean = keep(engine.DeviceMatrix(m, int(nz.size), ctx=ctx))
			cross.matmat_dmat(Alpha, 0, Mean, 0, int(nz.size))
			mean[:, nz] = Mean.get()
			_finite(mean, "the mean", rtol)
			if grad:  # d mean_q / d x*: the cross form with U a column of ones and W = alpha_q, one column at a time
				pacc, Ones = keep(engine.KernelPointGradAccumulator(cross)), keep(engine.DeviceMatrix(m, 1, ctx=ctx))
				Ones.set(0, np.ones((m, 1)))
				for c, col in enumerate(nz):
					pacc.update(Ones, 0, Alpha, c, 1, alpha=1.0, beta=0.0)
					dmean[:, :, col] = pacc.get()[0]
				_finite(dmean, "the gradient of the mean", rtol)
				for obj in (pacc, Ones):
					obj.close()
			for obj in (Mean, cross, Alpha, plan):
				obj.close()
		mean = mean[:, 0] if vector else mean
		if grad:
			dmean = dmean[:, :, 0] if vector else dmean
		if not variance:
			return mean, None, info, dmean, None

		mb_max = min(batch, m)
		B, Cv = keep(engine.DeviceMatrix(n, mb_max, ctx=ctx)), keep(engine.DeviceMatrix(n, mb_max, ctx=ctx))
		tmp = tuple(keep(engine.DeviceMatrix(n, mb_max, ctx=ctx)) for _ in range(2)) if pop is not None else None
		plans = {}
		quad = np.zeros(m)
		block_full = None
		for i0 in range(0, m, batch):
			i1 = min(m, i0 + batch)
			mb = i1 - i0
			crossb = keep(engine.KernelCross(op, Cop.Xnew[i0:i1]))
			Eye = keep(engine.DeviceMatrix(mb, mb, ctx=ctx))
			Eye.set(0, np.eye(mb))
			crossb.matmat_dmat(Eye, 0, B, 0, mb, trans=True)  # B = C_b^T: the batch's k* as columns
			zero = np.flatnonzero(np.diag(B.tn(0, mb, B, 0, mb)) == 0.0)
			good = np.setdiff1d(np.arange(mb), zero)
			block = np.zeros((mb, mb))
			if good.size:
				for j in zero:  # (a stand-in the plan can run on; its results are dropped below)
					B.copy_from(int(j), B, int(good[0]), 1)
				if mb not in plans:
					plans[mb] = keep(engine.LanczosPlan(solve_op, mb, deg, orth_arg, basis="keep"))
				solve_into(plans[mb], B, Cv, mb, tmp)
				info["steps"].append(plans[mb].steps_done)
				block = B.tn(0, mb, Cv, 0, mb)
				_finite(block, f"the variance block of the new points [{i0}, {i1})", rtol)
				block[zero, :] = 0.0
				block[:, zero] = 0.0
				if grad:  # d var_a / d x*_a = -2 (d k_a / d x*_a)^T A^-1 k_a: U = I picks column a of Cv = A^-1 C_b^T for row a
					paccb = keep(engine.KernelPointGradAccumulator(crossb))
					paccb.update(Eye, 0, Cv, 0, mb, alpha=-2.0, beta=0.0)
					dv = paccb.get()[0]
					_finite(dv, f"the gradient of the variance of the new points [{i0}, {i1})", rtol)
					dv[zero, :] = 0.0
					dvar[i0:i1] = dv
					paccb.close()
			info["batches"] += 1
			info["zero_columns"].extend(int(i0 + j) for j in zero)
			quad[i0:i1] = np.diag(block)
			if covariance:
				block_full = 0.5 * (block + block.T)
			Eye.close()
			crossb.close()
		var = s - quad + (float(K.noise) if include_noise else 0.0)
		if covariance:
			cov = _prior_block(K, Cop.scaled_points().astype(np.float64)) - block_full
			if include_noise:
				cov[np.diag_indices(m)] += float(K.noise)
			return mean, cov, info, dmean, dvar
		return mean, var, info, dmean, dvar
	finally:
		for obj in reversed(live):
			obj.close()


def posterior_grad(K, y, Xnew, deg: int = 60, orth: Optional[int] = None, variance: bool = True, batch: int = 128, precond_rank: int = 0) -> tuple:
	"""(dmean, dvar, info): the gradients of `posterior`'s mean and variance with respect to the NEW points - what
	Bayesian optimisation differentiates. The solves are exactly `posterior`'s (same plans, same right-hand sides, same order; rtol = 0),
	and each gradient is a cross-form point-gradient update (engine.KernelPointGradAccumulator) on what a solve left on the device:

	    dmean[a, k]   = d mean_a / d x*_ak       (m x d, or m x d x q for y (n, q)): U a column of ones, W = alpha_q = A^-1 y_q
	    dvar[a, k]    = d var_a / d x*_ak = -2 R[a, k](U = I, W = A^-1 C_b^T) per batch of at most `batch` new points (None with
	                    variance=False); the prior variance s does not depend on the point.

	The derivative is that of the smooth formula at the rounded scaled points. A new point whose column of C^T is exactly zero has
	dvar = 0 exactly (its mean's gradient is 0 by the profile's own underflow); a zero column of y has dmean = 0. Nothing of size n
	leaves the device: only the m x d arrays do. There is no gradient in the TRAINING points here. info: `posterior`'s."""
	mean, var, info, dmean, dvar = _posterior(K, y, Xnew, deg, orth, 0.0, variance, batch, False, False, precond_rank, True, who="posterior_grad")
	return dmean, dvar, info


## ---- the gradient of logdet A through the preconditioner, and the marginal likelihood ---------------------------
CONTROL_VARIATE_RITZ_MAX = 2.0  # B >= I, and |1 / lam - 1| <= 1 / lam exactly when lam <= 2: beyond it subtracting w makes a probe's term larger


def control_variate_auto(ritz_max: float) -> bool:
	"""The `control_variate="auto"` rule: on iff the largest Ritz value of B over the probes of the first batch is at most 2."""
	return bool(ritz_max <= CONTROL_VARIATE_RITZ_MAX)


def ritz_max(alpha: np.ndarray, beta: np.ndarray, steps: np.ndarray) -> float:
	"""The largest eigenvalue of the Lanczos tridiagonals of `LanczosPlan.tridiag()` (alpha, beta: nprobes x (deg + 1), beta[:, 0] = 0;
	steps: the steps each probe took), on the host."""
	top = -np.inf
	for a, b, k in zip(np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64), np.asarray(steps).astype(int)):
		if k < 1:
			continue
		T = np.diag(a[:k]) + np.diag(b[1:k], 1) + np.diag(b[1:k], -1)
		top = max(top, float(np.linalg.eigvalsh(T)[-1]))
	return top


class _Phases:
	"""Wall time per named phase, each closed by a stream synchronisation (scripts/bench_gp_mll.py); off: no synchronisation at all."""

	def __init__(self, ctx, on: bool):
		self.ctx, self.on, self.ms = ctx, bool(on), {}

	def __call__(self, name: str):
		@contextlib.contextmanager
		def span():
			if not self.on:
				yield
				return
			self.ctx.synchronize()
			t = time.perf_counter()
			try:
				yield
			finally:
				self.ctx.synchronize()
				self.ms[name] = self.ms.get(name, 0.0) + 1e3 * (time.perf_counter() - t)

		return span()


def _kernel_and_precond(K, rank: int, who: str):
	"""(the base KernelOperator, the PreconditionedKernelOperator or None): K is either; a preconditioned operator brings its own rank."""
	kind = getattr(K, "_slq_kind", None)
	if kind == "kernel_precond":
		base, B = K.base, K
	elif kind == "kernel":
		base, B = K, (K.preconditioned(rank) if rank > 0 else None)
	else:
		raise ValueError(f"{who} needs a KernelOperator (or its preconditioned(rank))")
	refuse_diag_scale(base, f"gp.{who}")
	if np.dtype(base.dtype) != np.float64:
		raise ValueError(f"{who} is fp64 only: the KernelOperator is {np.dtype(base.dtype)}")
	return base, B


def _batches(count: int, batch: int, probes, n: int, who: str):
	"""(nb, batch, probes as float64 or None): whole batches of equal size, as `logdet` cuts them; explicit probes must fill them."""
	nb = -(-count // batch)
	batch = -(-count // nb)
	if probes is not None:
		V = np.asarray(probes, dtype=np.float64)
		if V.ndim != 2 or V.shape[0] != n or V.shape[1] != nb * batch:
			raise ValueError(f"{who}: probes must be an n x count array of whole batches ({n} x {nb * batch}), got {V.shape}")
		return nb, batch, V
	return nb, batch, None


def _logdet_grad(base, B, deg: int, count: int, batch: int, pdf, seed, probes, control_variate, phases=None, points: bool = False) -> tuple:
	"""(value, vals, info) with vals the d + 2 raw gradient values of logdet A; `logdet_grad` behind its argument checks (rank > 0).
	points: a point-gradient accumulator is updated at the same places with the same factors - the batches' weights 1 / (batch nb) summed
	on the device, the exact part on top - and info["points_values"] is its n x d (None without): one readback, at the end."""
	from .estimators import MeanEstimator
	from .grad import _probe_loader
	from .operators import MatrixFunction

	if control_variate not in ("auto", True, False):
		raise ValueError(f"control_variate = {control_variate!r} (one of 'auto', True, False)")
	n = int(base.shape[0])
	op = _as_device_operator(base, dtype=np.float64)
	pop = _as_device_operator(B, dtype=np.float64)  # (refreshes lazily when the base's hyperparameters have changed)
	ctx = op.ctx
	phases = phases or _Phases(ctx, False)
	nb, batch, V = _batches(count, batch, probes, n, "logdet_grad")
	total = nb * batch
	load = _probe_loader(pdf, seed, V, n, total, False)
	M = MatrixFunction(B, fun="log", deg=deg, dtype=np.float64)
	pinfo = pop.info()
	estimator = MeanEstimator(covariance=True, record=True)
	live = []
	try:
		acc = engine.KernelGradAccumulator(op)
		live.append(acc)
		pacc = None
		if points:
			pacc = engine.KernelPointGradAccumulator(op)
			live.append(pacc)
		W, Vm, T, U = (engine.DeviceMatrix(n, batch, ctx=ctx) for _ in range(4))
		live.extend((W, Vm, T, U))
		exact = None
		use_cv, top = (None if control_variate == "auto" else bool(control_variate)), None
		per_batch = []
		eye = np.eye(batch)
		for j in range(nb):
			with phases("lanczos"):
				plan = M._plan(batch, True)
				load(plan, j * batch, batch)
				plan.get_probes_into(W, 0)
				plan.run(M._rtol)
				estimator.update(plan.quadrature("log"))
				plan.fun_action_into(T, 0, "inv")
			if j == 0:  # the decision, before this batch's update; held for the whole call
				top = ritz_max(*plan.tridiag())
				if use_cv is None:
					use_cv = control_variate_auto(top)
			with phases("applies"):
				pop.inv_sqrt_dmat(W, 0, Vm, 0, batch)
				if use_cv:
					T.add_product(0, W, 0, eye, alpha=-1.0, beta=1.0)
				pop.inv_sqrt_dmat(T, 0, U, 0, batch)
			with phases("updates"):
				acc.update(U, 0, Vm, 0, batch, alpha=1.0 / batch, beta=0.0)
				per_batch.append(acc.get()[0])
			if pacc is not None:
				with phases("points"):
					pacc.update(U, 0, Vm, 0, batch, alpha=1.0 / (batch * nb), beta=0.0 if j == 0 else 1.0)
		if use_cv:
			with phases("exact"):
				pop.precond_trace_grad(acc, alpha=1.0, beta=0.0)
				exact = acc.get()[0]
			if pacc is not None:
				with phases("points"):
					pop.precond_trace_point_grad(pacc, alpha=1.0, beta=1.0)
		pvals = None
		if pacc is not None:
			with phases("points"):
				pvals = pacc.get()[0]
			if not np.all(np.isfinite(pvals)):
				raise FloatingPointError("logdet_grad: the sampled gradient in the points is not finite: a probe's Lanczos run stopped before `deg` steps: lower deg or rank")
		per_batch = np.array(per_batch)
		if not np.all(np.isfinite(per_batch)):
			raise FloatingPointError("logdet_grad: the sampled gradient is not finite: a probe's Lanczos run stopped before `deg` steps (B is so close to the identity that its Krylov space is exhausted), which the 'inv' action does not survive: lower deg or rank")
		vals = per_batch.mean(axis=0) + (exact if exact is not None else 0.0)
		qv = np.asarray(estimator.values, dtype=np.float64).ravel()
		est = float(estimator.estimate)
		info = dict(rank=int(pinfo["rank"]), logdet_precond=float(pinfo["logdet_p"]), trace=est, count=int(qv.size), deg=deg,
					std_error=float(np.std(qv, ddof=1) / np.sqrt(qv.size)), control_variate=bool(use_cv), ritz_max=float(top),
					grad_exact_values=exact, grad_per_batch=per_batch, batches=nb)  # fmt: skip
		if points:
			info["points_values"] = pvals
		return est + float(pinfo["logdet_p"]), vals, info
	finally:
		if hasattr(M, "close"):
			M.close()
		for obj in reversed(live):
			obj.close()


def _fold(base, vals) -> np.ndarray:
	"""(..., d + 2) raw values to (..., p + 2) shaped like the parameters: a scalar lengthscale's value is the sum over the dimensions."""
	d = base.X.shape[1]
	vals = np.asarray(vals, dtype=np.float64)
	if np.size(base.lengthscale) == 1:
		return np.concatenate([vals[..., :d].sum(axis=-1, keepdims=True), vals[..., d:]], axis=-1)
	return vals


def _as_params(base, f: np.ndarray) -> dict:
	p = f.size - 2
	return dict(lengthscale=np.array(f[:p], dtype=np.float64).reshape(np.shape(base.lengthscale)), outputscale=float(f[p]), noise=float(f[p + 1]))


def _shape_grad_info(base, info: dict, scale: float = 1.0) -> dict:
	"""The raw entries of `_logdet_grad`'s info as dicts shaped like the parameters: grad_exact, and grad_std_error from the per-batch
	means folded to the parameters' shape first (the error of a scalar lengthscale's summed gradient is that of the sums)."""
	ex, pb = info.pop("grad_exact_values"), info.pop("grad_per_batch")
	info["grad_exact"] = None if ex is None else _as_params(base, scale * _fold(base, ex))
	nb = pb.shape[0]
	info["grad_std_error"] = None if nb < 2 else _as_params(base, abs(scale) * _fold(base, pb).std(axis=0, ddof=1) / np.sqrt(nb))
	return info


def logdet_grad(K, rank: int = 100, deg: int = 20, count: int = 64, batch: int = 16, pdf: str = "device:rademacher", seed=None, probes=None,
				control_variate="auto", points: bool = False) -> tuple:  # fmt: skip
	"""(value, grads, info): log det A of the KernelOperator `K` (A = K0 + noise I, float64) as `logdet` estimates it, and the
	gradient of log det A with respect to the hyperparameters,

	    grads = dict(lengthscale=array shaped like K.lengthscale, outputscale=float, noise=float) ~ tr(A^-1 dA/dtheta),

	through the pivoted-Cholesky preconditioner. With M = P^{-1/2}, B = M A M and probes w,

	    tr(A^-1 D) = tr(P^-1 D) + E_w[(M (B^-1 - I) w)^T D (M w)]     control variate on
	               =              E_w[(M  B^-1      w)^T D (M w)]     off

	both unbiased for any factor. tr(P^-1 D) is exact and deterministic, from the factor's columns on the device
	(`DeviceOperator.precond_trace_grad`); the expectation is sampled with the probes of the value, B^-1 w being the "inv" action of
	the same Lanczos run whose quadrature is the value. This is the gradient of logdet A itself, NOT the derivative of the sampled
	value, and the factor P is not differentiated.

	K: a KernelOperator (a factor of rank `rank` is built), or a `K.preconditioned(rank)` kept by the caller, whose factor is refreshed
	only when K's hyperparameters have changed - the form for a training loop. rank = 0: `kernel_trace_grad` on A itself.
	count, batch: `count` probes in whole batches of equal size, cut as `logdet` cuts them. probes: a host n x count array instead of
	`pdf` (count must then be whole batches). control_variate: True, False, or "auto": on iff the largest Ritz value of B over the
	probes of the FIRST batch (from the plan's tridiagonals, on the host) is <= 2 - B >= I, and |1 / lam - 1| <= 1 / lam exactly when
	lam <= 2; with a poor factor the control variate makes the variance larger. The decision is taken before the first batch's update
	and holds for the whole call.
	info: logdet's (rank, logdet_precond, trace, std_error, count, deg), control_variate (the decision), ritz_max, grad_exact (the
	deterministic part shaped like grads; None with the control variate off), grad_std_error (per component, the sample standard
	deviation of the per-batch means over sqrt(batches); None with fewer than 2 batches), batches.
	points=True: grads["points"] (n x d) ~ tr(A^-1 dA/dx_ak), the gradient of log det A with respect to the points:
	a second accumulator updated at the same places with the same factors and weights, the exact part tr(P^-1 dA/dx) included when the
	control variate is on. With False every number keeps its bits."""
	from .grad import _kernel_grads

	rank, deg, count, batch = int(rank), int(deg), int(count), int(batch)
	if rank < 0 or deg < 1 or count < 2 or batch < 1:
		raise ValueError(f"rank = {rank} must be >= 0, deg = {deg} and batch = {batch} >= 1, count = {count} >= 2")
	base, B = _kernel_and_precond(K, rank, "logdet_grad")
	if probes is not None and np.asarray(probes).ndim == 2:
		count = int(np.asarray(probes).shape[1])
	if B is None:
		from .grad import kernel_trace_grad
		from .operators import MatrixFunction

		M = MatrixFunction(base, fun="log", deg=deg, dtype=np.float64)
		try:
			est, grads, ginfo = kernel_trace_grad(M, pdf=pdf, count=count, batch=batch, seed=seed, probes=probes, points=points)
		finally:
			if hasattr(M, "close"):
				M.close()
		q = np.asarray(ginfo["quad"], dtype=np.float64)
		info = dict(rank=0, logdet_precond=0.0, trace=float(est), count=int(q.size), deg=deg, std_error=float(np.std(q, ddof=1) / np.sqrt(q.size)),
					control_variate=False, ritz_max=None, grad_exact=None, grad_std_error=None, batches=-(-count // batch))  # fmt: skip
		return float(est), grads, info
	value, vals, info = _logdet_grad(base, B, deg, count, batch, pdf, seed, probes, control_variate, points=points)
	grads = _kernel_grads(base, vals)
	if points:
		grads["points"] = info.pop("points_values")
	return value, grads, _shape_grad_info(base, info)


def _params_vec(grads: dict) -> np.ndarray:
	return np.concatenate([np.ravel(np.asarray(grads["lengthscale"], dtype=np.float64)), [float(grads["outputscale"])], [float(grads["noise"])]])


def mll(K, y, rank: int = 100, deg: int = 20, solve_deg: Optional[int] = None, count: int = 64, batch: int = 16, pdf: str = "device:rademacher",
		seed=None, probes=None, control_variate="auto", profile: bool = False, points: bool = False) -> tuple:  # fmt: skip
	"""(value, grads, info): the marginal log-likelihood of a zero-mean Gaussian process with the kernel operator `K` (A = K0 + noise I,
	float64) for the observations `y` ((n,) or (n, q): q independent outputs sharing A), and its gradient with respect to the
	hyperparameters, shaped as `logdet_grad`'s:

	    value = -1/2 sum_q y_q^T alpha_q - (q / 2) logdet A - (n q / 2) log 2 pi,        alpha = A^-1 y,
	    grads =  1/2 sum_q alpha_q^T (dA/dtheta) alpha_q - (q / 2) tr(A^-1 dA/dtheta).

	alpha = M B^-1 M y comes from one kept-basis plan of `solve_deg` steps (None: deg) on the preconditioned operator, as in
	`posterior`; the data-fit gradient is ONE KernelGradAccumulator update on alpha, which never leaves the device; logdet A and
	tr(A^-1 dA/dtheta) are `logdet_grad`'s (rank, deg, count, batch, pdf, seed, probes, control_variate go there). The data-fit part
	is deterministic, the log-determinant part sampled: the gradient is that of the marginal likelihood itself - unbiased for any
	factor -, not the derivative of the sampled value. A zero column of `y` contributes only its log-determinant terms.
	K: a KernelOperator, or its `preconditioned(rank)` kept by the caller (refreshed only when the hyperparameters have changed).
	rank = 0: everything on A itself (for large noise).
	info: datafit and datafit_grad (-1/2 sum y^T alpha and its gradient), logdet and logdet_grad (the log-determinant and its
	gradient, unscaled), logdet_info (`logdet_grad`'s info), grad_std_error (of grads: q / 2 times logdet_grad's), steps (of the
	solve), q, zero_columns; with profile=True also timing_ms: wall time per phase, each closed by a synchronisation - refresh (the
	factor), solve, lanczos (the batches' runs, quadratures and actions), applies (M on the probes and the actions), updates (the
	accumulator, with its readback per batch), exact (tr(P^-1 dA/dtheta)), datafit (its update).
	points=True: grads["points"] (n x d), the gradient with respect to the training points X = the data-fit part -
	ONE point-gradient update on alpha with the weight 1/2 - minus (q / 2) times the log-determinant's (`logdet_grad(points=True)`); info
	gains datafit_points and logdet_points, timing_ms the phase "points". With False every number keeps its bits."""
	from .grad import _kernel_grads

	rank, deg, count, batch = int(rank), int(deg), int(count), int(batch)
	if rank < 0 or deg < 1 or count < 2 or batch < 1:
		raise ValueError(f"rank = {rank} must be >= 0, deg = {deg} and batch = {batch} >= 1, count = {count} >= 2")
	solve_deg = deg if solve_deg is None else int(solve_deg)
	if solve_deg < 1:
		raise ValueError(f"solve_deg = {solve_deg} must be >= 1")
	base, B = _kernel_and_precond(K, rank, "mll")
	n = int(base.shape[0])
	yh = np.asarray(y, dtype=np.float64)
	yh = yh.reshape(-1, 1) if yh.ndim == 1 else yh
	if yh.ndim != 2 or yh.shape[0] != n or yh.shape[1] < 1:
		raise ValueError(f"y must be ({n},) or ({n}, q), got shape {np.asarray(y).shape}")
	if not np.all(np.isfinite(yh)):
		raise ValueError("y must be finite")
	q = int(yh.shape[1])
	op = _as_device_operator(base, dtype=np.float64)
	ctx = op.ctx
	phases = _Phases(ctx, profile)
	with phases("refresh"):
		pop = _as_device_operator(B, dtype=np.float64) if B is not None else None
	solve_op = op if pop is None else pop
	nz = np.flatnonzero(np.any(yh != 0.0, axis=0))
	live = []
	fit, fit_vals, steps = 0.0, np.zeros(base.X.shape[1] + 2), None
	fit_points = np.zeros(base.X.shape) if points else None
	try:
		if nz.size:
			m = int(nz.size)
			with phases("solve"):
				plan = engine.LanczosPlan(solve_op, m, solve_deg, -1, basis="keep")
				live.append(plan)
				Yd, Alpha = engine.DeviceMatrix(n, m, ctx=ctx), engine.DeviceMatrix(n, m, ctx=ctx)
				live.extend((Yd, Alpha))
				Yd.set(0, np.asfortranarray(yh[:, nz]))
				tmp = None
				if pop is not None:
					tmp = (engine.DeviceMatrix(n, m, ctx=ctx), engine.DeviceMatrix(n, m, ctx=ctx))
					live.extend(tmp)
				_solve_into(pop, plan, Yd, Alpha, m, tmp, 0.0)
				steps = plan.steps_done
				fit = float(np.trace(Yd.tn(0, m, Alpha, 0, m)))
			if not np.isfinite(fit):
				raise FloatingPointError("mll: y^T A^-1 y is not finite")
			with phases("datafit"):
				acc = engine.KernelGradAccumulator(op)
				live.append(acc)
				acc.update(Alpha, 0, Alpha, 0, m, alpha=0.5, beta=0.0)
				fit_vals = acc.get()[0]
			if points:
				with phases("points"):
					pacc = engine.KernelPointGradAccumulator(op)
					live.append(pacc)
					pacc.update(Alpha, 0, Alpha, 0, m, alpha=0.5, beta=0.0)
					fit_points = pacc.get()[0]
	finally:
		for obj in reversed(live):
			obj.close()
	if B is None:
		ld, ld_grads, ld_info = logdet_grad(base, rank=0, deg=deg, count=count, batch=batch, pdf=pdf, seed=seed, probes=probes, points=points)
		ld_points = ld_grads.pop("points", None)
	else:
		if probes is not None and np.asarray(probes).ndim == 2:
			count = int(np.asarray(probes).shape[1])
		ld, ld_vals, ld_info = _logdet_grad(base, B, deg, count, batch, pdf, seed, probes, control_variate, phases, points=points)
		ld_points = ld_info.pop("points_values", None)
		ld_grads, ld_info = _kernel_grads(base, ld_vals), _shape_grad_info(base, ld_info)
	fit_grads = _kernel_grads(base, fit_vals)
	total = _params_vec(fit_grads) - 0.5 * q * _params_vec(ld_grads)
	value = -0.5 * fit - 0.5 * q * ld - 0.5 * n * q * float(np.log(2.0 * np.pi))
	se = ld_info.get("grad_std_error")
	info = dict(datafit=-0.5 * fit, datafit_grad=fit_grads, logdet=ld, logdet_grad=ld_grads, logdet_info=ld_info, steps=steps, q=q,
				zero_columns=[int(c) for c in np.setdiff1d(np.arange(q), nz)],
				grad_std_error=None if se is None else _as_params(base, 0.5 * q * _params_vec(se)))  # fmt: skip
	if profile:
		info["timing_ms"] = dict(phases.ms)
	grads = _as_params(base, total)
	if points:
		info["datafit_points"], info["logdet_points"] = fit_points, ld_points
		grads["points"] = fit_points - 0.5 * q * ld_points
	return value, grads, info


## ---- posterior function samples by pathwise conditioning ----------------------------------------------------------
SAMPLE_SOLVE_CHUNK = 128  # columns of one solve: a kept-basis plan of that many probes


def _param_key(K) -> tuple:
	return (tuple(np.ravel(np.asarray(K.lengthscale, dtype=np.float64)).tolist()), float(K.outputscale), float(K.noise))


class PosteriorPaths:
	"""`count` sample functions of a Gaussian process, each a function that can be evaluated and differentiated at any later points
	(`sample_paths` makes them):

	    f_c(x) = Phi(x) w_c + K(x, X) v_c,        v_c = A^-1 (y - Phi(X) w_c - sqrt(noise) eps_c)        (prior paths: the first term alone)

	It holds on the device the feature map (engine.KernelFeatureMap), the weights W (2 F2 x count) and V (n x count; None for prior
	paths), and keeps the device operator alive. Attributes: `features` (the KernelFeatures), `weights` (the host 2 F2 x count array),
	`info` (deg, steps: the Lanczos steps of each solve chunk, rank, count, num_features). The hyperparameters are those at creation:
	`evaluate` raises if K's have changed since - V belongs to that A. `close()` frees the device arrays; a context manager does."""

	def __init__(self, K, op, features, fmap, weights, Wd, V, E, info):
		self.K, self._op, self.features, self._fmap, self.weights, self._Wd, self._V, self._E, self.info = K, op, features, fmap, weights, Wd, V, E, info
		self.count = int(weights.shape[1])
		self._key = _param_key(K)

	def noise_draws(self) -> Optional[np.ndarray]:
		"""eps (n x count) as the solve used it, read back from the device; None where none was drawn (prior paths, noise = 0)."""
		return None if self._E is None else self._E.get()

	def evaluate(self, Xnew, grad: bool = False):
		"""F (m x count), F[a, c] = f_c(x*_a), computed on the device: only the m x count result leaves it. grad=True: (F, dF) with
		dF (m x d x count) = d f_c / d x*_a: the data term is the cross form of the point gradient with U a column of ones and W = v_c, one
		column at a time; the feature term is the same feature product on the weights W'[j] = Omega_jk w_{F2+j}, W'[F2+j] = -Omega_jk w_j,
		divided by the lengthscale of coordinate k."""
		if self._fmap is None:
			raise ValueError("the paths have been closed")
		if _param_key(self.K) != self._key:
			raise ValueError("the KernelOperator's hyperparameters have changed since these paths were drawn: V belongs to the A of then (draw new paths)")
		Cop = self.K.cross(Xnew)  # (checks the shape and the values of the new points)
		m, d = Cop.Xnew.shape
		count, ctx = self.count, self._op.ctx
		live = []

		def keep(obj):
			live.append(obj)
			return obj

		try:
			cross = keep(Cop.device(self._op))
			Fd = keep(engine.DeviceMatrix(m, count, ctx=ctx))
			self._fmap.matmat_dmat(self._Wd, 0, Fd, 0, count, rows=cross)
			if self._V is not None:
				Td = keep(engine.DeviceMatrix(m, count, ctx=ctx))
				cross.matmat_dmat(self._V, 0, Td, 0, count)
				for c0 in range(0, count, SAMPLE_SOLVE_CHUNK):  # (the axpy we have: a product with an identity)
					cb = min(SAMPLE_SOLVE_CHUNK, count - c0)
					Fd.add_product(c0, Td, c0, np.eye(cb), alpha=1.0, beta=1.0)
			F = Fd.get()
			if not np.all(np.isfinite(F)):
				raise FloatingPointError("evaluate: the paths' values are not finite")
			if not grad:
				return F
			dF = np.zeros((m, d, count))
			om = self.features.rounded().astype(np.float64)
			F2 = om.shape[0]
			ls = np.broadcast_to(np.asarray(self.K.lengthscale, dtype=np.float64), (d,))
			Wk = keep(engine.DeviceMatrix(2 * F2, count, ctx=ctx))
			for k in range(d):
				Wk.set(0, np.vstack([om[:, k][:, None] * self.weights[F2:], -om[:, k][:, None] * self.weights[:F2]]))
				self._fmap.matmat_dmat(Wk, 0, Fd, 0, count, rows=cross)
				dF[:, k, :] = Fd.get() / ls[k]
			if self._V is not None:
				pacc, Ones = keep(engine.KernelPointGradAccumulator(cross)), keep(engine.DeviceMatrix(m, 1, ctx=ctx))
				Ones.set(0, np.ones((m, 1)))
				for c in range(count):
					pacc.update(Ones, 0, self._V, c, 1, alpha=1.0, beta=0.0)
					dF[:, :, c] += pacc.get()[0]
			if not np.all(np.isfinite(dF)):
				raise FloatingPointError("evaluate: the paths' gradients are not finite")
			return F, dF
		finally:
			for obj in reversed(live):
				obj.close()

	def close(self):
		for name in ("_E", "_V", "_Wd", "_fmap"):
			obj = getattr(self, name, None)
			if obj is not None:
				obj.close()
			setattr(self, name, None)

	def __enter__(self):
		return self

	def __exit__(self, *exc):
		self.close()

	def __del__(self):
		try:
			self.close()
		except Exception:  # noqa: BLE001
			pass


def sample_paths(K, y=None, count: int = 16, num_features: int = 2048, deg: int = 60, orth: Optional[int] = None, precond_rank: int = 0, seed=None,
				 features=None, weights=None, noise_draws=None) -> PosteriorPaths:  # fmt: skip
	"""`count` function samples of the Gaussian process with the kernel operator `K` (a `KernelOperator` in float64; its noise is the
	observation noise) and zero prior mean, conditioned on the observations `y` ((n,)) at K's points - or of the prior, with y=None -
	by pathwise conditioning with a random-feature prior (Matheron's rule; Wilson et al. 2020). For each sample c

	    f_c(x) = Phi(x) w_c + K(x, X) v_c,        v_c = A^-1 (y - Phi(X) w_c - sqrt(noise) eps_c),        w_c ~ N(0, I),  eps_c ~ N(0, I)

	with Phi the `num_features` paired random Fourier features of K's profile (`KernelOperator.features`; `features=` takes a
	`KernelFeatures` instead of the draw). One feature product at the training points, the residual formed on the device, ONE solve
	over `count` columns - kept-basis Lanczos plans of `deg` steps (`orth` vectors of re-orthogonalisation, None: all) on A, or on
	`K.preconditioned(precond_rank)` as M B^-1 M for small noise - in chunks of at most 128 columns; V (n x count) stays on the device.
	A V that is not finite raises FloatingPointError, as `posterior` does. y=None: no solve, no V. noise = 0 draws no eps.

	Draws: `numpy.random.default_rng(seed)` gives the frequencies, then `weights` (2 F2 x count, standard normal), then the seed of eps;
	eps (n x count) is drawn on the device (`DeviceMatrix.generate(pdf="normal")`), so that nothing of size n crosses the bus.
	`weights=` and `noise_draws=` (a host n x count array) take explicit values, for tests.

	Given the frequencies, the paths have the mean C A^-1 y exactly, whatever the frequencies, and the covariance
	(Phi* - C A^-1 Phi_X)(...)^T + noise C A^-2 C^T, which tends to the posterior covariance as 1 / sqrt(F2).
	Returns a `PosteriorPaths`: `.evaluate(Xnew, grad=False)`."""
	from .operators import KernelFeatures, draw_kernel_frequencies

	if getattr(K, "_slq_kind", None) != "kernel":
		raise ValueError("sample_paths needs a KernelOperator")
	refuse_diag_scale(K, "gp.sample_paths")
	if np.dtype(K.dtype) != np.float64:
		raise ValueError(f"sample_paths is fp64 only (the device matrices are fp64): the KernelOperator is {np.dtype(K.dtype)}")
	n, d = K.X.shape
	count, deg, precond_rank = int(count), int(deg), int(precond_rank)
	if count < 1 or deg < 1 or precond_rank < 0:
		raise ValueError(f"count = {count} and deg = {deg} must be >= 1, precond_rank = {precond_rank} >= 0")
	yh = None
	if y is not None:
		yh = np.asarray(y, dtype=np.float64)
		if yh.shape != (n,):
			raise ValueError(f"y must be ({n},), got shape {yh.shape} (multi-output y is not built)")
		if not np.all(np.isfinite(yh)):
			raise ValueError("y must be finite")
	rng = np.random.default_rng(seed)
	if features is None:
		features = KernelFeatures(K, draw_kernel_frequencies(K.kernel, int(num_features), d, rng))
	elif not isinstance(features, KernelFeatures) or features.K is not K:
		raise ValueError("features must be a KernelFeatures of this KernelOperator (K.features(...))")
	F2 = features.num_features
	if weights is None:
		Wh = rng.standard_normal((2 * F2, count))
	else:
		Wh = np.array(weights, dtype=np.float64)
		if Wh.shape != (2 * F2, count) or not np.all(np.isfinite(Wh)):
			raise ValueError(f"weights must be a finite (2 F2, count) = ({2 * F2}, {count}) array, got shape {Wh.shape}")
	eps_seed = int(rng.integers(0, 2**63 - 1))
	sigma2 = float(K.noise)
	Eh = None
	if noise_draws is not None:
		Eh = np.asarray(noise_draws, dtype=np.float64)
		if Eh.shape != (n, count) or not np.all(np.isfinite(Eh)):
			raise ValueError(f"noise_draws must be a finite (n, count) = ({n}, {count}) array, got shape {Eh.shape}")

	op = _as_device_operator(K, dtype=np.float64)
	ctx = op.ctx
	orth_arg = -1 if orth is None else int(orth)
	info = dict(deg=min(deg, n), steps=[], rank=0, count=count, num_features=F2)
	kept, live = [], []
	try:
		fmap = features.device(op)
		kept.append(fmap)
		Wd = engine.DeviceMatrix(2 * F2, count, ctx=ctx)
		kept.append(Wd)
		Wd.set(0, Wh)
		V = E = None
		if yh is not None:
			pop = _as_device_operator(K.preconditioned(precond_rank), dtype=np.float64) if precond_rank > 0 else None
			if pop is not None:
				info["rank"] = int(pop.info()["rank"])
			solve_op = op if pop is None else pop
			## the residual y - Phi W - sqrt(noise) E, on the device
			R = engine.DeviceMatrix(n, count, ctx=ctx)
			live.append(R)
			fmap.matmat_dmat(Wd, 0, R, 0, count)
			Yd = engine.DeviceMatrix(n, 1, ctx=ctx)
			live.append(Yd)
			Yd.set(0, yh.reshape(-1, 1))
			R.add_product(0, Yd, 0, np.ones((1, count)), alpha=1.0, beta=-1.0)
			if sigma2 > 0.0:
				E = engine.DeviceMatrix(n, count, ctx=ctx)
				kept.append(E)
				if Eh is not None:
					E.set(0, Eh)
				else:
					E.generate(0, count, pdf="normal", seed=eps_seed)
				for c0 in range(0, count, SAMPLE_SOLVE_CHUNK):  # (the axpy we have: a product with an identity)
					cb = min(SAMPLE_SOLVE_CHUNK, count - c0)
					R.add_product(c0, E, c0, np.eye(cb), alpha=-float(np.sqrt(sigma2)), beta=1.0)
			V = engine.DeviceMatrix(n, count, ctx=ctx)
			kept.append(V)
			plans = {}
			for c0 in range(0, count, SAMPLE_SOLVE_CHUNK):
				cb = min(SAMPLE_SOLVE_CHUNK, count - c0)
				if cb not in plans:  # a plan of cb probes with its right-hand sides, its solution and the preconditioned path's scratch
					plan = engine.LanczosPlan(solve_op, cb, deg, orth_arg, basis="keep")
					live.append(plan)
					mats = [engine.DeviceMatrix(n, cb, ctx=ctx) for _ in range(2 if pop is None else 4)]
					live.extend(mats)
					plans[cb] = (plan, mats[0], mats[1], tuple(mats[2:]) or None)
				plan, rhs, sol, tmp = plans[cb]
				rhs.copy_from(0, R, c0, cb)
				_solve_into(pop, plan, rhs, sol, cb, tmp, 0.0)
				info["steps"].append(plan.steps_done)
				V.copy_from(c0, sol, 0, cb)
				g = np.diag(sol.tn(0, cb, sol, 0, cb))  # (cb x cb on the host: nothing of size n leaves the device)
				if not np.all(np.isfinite(g)):
					raise FloatingPointError(f"sample_paths: V is not finite in the columns [{c0}, {c0 + cb}) (a Lanczos run stopped before `deg` steps, which the 'inv' action does not survive: lower deg)")
		paths = PosteriorPaths(K, op, features, fmap, Wh, Wd, V, E, info)
		kept = []
		return paths
	finally:
		for obj in reversed(live + kept):
			obj.close()


## ---- weight-space regression with the feature model K ~ Phi Phi^T -------------------------------------------------
FEATURE_POSTERIOR_MAX_WEIGHTS = 8192  # 2 F2: the weight-space system is factorised on the host by NumPy
FEATURE_PREDICT_CHUNK = 128  # columns of L^-T per feature product of the predictive variance


class FeaturePosterior:
	"""The Gaussian process with the kernel Phi Phi^T in the place of K's (`feature_posterior` makes it): w ~ N(0, I),
	y = Phi w + noise. Attributes: `mll` (the log marginal likelihood of that model), `mean_weights` (w_bar = M^-1 Phi^T y, M = Phi^T Phi
	+ sigma2 I = L L^T), `features` (the KernelFeatures), `info` (num_features, gram_asymmetry, m_diag_min, m_diag_max). The
	hyperparameters are those at creation: `predict` and `sample_paths` raise if K's have changed since. `close()` frees the device
	feature map; a context manager does."""

	def __init__(self, K, op, features, fmap, L, mean_weights, mll, info):
		self.K, self._op, self.features, self._fmap, self._L = K, op, features, fmap, L
		self.mean_weights, self.mll, self.info = mean_weights, float(mll), info
		self._sigma2 = float(K.noise)
		self._key = _param_key(K)

	def _check(self, who: str):
		if self._fmap is None:
			raise ValueError("the feature posterior has been closed")
		if _param_key(self.K) != self._key:
			raise ValueError(f"{who}: the KernelOperator's hyperparameters have changed since this feature posterior was made: its weights belong to the Phi of then (make a new one)")

	def predict(self, Xnew, variance: bool = True, include_noise: bool = False) -> tuple:
		"""(mean, var) at the new points (m x d): mean = Phi(X*) w_bar, one feature product; var = sigma2 |L^-1 phi*|^2, feature products
		on column chunks of L^-T with the row sums of squares of the m x chunk blocks accumulated on the host (None with variance=False);
		include_noise adds sigma2."""
		from scipy.linalg import solve_triangular

		self._check("predict")
		Cop = self.K.cross(Xnew)  # (checks the shape and the values of the new points)
		m = Cop.Xnew.shape[0]
		m2, ctx = self.mean_weights.shape[0], self._op.ctx
		live = []
		try:
			cross = Cop.device(self._op)
			live.append(cross)
			chunk = min(FEATURE_PREDICT_CHUNK, m2)
			Wd = engine.DeviceMatrix(m2, chunk, ctx=ctx)
			live.append(Wd)
			Fd = engine.DeviceMatrix(m, chunk, ctx=ctx)
			live.append(Fd)
			Wd.set(0, np.hstack([self.mean_weights[:, None], np.zeros((m2, chunk - 1))]))
			self._fmap.matmat_dmat(Wd, 0, Fd, 0, 1, rows=cross)
			mean = Fd.get(0, 1)[:, 0].copy()
			var = None
			if variance:
				acc = np.zeros(m)
				for c0 in range(0, m2, chunk):
					cb = min(chunk, m2 - c0)
					E = np.zeros((m2, cb))
					E[c0 + np.arange(cb), np.arange(cb)] = 1.0
					B = solve_triangular(self._L, E, lower=True, trans="T", check_finite=False)  # columns [c0, c0 + cb) of L^-T
					Wd.set(0, np.hstack([B, np.zeros((m2, chunk - cb))]))
					self._fmap.matmat_dmat(Wd, 0, Fd, 0, cb, rows=cross)
					acc += np.sum(Fd.get(0, cb) ** 2, axis=1)
				var = self._sigma2 * acc + (self._sigma2 if include_noise else 0.0)
			if not np.all(np.isfinite(mean)) or (var is not None and not np.all(np.isfinite(var))):
				raise FloatingPointError("predict: the feature model's prediction is not finite")
			return mean, var
		finally:
			for obj in reversed(live):
				obj.close()

	def sample_paths(self, count: int = 16, seed=None, normals=None) -> PosteriorPaths:
		"""`count` sample functions of the weight-space posterior as a `PosteriorPaths` without a data term (V = None): the weights are
		W = w_bar 1^T + sqrt(sigma2) L^-T Xi with Xi = default_rng(seed).standard_normal((2 F2, count)), or `normals` given explicitly."""
		from scipy.linalg import solve_triangular

		self._check("sample_paths")
		count = int(count)
		m2 = self.mean_weights.shape[0]
		if count < 1:
			raise ValueError(f"count = {count} must be >= 1")
		if normals is None:
			Xi = np.random.default_rng(seed).standard_normal((m2, count))
		else:
			Xi = np.array(normals, dtype=np.float64)
			if Xi.shape != (m2, count) or not np.all(np.isfinite(Xi)):
				raise ValueError(f"normals must be a finite (2 F2, count) = ({m2}, {count}) array, got shape {Xi.shape}")
		Wh = self.mean_weights[:, None] + np.sqrt(self._sigma2) * solve_triangular(self._L, Xi, lower=True, trans="T", check_finite=False)
		kept = []
		try:
			fmap = self.features.device(self._op)  # (the paths own and close their map)
			kept.append(fmap)
			Wd = engine.DeviceMatrix(m2, count, ctx=self._op.ctx)
			kept.append(Wd)
			Wd.set(0, Wh)
			paths = PosteriorPaths(self.K, self._op, self.features, fmap, Wh, Wd, None, None, dict(count=count, num_features=self.features.num_features))
			kept = []
			return paths
		finally:
			for obj in reversed(kept):
				obj.close()

	def close(self):
		if getattr(self, "_fmap", None) is not None:
			self._fmap.close()
		self._fmap = None

	def __enter__(self):
		return self

	def __exit__(self, *exc):
		self.close()

	def __del__(self):
		try:
			self.close()
		except Exception:  # noqa: BLE001
			pass


def feature_posterior(K, y, num_features: int = 1024, seed=None, features=None) -> FeaturePosterior:
	"""Sparse-spectrum GP regression: the Gaussian process with the kernel Phi Phi^T in the place of K's, Phi the `num_features` paired
	random Fourier features of K's profile (the frequency draw and `features=` as in `sample_paths`), zero mean, w ~ N(0, I) and
	noise sigma2 = K.noise > 0. K: a `KernelOperator` in float64; y: (n,), finite; 2 F2 <= 8192.

	    h = Phi^T y (one adjoint product)        G = Phi^T Phi (KernelFeatureMap.gram)        M = G + sigma2 I = L L^T (host)
	    w_bar = M^-1 h        mll = -1/2 [ (y^T y - h^T w_bar) / sigma2 + 2 sum log L_jj + (n - 2 F2) log sigma2 + n log 2 pi ]

	Only y, h and the blocks of G cross the bus; nothing of size n x F2 is held. A failed Cholesky raises FloatingPointError.
	Returns a `FeaturePosterior`: `.mll`, `.mean_weights`, `.predict(Xnew)`, `.sample_paths(count)`."""
	from .operators import KernelFeatures, draw_kernel_frequencies

	if getattr(K, "_slq_kind", None) != "kernel":
		raise ValueError("feature_posterior needs a KernelOperator")
	refuse_diag_scale(K, "gp.feature_posterior")
	if np.dtype(K.dtype) != np.float64:
		raise ValueError(f"feature_posterior is fp64 only (the device matrices are fp64): the KernelOperator is {np.dtype(K.dtype)}")
	n, d = K.X.shape
	yh = np.asarray(y, dtype=np.float64)
	if yh.shape != (n,):
		raise ValueError(f"y must be ({n},), got shape {yh.shape} (multi-output y is not built)")
	if not np.all(np.isfinite(yh)):
		raise ValueError("y must be finite")
	sigma2 = float(K.noise)
	if not sigma2 > 0.0:
		raise ValueError(f"feature_posterior needs noise > 0, got {sigma2}: Phi^T Phi alone is singular when 2 F2 > n")
	rng = np.random.default_rng(seed)
	if features is None:
		if 2 * int(num_features) > FEATURE_POSTERIOR_MAX_WEIGHTS:
			raise ValueError(f"feature_posterior: 2 F2 = {2 * int(num_features)} weights exceed the limit of {FEATURE_POSTERIOR_MAX_WEIGHTS} (the weight-space system is solved on the host)")
		features = KernelFeatures(K, draw_kernel_frequencies(K.kernel, int(num_features), d, rng))
	elif not isinstance(features, KernelFeatures) or features.K is not K:
		raise ValueError("features must be a KernelFeatures of this KernelOperator (K.features(...))")
	F2 = features.num_features
	if 2 * F2 > FEATURE_POSTERIOR_MAX_WEIGHTS:
		raise ValueError(f"feature_posterior: 2 F2 = {2 * F2} weights exceed the limit of {FEATURE_POSTERIOR_MAX_WEIGHTS} (the weight-space system is solved on the host)")

	op = _as_device_operator(K, dtype=np.float64)
	fmap = features.device(op)
	try:
		from scipy.linalg import solve_triangular

		h = fmap.rmatmat(yh.reshape(-1, 1))[:, 0]
		G = fmap.gram()
		M = G + sigma2 * np.eye(2 * F2)
		if not np.all(np.isfinite(M)):
			raise FloatingPointError("feature_posterior: Phi^T Phi is not finite")
		try:
			L = np.linalg.cholesky(M)
		except np.linalg.LinAlgError as e:
			raise FloatingPointError(f"feature_posterior: the Cholesky factorisation of Phi^T Phi + sigma2 I failed ({e})") from None
		wbar = solve_triangular(L, solve_triangular(L, h, lower=True, check_finite=False), lower=True, trans="T", check_finite=False)
		dg = np.diag(M)
		mll = -0.5 * ((float(yh @ yh) - float(h @ wbar)) / sigma2 + 2.0 * float(np.sum(np.log(np.diag(L)))) + (n - 2 * F2) * np.log(sigma2) + n * np.log(2.0 * np.pi))
		info = dict(num_features=F2, gram_asymmetry=fmap.gram_asymmetry, m_diag_min=float(dg.min()), m_diag_max=float(dg.max()))
		post = FeaturePosterior(K, op, features, fmap, L, wbar, mll, info)
		fmap = None
		return post
	finally:
		if fmap is not None:
			fmap.close()


## ---- the diagonally scaled operator: fixed per-point noise and the Laplace approximation -------------------------
def _scale_rows(M, c0: int, nc: int, c_dev) -> None:
	"""M[:, c0 : c0 + nc] *= c[:, None] on the device (torch on the matrix's own memory; `c_dev`: a torch tensor of n entries on the
	context's GPU). The library writes on its own stream and torch on its: both are waited for."""
	import torch

	dev = f"cuda:{M.ctx.device}"
	t = torch.as_tensor(M.cuda_array(c0, nc), device=dev).view(nc, M.n)
	M.ctx.synchronize()
	t.mul_(c_dev)
	torch.cuda.synchronize(dev)


def _scale_to_device(c: np.ndarray, ctx):
	import torch

	return torch.as_tensor(np.ascontiguousarray(c, dtype=np.float64), device=f"cuda:{ctx.device}")


def _scaled_operator(K, c: np.ndarray, noise: float):
	"""A KernelOperator of its own on K's points, profile, lengthscales and outputscale with the diagonal scale `c` and `noise`: K is not
	mutated, and the new operator's z are K's bit for bit (the same points, centre and lengthscales)."""
	from .operators import KernelOperator

	return KernelOperator(K.X, K.kernel, lengthscale=K.lengthscale, outputscale=K.outputscale, noise=noise, dtype=np.float64, diag_scale=c)


def _check_gp_operator(K, who: str) -> None:
	if getattr(K, "_slq_kind", None) != "kernel":
		raise ValueError(f"{who} needs a KernelOperator")
	if np.dtype(K.dtype) != np.float64:
		raise ValueError(f"{who} is fp64 only (the device matrices are fp64): the KernelOperator is {np.dtype(K.dtype)}")
	if getattr(K, "diag_scale", None) is not None:
		raise ValueError(f"{who} builds the scaled operator itself: pass the KernelOperator of the prior, without a diagonal scale")


def _scaled_variance(op, c_dev, Cop, s: float, deg: int, orth_arg: int, batch: int, info: dict, who: str) -> np.ndarray:
	"""s - diag((D C^T)^T A'^-1 (D C^T)) for the new points of the KernelCrossOperator `Cop`, A' the scaled device operator `op` and D =
	diag(c), per batch of at most `batch` new points as `posterior` does it: C_b^T by the adjoint cross product (which ignores the
	scale), its rows scaled on the device, one kept-basis solve, the m_b x m_b block on the host. A zero column (a new point whose
	phi has underflowed against every training point, or whose neighbours all have c = 0) has var = s exactly and never reaches the plan."""
	n, m = op.shape[0], Cop.Xnew.shape[0]
	ctx = op.ctx
	live = []
	try:
		mb_max = min(batch, m)
		B, Cv = engine.DeviceMatrix(n, mb_max, ctx=ctx), engine.DeviceMatrix(n, mb_max, ctx=ctx)
		live += [B, Cv]
		plans = {}
		quad = np.zeros(m)
		for i0 in range(0, m, batch):
			i1 = min(m, i0 + batch)
			mb = i1 - i0
			crossb = engine.KernelCross(op, Cop.Xnew[i0:i1])
			live.append(crossb)
			Eye = engine.DeviceMatrix(mb, mb, ctx=ctx)
			live.append(Eye)
			Eye.set(0, np.eye(mb))
			crossb.matmat_dmat(Eye, 0, B, 0, mb, trans=True)
			_scale_rows(B, 0, mb, c_dev)  # B = D C_b^T
			zero = np.flatnonzero(np.diag(B.tn(0, mb, B, 0, mb)) == 0.0)
			good = np.setdiff1d(np.arange(mb), zero)
			block = np.zeros((mb, mb))
			if good.size:
				for j in zero:
					B.copy_from(int(j), B, int(good[0]), 1)
				if mb not in plans:
					plans[mb] = engine.LanczosPlan(op, mb, deg, orth_arg, basis="keep")
					live.append(plans[mb])
				plans[mb].set_probes_device(B.col_ptr(0))
				plans[mb].run(0.0)
				plans[mb].fun_action_into(Cv, 0, "inv")
				info["steps"].append(plans[mb].steps_done)
				block = B.tn(0, mb, Cv, 0, mb)
				if not np.all(np.isfinite(block)):
					raise FloatingPointError(f"{who}: the variance block of the new points [{i0}, {i1}) is not finite")
				block[zero, :] = 0.0
				block[:, zero] = 0.0
			info["batches"] += 1
			info["zero_columns"].extend(int(i0 + j) for j in zero)
			quad[i0:i1] = np.diag(block)
			Eye.close()
			crossb.close()
		return s - quad
	finally:
		for obj in reversed(live):
			obj.close()


def fixed_noise_posterior(K, y, noise_var, Xnew, deg: int = 100, orth: Optional[int] = None, variance: bool = True, batch: int = 128) -> tuple:
	"""(mean, var, info): the posterior of a zero-mean Gaussian process with the kernel of `K` (a `KernelOperator` in float64, without a
	diagonal scale; it is not mutated) under KNOWN PER-POINT observation noise e_i = K.noise + noise_var_i (all > 0), given `y` ((n,) or
	(n, q)) at K's points, at the new points `Xnew` (m x d). DESIGN.md §4.23: with c = e^{-1/2}, D = diag(c) and A' = D K0 D + I - the
	scaled operator, built here on K's points with noise 1 -

	    K0 + diag(e) = E^{1/2} A' E^{1/2},      alpha = (K0 + E)^-1 y = D A'^-1 D y,      mean = C alpha,
	    var = s - diag((D C^T)^T A'^-1 (D C^T)),

	the variance per batch of at most `batch` new points as `posterior` takes it (zero columns likewise: var = s exactly). A' has its
	eigenvalues in [1, 1 + s max(c)^2 n]: no preconditioner is needed at moderate noise, and none is built for a scaled operator. The
	solves are kept-basis Lanczos plans of `deg` steps (100 by default: plain Lanczos reaches 1e-13 at 100 steps where it has 1e-10 at
	posterior's 60 on a matern32 of condition 2e3) with `orth` vectors of re-orthogonalisation (None: all). The row scalings of device
	matrices happen on the device; of size n only c goes to the device and nothing comes back. The log-determinant is NOT computed here
	(logdet(K0 + E) = logdet A' + sum log e_i; `laplace(...).log_marginal` shows the estimator on a scaled operator).
	info: deg, batches, steps, zero_columns as `posterior`'s."""
	_check_gp_operator(K, "fixed_noise_posterior")
	n = K.X.shape[0]
	deg, batch = int(deg), int(batch)
	if deg < 1 or batch < 1:
		raise ValueError(f"deg = {deg} and batch = {batch} must be >= 1")
	yh = np.asarray(y, dtype=np.float64)
	vector = yh.ndim == 1
	yh = yh.reshape(-1, 1) if vector else yh
	if yh.ndim != 2 or yh.shape[0] != n or yh.shape[1] < 1:
		raise ValueError(f"y must be ({n},) or ({n}, q), got shape {np.asarray(y).shape}")
	if not np.all(np.isfinite(yh)):
		raise ValueError("y must be finite")
	nv = np.asarray(noise_var, dtype=np.float64)
	nv = np.full(n, float(nv)) if nv.ndim == 0 else nv.ravel()
	if nv.size != n:
		raise ValueError(f"noise_var must be a scalar or ({n},), got shape {np.asarray(noise_var).shape}")
	e = float(K.noise) + nv
	bad = np.flatnonzero(~(np.isfinite(e) & (e > 0)))
	if bad.size:
		raise ValueError(f"fixed_noise_posterior: the noise of point {int(bad[0])} is K.noise + noise_var = {e[bad[0]]}: every e_i must be a finite number > 0")
	c = 1.0 / np.sqrt(e)
	Cop = K.cross(Xnew)  # (checks the shape and the values of the new points; the cross products ignore the scale)
	m, q = Cop.Xnew.shape[0], yh.shape[1]
	orth_arg = -1 if orth is None else int(orth)
	s = float(K.outputscale)
	Ks = _scaled_operator(K, c, 1.0)
	ctx = engine.default_context()
	live = []
	info = dict(deg=min(deg, n), batches=0, steps=[], zero_columns=[])
	try:
		op = engine.DeviceOperator(Ks, ctx=ctx)
		live.append(op)
		c_dev = _scale_to_device(c, ctx)
		nz = np.flatnonzero(np.any(yh != 0.0, axis=0))
		mean = np.zeros((m, q))
		if nz.size:
			plan = engine.LanczosPlan(op, int(nz.size), deg, orth_arg, basis="keep")
			live.append(plan)
			Alpha = engine.DeviceMatrix(n, int(nz.size), ctx=ctx)
			live.append(Alpha)
			plan.set_probes(np.asfortranarray(c[:, None] * yh[:, nz]))  # D y: y comes from the host anyway
			plan.run(0.0)
			plan.fun_action_into(Alpha, 0, "inv")
			info["steps"].append(plan.steps_done)
			_scale_rows(Alpha, 0, int(nz.size), c_dev)  # alpha = D A'^-1 D y
			cross = Cop.device(op)
			live.append(cross)
			Mean = engine.DeviceMatrix(m, int(nz.size), ctx=ctx)
			live.append(Mean)
			cross.matmat_dmat(Alpha, 0, Mean, 0, int(nz.size))
			mean[:, nz] = Mean.get()
			if not np.all(np.isfinite(mean)):
				raise FloatingPointError("fixed_noise_posterior: the mean is not finite")
			for obj in (Mean, cross, Alpha, plan):
				obj.close()
		mean = mean[:, 0] if vector else mean
		var = _scaled_variance(op, c_dev, Cop, s, deg, orth_arg, batch, info, "fixed_noise_posterior") if variance else None
		return mean, var, info
	finally:
		for obj in reversed(live):
			obj.close()


LAPLACE_LIKELIHOODS = ("logit", "poisson")
LAPLACE_MAX_HALVINGS = 30


def _laplace_targets(y, likelihood: str, n: int) -> np.ndarray:
	"""The observations as the likelihood's formulas take them: logit - t in {0, 1} from labels in {-1, +1} or {0, 1}; poisson - counts."""
	yh = np.asarray(y, dtype=np.float64).ravel()
	if yh.size != n:
		raise ValueError(f"y must be ({n},), got shape {np.asarray(y).shape}")
	if likelihood == "logit":
		if np.all(np.isin(yh, (-1.0, 1.0))):
			return 0.5 * (yh + 1.0)
		if np.all(np.isin(yh, (0.0, 1.0))):
			return yh.copy()
		raise ValueError("laplace(likelihood='logit'): the labels must all be in {-1, +1} or all in {0, 1}")
	if not (np.all(np.isfinite(yh)) and np.all(yh >= 0) and np.all(yh == np.round(yh))):
		raise ValueError("laplace(likelihood='poisson'): y must be non-negative integers")
	return yh.copy()


def laplace_likelihood(likelihood: str, t: np.ndarray, f: np.ndarray) -> tuple:
	"""(log p(y|f), its gradient, W = minus its diagonal Hessian) of the two log-concave likelihoods, in closed form:
	logit    log p = sum t f - log(1 + e^f),   grad = t - sigmoid(f),   W = sigmoid(f) (1 - sigmoid(f))        (t in {0, 1})
	poisson  log p = sum y f - e^f - log y!,   grad = y - e^f,          W = e^f                                   (log link)
	W >= 0 always; it may underflow to 0 for a saturated logistic, which the scaled operator admits (c_i = 0)."""
	from scipy.special import expit, gammaln

	if likelihood == "logit":
		pi = expit(f)
		return float(np.sum(t * f - np.logaddexp(0.0, f))), t - pi, expit(f) * expit(-f)
	ef = np.exp(f)
	return float(np.sum(t * f - ef - gammaln(t + 1.0))), t - ef, ef


class LaplacePosterior:
	"""The Laplace approximation of a Gaussian-process posterior under a non-Gaussian likelihood (`laplace` makes it).
	Attributes: `f_hat` (the mode), `a` (= K0^-1 f_hat, never formed by a solve with K0), `W` (minus the Hessian of log p(y|f) at the
	mode, diagonal), `iterations`, `converged`, `objective` (Psi(f_hat) = log p(y|f_hat) - a^T f_hat / 2), `info`. It holds ONE scaled
	device operator, B = I + W^{1/2} K0 W^{1/2} at the mode, until `close()` (context manager, `__del__`)."""

	def __init__(self, K, likelihood, t, op, f_hat, a, W, grad, iterations, converged, objective, deg, orth_arg, info):
		self.K, self.likelihood, self._t, self._op = K, likelihood, t, op
		self.f_hat, self.a, self.W, self._grad = f_hat, a, W, grad
		self.iterations, self.converged, self.objective = int(iterations), bool(converged), float(objective)
		self._deg, self._orth = deg, orth_arg
		self._key = _param_key(K)
		self.info = info
		self.quadratures = None  # the per-probe v^T log(B) v of the last log_marginal

	def _check(self, who: str):
		if self._op is None:
			raise ValueError(f"{who}: the LaplacePosterior has been closed")
		if _param_key(self.K) != self._key:
			raise ValueError(f"{who}: the KernelOperator's hyperparameters have changed since laplace(): fit again")

	def predict(self, Xnew, variance: bool = True, batch: int = 128) -> tuple:
		"""(mean, var) of the latent function at `Xnew` (m x d) - mean = C grad log p(y|f_hat), var = s - diag((D C^T)^T B^-1 (D C^T)) with
		D = W^{1/2} (Rasmussen & Williams, eqs. 3.21 and 3.24), the variance by the batched solve of `fixed_noise_posterior` - and for
		"logit" a third value: the class probability sigmoid(mean / sqrt(1 + pi var / 8)), the probit approximation of the averaged
		logistic (None with variance=False)."""
		from scipy.special import expit

		self._check("LaplacePosterior.predict")
		K, op = self.K, self._op
		Cop = K.cross(Xnew)
		m, n = Cop.Xnew.shape[0], K.X.shape[0]
		live = []
		info = dict(batches=0, steps=[], zero_columns=[])
		try:
			G = engine.DeviceMatrix(n, 1, ctx=op.ctx)
			live.append(G)
			G.set(0, self._grad.reshape(-1, 1))
			cross = Cop.device(op)
			live.append(cross)
			Mean = engine.DeviceMatrix(m, 1, ctx=op.ctx)
			live.append(Mean)
			cross.matmat_dmat(G, 0, Mean, 0, 1)
			mean = Mean.get()[:, 0]
			var = None
			if variance:
				c_dev = _scale_to_device(np.sqrt(self.W), op.ctx)
				var = _scaled_variance(op, c_dev, Cop, float(K.outputscale), self._deg, self._orth, int(batch), info, "LaplacePosterior.predict")
			self.info["predict"] = info
			if self.likelihood != "logit":
				return mean, var
			prob = None if var is None else expit(mean / np.sqrt(1.0 + np.pi * np.maximum(var, 0.0) / 8.0))
			return mean, var, prob
		finally:
			for obj in reversed(live):
				obj.close()

	def log_marginal(self, count: int = 64, deg: int = 30, seed=None, probes=None) -> tuple:
		"""(value, stderr): the Laplace estimate of log p(y) = Psi(f_hat) - logdet(B) / 2 (Rasmussen & Williams, eq. 3.32), the
		log-determinant by stochastic Lanczos quadrature on the scaled operator: `count` Rademacher probes drawn by
		numpy.random.default_rng(seed) - or the explicit `probes` (n x count, entries +-1 for an unbiased estimate) - `deg` steps, full
		re-orthogonalisation. stderr is that of the value: half the sample standard deviation of the per-probe v^T log(B) v over
		sqrt(count). `self.quadratures` keeps the per-probe values."""
		self._check("LaplacePosterior.log_marginal")
		n = self.K.X.shape[0]
		if probes is None:
			count = int(count)
			if count < 2:
				raise ValueError(f"count = {count} must be >= 2")
			V = np.where(np.random.default_rng(seed).random((n, count)) < 0.5, -1.0, 1.0)
		else:
			V = np.asarray(probes, dtype=np.float64)
			if V.ndim != 2 or V.shape[0] != n or V.shape[1] < 2 or not np.all(np.isfinite(V)):
				raise ValueError(f"probes must be a finite ({n}, count >= 2) array, got shape {V.shape}")
		count, deg = V.shape[1], int(deg)
		if deg < 1:
			raise ValueError(f"deg = {deg} must be >= 1")
		vals = np.empty(count)
		plans = {}
		try:
			for c0 in range(0, count, 128):
				cb = min(128, count - c0)
				if cb not in plans:
					plans[cb] = engine.LanczosPlan(self._op, cb, deg, -1)
				plans[cb].set_probes(np.asfortranarray(V[:, c0 : c0 + cb]))
				plans[cb].run(0.0)
				vals[c0 : c0 + cb] = plans[cb].quadrature("log")
		finally:
			for p in plans.values():
				p.close()
		self.quadratures = vals
		return self.objective - 0.5 * float(np.mean(vals)), 0.5 * float(np.std(vals, ddof=1) / np.sqrt(count))

	def close(self):
		if getattr(self, "_op", None) is not None:
			self._op.close()
			self._op = None

	def __enter__(self):
		return self

	def __exit__(self, *exc):
		self.close()

	def __del__(self):
		try:
			self.close()
		except Exception:  # noqa: BLE001
			pass


def laplace(K, y, likelihood: str, deg: int = 40, orth: Optional[int] = None, max_iter: int = 30, tol: float = 1e-10) -> LaplacePosterior:
	"""The Laplace approximation of the posterior of a zero-mean Gaussian process with the kernel of `K` under a non-Gaussian likelihood:
	"logit" (binary labels in {-1, +1} or {0, 1}) or "poisson" (log link, non-negative integer counts) - both log-concave with a
	closed-form gradient and W = -d2 log p / df2 >= 0. K: a `KernelOperator` in float64 without a diagonal scale and with noise = 0: the
	prior of the LATENT function is K0 itself - the likelihood is the observation model, and a Gaussian noise term on top of it would be
	a different model (a jitter belongs in the kernel, not here). K is not mutated.

	Newton's iteration of Rasmussen & Williams, Algorithm 3.1, on ONE scaled device operator B = I + W^{1/2} K0 W^{1/2} (DESIGN.md §4.23:
	c = W^{1/2}, noise 1) whose scale is reset each iteration, and a second, unscaled noise-free operator on the same points for K0 b:

	    b = W f + grad log p(y|f),      a = b - W^{1/2} B^-1 W^{1/2} K0 b,      f = K0 a,

	the solve a kept-basis plan's `fun_action_into(..., "inv")` of `deg` steps (B has its eigenvalues in [1, 1 + max(W) lambda_max(K0)]).
	The step from (a, f) to the Newton point is halved while the objective Psi = log p(y|f) - a^T f / 2 decreases (f is linear in a: no
	further product). It stops when max |delta f| <= tol max(1, max |f|), or after `max_iter` iterations (`converged` says which).
	The n-vectors f, W, b live on the host - the likelihood is NumPy - and cross the bus once per product; the n^2 work is the device's."""
	_check_gp_operator(K, "laplace")
	if likelihood not in LAPLACE_LIKELIHOODS:
		raise ValueError(f"laplace: unknown likelihood {likelihood!r} (one of {', '.join(LAPLACE_LIKELIHOODS)})")
	if float(K.noise) != 0.0:
		raise ValueError(f"laplace needs K.noise = 0 (the prior of the latent function is K0; the likelihood is the observation model), got {K.noise}")
	n = K.X.shape[0]
	deg, max_iter, tol = int(deg), int(max_iter), float(tol)
	if deg < 1 or max_iter < 1 or not (np.isfinite(tol) and tol > 0):
		raise ValueError(f"deg = {deg} and max_iter = {max_iter} must be >= 1, tol = {tol} a finite number > 0")
	t = _laplace_targets(y, likelihood, n)
	orth_arg = -1 if orth is None else int(orth)
	ctx = engine.default_context()
	f, a = np.zeros(n), np.zeros(n)
	lp, grad, W = laplace_likelihood(likelihood, t, f)
	psi = lp
	Ks = _scaled_operator(K, np.sqrt(W), 1.0)
	K0 = _scaled_operator(K, None, 0.0)
	live, op = [], None
	info = dict(deg=min(deg, n), steps=[], halvings=[], objective=[psi])
	try:
		op = engine.DeviceOperator(Ks, ctx=ctx)
		op0 = engine.DeviceOperator(K0, ctx=ctx)
		live.append(op0)
		plan = engine.LanczosPlan(op, 1, deg, orth_arg, basis="keep")
		live.append(plan)
		Out = engine.DeviceMatrix(n, 1, ctx=ctx)
		live.append(Out)
		converged, it = False, 0
		for it in range(1, max_iter + 1):
			sw = np.sqrt(W)
			Ks.set_diag_scale(sw)  # (forwarded to op: the plan's graph replays with the new values)
			b = W * f + grad
			kb = op0.matmat(b.reshape(-1, 1))[:, 0]
			rhs = sw * kb
			if np.any(rhs != 0.0):
				plan.set_probes(rhs.reshape(-1, 1))
				plan.run(0.0)
				plan.fun_action_into(Out, 0, "inv")
				info["steps"].append(plan.steps_done)
				sol = Out.get()[:, 0]
			else:
				sol = np.zeros(n)
			a_new = b - sw * sol
			if not np.all(np.isfinite(a_new)):
				raise FloatingPointError(f"laplace: the Newton step of iteration {it} is not finite")
			f_new = op0.matmat(a_new.reshape(-1, 1))[:, 0]
			da, df = a_new - a, f_new - f
			step, halv = 1.0, 0
			while True:
				a_try, f_try = a + step * da, f + step * df
				lp_try, grad_try, W_try = laplace_likelihood(likelihood, t, f_try)
				psi_try = lp_try - 0.5 * float(a_try @ f_try)
				## (a decrease within the rounding of Psi's own n-term sums is none: at the mode a full Newton step changes Psi by less)
				if psi_try >= psi - 8.0 * n * np.finfo(np.float64).eps * max(1.0, abs(psi)) or halv >= LAPLACE_MAX_HALVINGS:
					break
				step, halv = 0.5 * step, halv + 1
			delta = float(np.max(np.abs(f_try - f)))
			a, f, grad, W, psi = a_try, f_try, grad_try, W_try, psi_try
			info["halvings"].append(halv)
			info["objective"].append(psi)
			if delta <= tol * max(1.0, float(np.max(np.abs(f)))):
				converged = True
				break
		Ks.set_diag_scale(np.sqrt(W))  # B at the mode: what predict and log_marginal run on
		post = LaplacePosterior(K, likelihood, t, op, f, a, W, grad, it, converged, psi, deg, orth_arg, info)
		op = None
		return post
	finally:
		for obj in reversed(live):
			obj.close()
		if op is not None:
			op.close()
