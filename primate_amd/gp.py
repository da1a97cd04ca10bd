"""Gaussian-process prediction and log-determinants on the matrix-free kernel operator.

With A = K + noise I the operator of a `KernelOperator` on the training points X, C = outputscale * phi(r2(X*, X)) the
cross-covariance to new points X* (`KernelOperator.cross`, engine.KernelCross) and s the outputscale,

    mean = C A^-1 y,        var_i = s - (C A^-1 C^T)_ii.

With a pivoted-Cholesky preconditioner (`KernelOperator.preconditioned`, §4.18) M = P^{-1/2} and B = M A M,

    logdet A = tr log B + logdet P,        A^-1 y = M B^-1 M y,

which is what `logdet` computes and what `posterior(precond_rank > 0)` solves with: the path for small noise, where Lanczos on A
itself does not converge in any affordable number of steps.

Neither A nor C is ever formed: A^-1 is the Lanczos action `fun_action_into(..., "inv")` of a kept-basis plan over the device
operator, C and C^T are the cross-covariance products, and the contraction C A^-1 C^T of a batch is `DeviceMatrix.tn`.
"""

from __future__ import annotations

from typing import Optional

import numpy as np

from . import engine
from .lanczos import _as_device_operator
from .operators import _kernel_profile


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
	if getattr(K, "_slq_kind", None) != "kernel":
		raise ValueError("posterior needs a KernelOperator")
	if np.dtype(K.dtype) != np.float64:
		raise ValueError(f"posterior is fp64 only (the device matrices are fp64): the KernelOperator is {np.dtype(K.dtype)}")
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
		"""OUT[:, :b] = A^-1 RHS[:, :b] by `plan` (on solve_op); tmp: two n x b DeviceMatrix of scratch for the preconditioned path."""
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

	def keep(obj):
		live.append(obj)
		return obj

	info = dict(deg=min(deg, n), batches=0, steps=[], zero_columns=[])
	try:
		## alpha = A^-1 y over the non-zero columns of y, mean = C alpha
		nz = np.flatnonzero(np.any(yh != 0.0, axis=0))
		mean = np.zeros((m, q))
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
			for obj in (Mean, cross, Alpha, plan):
				obj.close()
		mean = mean[:, 0] if vector else mean
		if not variance:
			return mean, None, info

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
			return mean, cov, info
		return mean, var, info
	finally:
		for obj in reversed(live):
			obj.close()
