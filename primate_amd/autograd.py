"""tr f(A) as a differentiable torch function of the values of a sparse-CSR tensor on the GPU:

    loss = trace_fun(A_csr, "log", deg=30, count=256, seed=0)   # ~ log det A
    loss.backward()                                              # A_csr.values().grad ~ (A^-1) on the pattern

`forward` is one `primate_amd.grad.trace_grad` call with `pattern=A_csr` and probes drawn on the device: the value and the
gradient come out of the same runs, and the gradient stays in HBM (a clone of the accumulator's values). `backward` scales it.
The operator is rebuilt on every call - its values changed, which is the point.

`kernel_trace_fun` is the same for a Gaussian process's kernel matrix over points: differentiable with respect to lengthscale,
outputscale and noise (`primate_amd.grad.kernel_trace_grad`; d + 2 numbers, stored on the parameters' devices).

`gp_mll_fun` is the marginal log-likelihood of a Gaussian process, differentiable in the same three parameters through the
pivoted-Cholesky preconditioner (`primate_amd.gp.mll`): what a torch optimiser trains a GP with at small noise.
"""

from __future__ import annotations

import torch

from . import engine
from .grad import trace_grad

METHODS = ("lanczos", "chebyshev")


class _TraceFun(torch.autograd.Function):
	@staticmethod
	def forward(ctx, values, A_csr, opts):
		from .chebyshev import ChebyshevFunction
		from .operators import MatrixFunction

		## a tensor of its own: no operator cached on the caller's tensor survives a change of its values
		A = torch.sparse_csr_tensor(A_csr.crow_indices(), A_csr.col_indices(), values.detach().to(torch.float64), size=tuple(A_csr.shape))
		o = dict(opts)
		method, fun, deg, count, seed = (o.pop(k) for k in ("method", "fun", "deg", "count", "seed"))
		tg = {k: o.pop(k) for k in ("batch", "pdf", "symmetric", "dfun") if k in o}
		tg.setdefault("pdf", "device:rademacher")
		M = (MatrixFunction if method == "lanczos" else ChebyshevFunction)(A, fun, deg=deg, **o)
		try:
			est, grad, info = trace_grad(M, count=count, seed=seed, pattern=A, keep_device=True, **tg)
		finally:
			if hasattr(M, "close"):
				M.close()
		acc = info.get("accumulator")
		if acc is not None:
			try:
				G = torch.as_tensor(acc.cuda_array(), device=values.device).clone()
			finally:
				acc.close()
		else:  # (an exact gradient: it never was on the device)
			G = torch.from_numpy(grad).to(values.device)
		ctx.save_for_backward(G.to(values.dtype))
		return values.new_tensor(est)

	@staticmethod
	def backward(ctx, grad_output):
		(G,) = ctx.saved_tensors
		return grad_output * G, None, None


class _KernelTraceFun(torch.autograd.Function):
	@staticmethod
	def forward(ctx, lengthscale, outputscale, noise, X, opts, Xt=None):
		from .chebyshev import ChebyshevFunction
		from .grad import kernel_trace_grad
		from .operators import KernelOperator, MatrixFunction

		o = dict(opts)
		kernel, method, fun, deg, count, seed = (o.pop(k) for k in ("kernel", "method", "fun", "deg", "count", "seed"))
		tg = {k: o.pop(k) for k in ("batch", "pdf", "probes") if k in o}
		tg.setdefault("pdf", "device:rademacher")
		## an operator of its own on every call: its parameters changed, which is the point
		K = KernelOperator(X, kernel, lengthscale=lengthscale.detach().cpu().numpy().astype("float64"), outputscale=float(outputscale),
						   noise=float(noise), dtype="float64")  # fmt: skip
		M = (MatrixFunction if method == "lanczos" else ChebyshevFunction)(K, fun, deg=deg, **o)
		try:
			est, grads, _ = kernel_trace_grad(M, count=count, seed=seed, points=Xt is not None, **tg)
		finally:
			if hasattr(M, "close"):
				M.close()
		G = [torch.as_tensor(grads[k], dtype=p.dtype, device=p.device).reshape(p.shape)
			 for k, p in (("lengthscale", lengthscale), ("outputscale", outputscale), ("noise", noise))]  # fmt: skip
		ctx.with_points = Xt is not None
		if ctx.with_points:  # (Xt: the points as the tensor that asked for a gradient; X carries the same values)
			G.append(torch.as_tensor(grads["points"], dtype=Xt.dtype, device=Xt.device).reshape(Xt.shape))
		ctx.save_for_backward(*G)
		return lengthscale.new_tensor(est)

	@staticmethod
	def backward(ctx, grad_output):
		out = tuple(grad_output.to(G.device) * G for G in ctx.saved_tensors)
		return out[:3] + (None, None) + ((out[3],) if ctx.with_points else (None,))


class _GpMllFun(torch.autograd.Function):
	@staticmethod
	def forward(ctx, lengthscale, outputscale, noise, X, y, opts, Xt=None):
		from .gp import mll
		from .operators import KernelOperator

		o = dict(opts)
		kernel = o.pop("kernel")
		## an operator of its own on every call: its parameters changed, which is the point
		K = KernelOperator(X, kernel, lengthscale=lengthscale.detach().cpu().numpy().astype("float64"), outputscale=float(outputscale),
						   noise=float(noise), dtype="float64")  # fmt: skip
		value, grads, _ = mll(K, y, points=Xt is not None, **o)
		G = [torch.as_tensor(grads[k], dtype=p.dtype, device=p.device).reshape(p.shape)
			 for k, p in (("lengthscale", lengthscale), ("outputscale", outputscale), ("noise", noise))]  # fmt: skip
		ctx.with_points = Xt is not None
		if ctx.with_points:
			G.append(torch.as_tensor(grads["points"], dtype=Xt.dtype, device=Xt.device).reshape(Xt.shape))
		ctx.save_for_backward(*G)
		return lengthscale.new_tensor(value)

	@staticmethod
	def backward(ctx, grad_output):
		out = tuple(grad_output.to(G.device) * G for G in ctx.saved_tensors)
		return out[:3] + (None, None, None) + ((out[3],) if ctx.with_points else (None,))


def gp_mll_fun(X, y, kernel, lengthscale, outputscale, noise, rank: int = 100, deg: int = 20, count: int = 64, seed: int = 0, **kw):
	"""The marginal log-likelihood of a zero-mean Gaussian process over the points X with observations y (`primate_amd.gp.mll`,
	fp64) as a 0-d tensor differentiable with respect to the three parameter tensors `lengthscale` (0-d, one element, or one per
	dimension), `outputscale`, `noise` (floats are taken as constants). X: when it is a tensor with `requires_grad` (learned inputs,
	latent variables) it receives grad_output times `gp.mll(points=True)`'s grads["points"], the gradient with respect to the training
	points (one element of X per coordinate: an (n,) tensor is one dimension); otherwise the points are data, no point
	gradient is computed and every number keeps its bits. y gets NO gradient. Backward is
	grad_output times the gradients `gp.mll` returned: the gradient of the marginal likelihood itself (exact data-fit term, exact
	tr(P^-1 dA/dtheta), sampled remainder), not the derivative of the sampled value. Maximise it with any torch optimiser on
	`-gp_mll_fun(...)`. kw: solve_deg, batch, pdf, probes, control_variate go to `gp.mll`. The same seed gives the same bits."""
	Xt = X if isinstance(X, torch.Tensor) and X.requires_grad else None
	if isinstance(X, torch.Tensor):
		X = X.detach().cpu().numpy()
	if isinstance(y, torch.Tensor):
		y = y.detach().cpu().numpy()
	ls, s, v = (p if isinstance(p, torch.Tensor) else torch.as_tensor(p, dtype=torch.float64) for p in (lengthscale, outputscale, noise))
	if s.numel() != 1 or v.numel() != 1:
		raise ValueError("outputscale and noise are single numbers")
	unknown = set(kw) - {"solve_deg", "batch", "pdf", "probes", "control_variate"}
	if unknown:
		raise ValueError(f"gp_mll_fun: unknown arguments {sorted(unknown)}")
	opts = dict(kw, kernel=kernel, rank=int(rank), deg=int(deg), count=int(count), seed=int(seed))
	if Xt is None:
		return _GpMllFun.apply(ls, s, v, X, y, opts)
	return _GpMllFun.apply(ls, s, v, X, y, opts, Xt)


def kernel_trace_fun(X, kernel, lengthscale, outputscale, noise, fun="log", deg: int = 30, count: int = 256, seed: int = 0, method: str = "lanczos", **kw):
	"""The Girard-Hutchinson estimate of tr f(A), A = outputscale * phi(r2) + noise * I over the points X (the KernelOperator of
	`primate_amd.operators`), as a 0-d tensor differentiable with respect to the three parameter tensors: `lengthscale` (0-d, one
	element, or one per dimension), `outputscale`, `noise` (floats are taken as constants). X: when it is a tensor with
	`requires_grad` it receives grad_output times `kernel_trace_grad(points=True)`'s grads["points"] (the Lanczos
	method only - the Chebyshev route refuses); otherwise the points are data, no point gradient is computed and every number keeps
	its bits. The value and the gradients come out of the same `count` probes (primate_amd.grad.kernel_trace_grad, fp64); backward is
	grad_output times the stored gradients. method: "lanczos" (fun in log, exp, identity) or "chebyshev". kw: batch, pdf (default
	"device:rademacher"), probes go to kernel_trace_grad, everything else to the operator (orth=, t=, bounds=, ...). The same seed
	gives the same bits."""
	if method not in METHODS:
		raise ValueError(f"unknown method '{method}' (one of {', '.join(METHODS)})")
	if kw.get("diag_scale") is not None or getattr(X, "diag_scale", None) is not None:
		raise ValueError("kernel_trace_fun is not built for a KernelOperator with a diagonal scale (diag_scale / set_diag_scale): "
						 "use gp.fixed_noise_posterior for per-point noise and gp.laplace for a non-Gaussian likelihood")  # fmt: skip
	Xt = X if isinstance(X, torch.Tensor) and X.requires_grad else None
	if isinstance(X, torch.Tensor):
		X = X.detach()
	ls, s, v = (p if isinstance(p, torch.Tensor) else torch.as_tensor(p, dtype=torch.float64) for p in (lengthscale, outputscale, noise))
	if s.numel() != 1 or v.numel() != 1:
		raise ValueError("outputscale and noise are single numbers")
	opts = dict(kw, kernel=kernel, method=method, fun=fun, deg=int(deg), count=int(count), seed=int(seed))
	if Xt is None:
		return _KernelTraceFun.apply(ls, s, v, X, opts)
	return _KernelTraceFun.apply(ls, s, v, X, opts, Xt)


def trace_fun(A_csr, fun="log", deg: int = 30, count: int = 256, seed: int = 0, method: str = "lanczos", **kw):
	"""The Girard-Hutchinson estimate of tr f(A) as a 0-d tensor on A's device, differentiable with respect to `A_csr.values()`:
	the gradient is the estimate of f'(A) on A's own pattern from the same `count` probes (primate_amd.grad.trace_grad).
	A_csr: a symmetric fp64 torch sparse-CSR tensor on the GPU. method: "lanczos" (MatrixFunction: fun in log, exp, identity) or
	"chebyshev" (ChebyshevFunction; `dfun=` for a callable). kw: batch, pdf (default "device:rademacher"), symmetric, dfun go to
	trace_grad, everything else to the operator (orth=, t=, bounds=, damping=, ...). The same seed gives the same bits."""
	if getattr(A_csr, "_slq_kind", None) == "kernel_precond":
		raise ValueError("trace_fun: a preconditioned kernel operator is not differentiable here: gradients through the preconditioner are gp.logdet_grad's (autograd.gp_mll_fun)")
	if getattr(A_csr, "_slq_kind", None) == "kernel":
		raise ValueError("trace_fun differentiates the values of a sparse tensor: the hyperparameter gradients of a KernelOperator come from kernel_trace_fun")
	if not engine._is_torch_csr(A_csr):
		raise ValueError("trace_fun takes a torch sparse-CSR tensor")
	if method not in METHODS:
		raise ValueError(f"unknown method '{method}' (one of {', '.join(METHODS)})")
	if not A_csr.is_cuda:
		raise ValueError("a torch sparse-CSR operator must live on the GPU")
	opts = dict(kw, method=method, fun=fun, deg=int(deg), count=int(count), seed=int(seed))
	return _TraceFun.apply(A_csr.values(), A_csr, opts)
