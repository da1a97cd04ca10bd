"""Object layer over the C-ABI: Context (one GPU + stream), DeviceOperator (operator plugin
resident on that GPU) and LanczosPlan (workspace + state of one batched lock-step Lanczos run).

Everything numeric happens in libslq's HIP kernels; this file only marshals arrays.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _capi
from ._capi import check, ptr


def fun_spec(fun, **kwargs) -> tuple:
	"""Map a built-in spectral function name to (fun_id, params) following the defaults of the
	reference registry (src/primate/special.py:78-107). Returns (None, None) for Python callables,
	which are applied on the host to the returned nodes."""
	if fun is None:
		fun = "identity"
	if not isinstance(fun, str):
		return None, None
	assert fun in _capi.FUN_IDS, "If given as a string, matrix_function be one of the builtin functions."
	p = np.zeros(4)
	if fun == "exp":
		p[0] = kwargs.get("t", 1.0)
	elif fun == "smoothstep":
		p[0], p[1] = kwargs.get("a", 0.0), kwargs.get("b", 1.0)
	elif fun == "numrank":
		p[0], p[1] = kwargs.get("threshold", 0.000001), 1.0
	elif fun == "step":
		p[0], p[1] = kwargs.get("c", 0.0), float(kwargs.get("nonnegative", False))
	elif fun == "softsign":
		p[0] = kwargs.get("q", 10)
	return _capi.FUN_IDS[fun], p


class Context:
	"""One per (process, GPU). `device=None` picks LOCAL_RANK (torchrun) or the current device."""

	def __init__(self, device: Optional[int] = None, stream: Optional[int] = None):
		L = _capi.lib()
		if device is None:
			device = int(os.environ["LOCAL_RANK"]) if "LOCAL_RANK" in os.environ else -1
		h = C.c_void_p()
		check(L.slq_context_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h)))
		self._h = h
		d = C.c_int(-1)
		check(L.slq_context_device(h, C.byref(d)))
		self.device = int(d.value)  # the resolved ordinal: what owns every pointer and stream this context hands out

	def synchronize(self):
		check(_capi.lib().slq_context_synchronize(self._h))

	def measure_stream(self, mode: str = "triad", nbytes: int = 1 << 31, reps: int = 10) -> float:
		"""Measured device bandwidth in GB/s: mode 'read' (2 read streams), 'triad' (in place, 2R+1W) or 'copy'."""
		g = C.c_double()
		check(_capi.lib().slq_measure_stream(self._h, {"read": 0, "triad": 1, "copy": 2}[mode], int(nbytes), int(reps), C.byref(g)))
		return g.value

	def meminfo(self) -> tuple:
		f, t = C.c_size_t(), C.c_size_t()
		check(_capi.lib().slq_context_meminfo(self._h, C.byref(f), C.byref(t)))
		return f.value, t.value

	def close(self):
		if getattr(self, "_h", None):
			_capi.lib().slq_context_destroy(self._h)
			self._h = None

	def __del__(self):
		try:
			self.close()
		except Exception:  # noqa: BLE001
			pass


_default_ctx: Optional[Context] = None


def default_context() -> Context:
	global _default_ctx
	if _default_ctx is None:
		_default_ctx = Context()
	return _default_ctx


class _Handle:
	"""A C handle `_h` and its end: `close()` destroys it once (the class names the library's destroy entry), and so does garbage collection."""

	_destroy: str
	_h = None

	def close(self):
		if getattr(self, "_h", None):
			getattr(_capi.lib(), self._destroy)(self._h)
			self._h = None

	def __del__(self):
		try:
			self.close()
		except Exception:  # noqa: BLE001
			pass


class DeviceOperator(_Handle):
	"""Operator plugin resident on the GPU: the counterpart of the reference's C++ operator
	wrappers (src/primate/include/eigen_operators.h:17-104, src/primate/include/pylinop.h:16-73).

	Accepted inputs mirror the six overloads of the reference FFI
	(src/primate/_lanczos.cpp:102-112): ndarray (dense), scipy.sparse (any format; stored as CSR
	with int32 indices), or any object with `.matvec` and `.shape` (host-callback fallback); beyond them a
	torch sparse-CSR tensor that already lives on the context's GPU (slq_csr_create_device).
	"""

	_destroy = "slq_operator_destroy"

	def __init__(self, A, dtype=None, ctx: Optional[Context] = None):
		import scipy.sparse as sp

		self.ctx = ctx or default_context()
		L = _capi.lib()
		## a torch sparse-CSR tensor on the GPU: slq_csr_create_device (its arrays are read from HBM, never through numpy)
		torch_csr = type(A).__module__.split(".")[0] == "torch" and str(getattr(A, "layout", "")) == "torch.sparse_csr"
		if torch_csr and dtype is None:
			dtype = {"torch.float64": np.float64, "torch.float32": np.float32}[str(A.dtype)]
		if dtype is None:
			dtype = getattr(A, "dtype", np.float64)
		self.dtype = np.dtype(dtype)
		dt = _capi.dtype_id(self.dtype)
		assert hasattr(A, "shape") and len(A.shape) >= 2, "Operator must be at least two dimensional."
		assert A.shape[0] == A.shape[1], "This function only works with square, symmetric matrices!"
		self.shape = (int(A.shape[0]), int(A.shape[1]))
		self._keep = []
		h = C.c_void_p()
		if torch_csr:
			import torch

			if not A.is_cuda:
				raise ValueError("a torch sparse-CSR operator must live on the GPU (use scipy.sparse for host matrices)")
			if A.device.index != self.ctx.device:
				raise ValueError(f"the matrix is on {A.device}, the context on GPU {self.ctx.device}")
			tdt = torch.float64 if self.dtype == np.float64 else torch.float32
			crow = A.crow_indices().to(torch.int32).contiguous()
			col = A.col_indices().to(torch.int32).contiguous()  # (as they are: the library takes unsorted rows and duplicate columns)
			val = A.values().to(tdt).contiguous()
			torch.cuda.synchronize(A.device)
			check(L.slq_csr_create_device(self.ctx._h, dt, self.shape[0], int(val.numel()), C.c_void_p(crow.data_ptr()), C.c_void_p(col.data_ptr()),
										 C.c_void_p(val.data_ptr()), C.byref(h)))  # fmt: skip
			self.kind, self.nnz = "csr", int(val.numel())
		elif isinstance(A, np.ndarray):
			M = np.asfortranarray(A, dtype=self.dtype)
			check(L.slq_dense_create(self.ctx._h, dt, M.shape[0], ptr(M), M.shape[0], C.byref(h)))
			self.kind, self.nnz = "dense", M.size
		elif sp.issparse(A):
			M = sp.csr_matrix(A)  # (shares A's arrays when A is CSR already: nothing below writes to them)
			if M.dtype != self.dtype:
				M = M.astype(self.dtype)
			if not M.has_sorted_indices:
				M = M.sorted_indices()
			rowptr = np.ascontiguousarray(M.indptr, dtype=np.int32)
			colind = np.ascontiguousarray(M.indices, dtype=np.int32)
			vals = np.ascontiguousarray(M.data, dtype=self.dtype)
			check(L.slq_csr_create(self.ctx._h, dt, M.shape[0], M.nnz, ptr(rowptr), ptr(colind), ptr(vals), C.byref(h)))
			self.kind, self.nnz = "csr", int(M.nnz)
		elif getattr(A, "_slq_kind", None) == "gram":
			## x -> B^T (B x) for a rectangular sparse B (primate_amd.operators.GramOperator): slq_csr_gram_create
			M = sp.csr_matrix(A.A).astype(self.dtype)
			M.sort_indices()
			rowptr = np.ascontiguousarray(M.indptr, dtype=np.int32)
			colind = np.ascontiguousarray(M.indices, dtype=np.int32)
			vals = np.ascontiguousarray(M.data, dtype=self.dtype)
			check(L.slq_csr_gram_create(self.ctx._h, dt, M.shape[0], M.shape[1], M.nnz, ptr(rowptr), ptr(colind), ptr(vals), C.byref(h)))
			self.kind, self.nnz = "gram", int(M.nnz)
		elif getattr(A, "_slq_kind", None) == "affine":
			## A + t B (primate_amd.operators.AffineOperator): slq_csr_affine_create; t follows A.set_parameter
			Ma, Mb = (sp.csr_matrix(Z).astype(self.dtype) for Z in (A.A, A.B))
			for Z in (Ma, Mb):
				Z.sort_indices()
			arrs = [np.ascontiguousarray(Z.indptr, dtype=np.int32) for Z in (Ma, Mb)] + [np.ascontiguousarray(Z.indices, dtype=np.int32) for Z in (Ma, Mb)]
			va, vb = (np.ascontiguousarray(Z.data, dtype=self.dtype) for Z in (Ma, Mb))
			check(L.slq_csr_affine_create(self.ctx._h, dt, Ma.shape[0], Ma.nnz, ptr(arrs[0]), ptr(arrs[2]), ptr(va), Mb.nnz, ptr(arrs[1]), ptr(arrs[3]), ptr(vb), C.byref(h)))
			self.kind, self.nnz = "affine", int(Ma.nnz + Mb.nnz)
			self._h = h
			self.set_parameter(getattr(A, "t", 0.0))
			A._device_ops = getattr(A, "_device_ops", [])
			import weakref

			A._device_ops.append(weakref.ref(self))
		elif getattr(A, "_slq_kind", None) == "kernel":
			## matrix-free kernel operator (primate_amd.operators.KernelOperator): slq_kernel_create, or slq_kernel_create_device for
			## points that are a torch tensor on this context's GPU; the hyperparameters follow A.set_parameters
			if self.dtype != np.dtype(A.dtype):
				raise ValueError(f"the KernelOperator is {A.dtype}: its device operator cannot be {self.dtype} (the operator is defined on points rounded to its dtype)")
			ls = np.ascontiguousarray(A.lengthscale, dtype=np.float64)
			prof = _capi.KERNEL_PROFILES[A.kernel]
			n, d = A.X.shape
			Xd = getattr(A, "_X_device", None)
			if Xd is not None:
				import torch

				if Xd.device.index != self.ctx.device:
					raise ValueError(f"the points are on {Xd.device}, the context on GPU {self.ctx.device}")
				Xt = Xd.detach().reshape(n, d).to(torch.float64 if self.dtype == np.float64 else torch.float32).contiguous()
				torch.cuda.synchronize(Xd.device)
				check(L.slq_kernel_create_device(self.ctx._h, dt, n, d, C.c_void_p(Xt.data_ptr()), d, prof, ptr(ls), ls.size, float(A.outputscale), float(A.noise), C.byref(h)))
			else:
				check(L.slq_kernel_create(self.ctx._h, dt, n, d, ptr(A.X), d, prof, ptr(ls), ls.size, float(A.outputscale), float(A.noise), C.byref(h)))
			self.kind, self.nnz = "kernel", int(n * d)
			if getattr(A, "diag_scale", None) is not None:
				self._h = h  # (close() frees the handle if the scale is refused)
				self.set_kernel_diag_scale(A.diag_scale)
			A._device_ops = getattr(A, "_device_ops", [])
			import weakref

			A._device_ops.append(weakref.ref(self))
		elif getattr(A, "_slq_kind", None) == "kernel_precond":
			## B = M A M, M = P^{-1/2} of a pivoted-Cholesky factor (primate_amd.operators.PreconditionedKernelOperator):
			## slq_kernel_precond_create over the base's device operator, which this object keeps alive
			if self.dtype != np.float64:
				raise ValueError("a preconditioned kernel operator is fp64 only")
			from .lanczos import _as_device_operator

			self.base = _as_device_operator(A.base, dtype=np.float64)
			if self.base.ctx is not self.ctx:
				raise ValueError("the base operator's device operator lives in another context")
			check(L.slq_kernel_precond_create(self.ctx._h, self.base._h, int(A.rank_max), float(A.tol), C.byref(h)))
			self.kind, self.nnz = "kernel_precond", int(self.shape[0] * min(int(A.rank_max), self.shape[0]))
			self._host_params = A.base
			self._fresh_for = self._param_key()
		elif getattr(A, "_slq_kind", None) == "toeplitz":
			## Toeplitz operator (primate_amd.operators.ToeplitzOperator): slq_toeplitz_create; the values follow A.set_values
			if self.dtype != np.dtype(A.dtype):
				raise ValueError(f"the ToeplitzOperator is {A.dtype}: its device operator cannot be {self.dtype} (the operator is defined on values rounded to its dtype)")
			c64, r64 = (np.ascontiguousarray(v, dtype=np.float64) for v in (A.c, A.r))
			check(L.slq_toeplitz_create(self.ctx._h, dt, c64.size, ptr(c64), ptr(r64), C.byref(h)))
			self.kind, self.nnz = "toeplitz", int(2 * c64.size - 1)
			A._device_ops = getattr(A, "_device_ops", [])
			import weakref

			A._device_ops.append(weakref.ref(self))
		elif hasattr(A, "matmat_device"):
			## GPU-resident plugin: A.matmat_device(X, Y, stream) receives two objects with
			## `__cuda_array_interface__` (shape (ncols, n), C order = column-major n x ncols) and a stream handle
			n, np_dt = self.shape[0], self.dtype
			self.error = None

			def _dcb(_user, dx, dy, nn, ncols, stream):
				try:
					A.matmat_device(_CudaArrayView(dx, nn * ncols, self, (ncols, nn), np_dt), _CudaArrayView(dy, nn * ncols, self, (ncols, nn), np_dt), stream)
					return 0
				except Exception as e:  # noqa: BLE001
					self.error = e
					return 1

			dcb = _capi.DEVICE_MATMAT_FN(_dcb)
			self._keep.append(dcb)
			check(L.slq_device_callback_create(self.ctx._h, dt, n, dcb, None, C.byref(h)))
			self.kind, self.nnz = "device_callback", 0
		else:
			if not hasattr(A, "matvec"):
				raise ValueError("Supplied object is missing 'matvec' attribute.")
			n, np_dt = self.shape[0], self.dtype
			self.error = None

			def _cb(_user, x, y):
				try:
					ct = C.c_double if np_dt == np.float64 else C.c_float
					xin = np.ctypeslib.as_array(C.cast(x, C.POINTER(ct)), shape=(n,))
					out = np.asarray(A.matvec(xin.copy())).astype(np_dt, copy=False).ravel()
					np.ctypeslib.as_array(C.cast(y, C.POINTER(ct)), shape=(n,))[:] = out[:n]
					return 0
				except Exception as e:  # noqa: BLE001
					self.error = e
					return 1

			cb = _capi.MATVEC_FN(_cb)
			self._keep.append(cb)
			check(L.slq_callback_create(self.ctx._h, dt, n, cb, None, C.byref(h)))
			self.kind, self.nnz = "callback", 0
		self._h = h

	def set_parameter(self, t: float) -> None:
		"""t of an affine operator A + t B (SparseEigenAffineOperator::set_parameter, eigen_operators.h:134-136)."""
		check(_capi.lib().slq_operator_set_parameter(self._h, float(t)))

	def set_kernel_parameters(self, lengthscale, outputscale: float, noise: float) -> None:
		"""Hyperparameters of a kernel operator (slq_kernel_set_parameters): z, |z|^2 and the scalars are recomputed in place on the
		context stream; live plans, and the graphs they captured, see the new values from their next run."""
		ls = np.ascontiguousarray(np.atleast_1d(lengthscale), dtype=np.float64)
		check(_capi.lib().slq_kernel_set_parameters(self._h, ptr(ls), ls.size, float(outputscale), float(noise)))

	def set_toeplitz_values(self, c, r=None) -> None:
		"""c and r of a Toeplitz operator (slq_toeplitz_set_values): the symbol is rewritten in place; live plans, and the graphs they
		captured, compute with the new values from their next run. A change of symmetry is refused."""
		c64 = np.ascontiguousarray(c, dtype=np.float64)
		r64 = None if r is None else np.ascontiguousarray(r, dtype=np.float64)
		check(_capi.lib().slq_toeplitz_set_values(self._h, ptr(c64), ptr(r64), c64.size))

	def toeplitz_values(self) -> dict:
		"""The rounded c and r of a Toeplitz operator and whether it is symmetric (slq_toeplitz_get_values)."""
		n = self.shape[0]
		c, r, sym = np.empty(n), np.empty(n), C.c_int(0)
		check(_capi.lib().slq_toeplitz_get_values(self._h, ptr(c), ptr(r), n, C.byref(sym)))
		return {"c": c, "r": r, "symmetric": bool(sym.value)}

	def set_kernel_diag_scale(self, c) -> None:
		"""The diagonal scale of a kernel operator (slq_kernel_set_diag_scale): A = s diag(c) phi(r2) diag(c) + noise I,
		c of n entries, finite and >= 0, rounded once to the operator's dtype; None clears it. Live plans, and the graphs they captured,
		compute with the new state from their next run."""
		if c is None:
			check(_capi.lib().slq_kernel_set_diag_scale(self._h, None, 0))
			return
		c = np.ascontiguousarray(np.asarray(c, dtype=np.float64).ravel())
		check(_capi.lib().slq_kernel_set_diag_scale(self._h, ptr(c), c.size))

	def kernel_diag_scale(self):
		"""The diagonal scale as rounded to the operator's dtype (float64 array of n entries), or None when none is set
		(slq_kernel_get_diag_scale)."""
		L = _capi.lib()
		is_set = C.c_int()
		check(L.slq_kernel_get_diag_scale(self._h, None, 0, C.byref(is_set)))
		if not is_set.value:
			return None
		c = np.empty(self.shape[0])
		check(L.slq_kernel_get_diag_scale(self._h, ptr(c), c.size, None))
		return c

	def kernel_parameters(self) -> dict:
		"""What slq_kernel_get_parameters reports: d, kernel, the d lengthscales, outputscale, noise; and `scaled`: whether a diagonal
		scale is set (slq_kernel_get_diag_scale)."""
		L = _capi.lib()
		d, prof, s, v = C.c_int(), C.c_int(), C.c_double(), C.c_double()
		check(L.slq_kernel_get_parameters(self._h, C.byref(d), C.byref(prof), None, 0, C.byref(s), C.byref(v)))
		ls = np.empty(d.value)
		check(L.slq_kernel_get_parameters(self._h, None, None, ptr(ls), d.value, None, None))
		name = {v_: k for k, v_ in _capi.KERNEL_PROFILES.items()}[prof.value]
		is_set = C.c_int()
		check(L.slq_kernel_get_diag_scale(self._h, None, 0, C.byref(is_set)))
		return dict(d=d.value, kernel=name, lengthscale=ls, outputscale=s.value, noise=v.value, scaled=bool(is_set.value))

	## ---- a preconditioned kernel operator (kind "kernel_precond"; slq_kernel_precond_*) ----
	def _need_precond(self, what: str) -> None:
		if self.kind != "kernel_precond":
			raise ValueError(f"{what} needs a preconditioned kernel operator, not kind '{self.kind}'")

	def refresh(self) -> None:
		"""Refactor in place for the base's hyperparameters of now (slq_kernel_precond_refresh): same rank_max, same addresses."""
		self._need_precond("refresh")
		check(_capi.lib().slq_kernel_precond_refresh(self._h))
		self._fresh_for = self._param_key()

	def _param_key(self):
		K = self._host_params
		return (tuple(np.atleast_1d(K.lengthscale).tolist()), float(K.outputscale), float(K.noise))

	def refresh_if_stale(self) -> None:
		"""The lazy refresh: refactor when the base's parameters have changed since the factor was built."""
		self._need_precond("refresh_if_stale")
		if self._fresh_for != self._param_key():
			self.refresh()

	def info(self) -> dict:
		"""{rank_max, rank, logdet_p, residual_trace, t_max} of the factor (slq_kernel_precond_info)."""
		self._need_precond("info")
		rm, r, ld, rt, tm = C.c_int(), C.c_int(), C.c_double(), C.c_double(), C.c_double()
		check(_capi.lib().slq_kernel_precond_info(self._h, C.byref(rm), C.byref(r), C.byref(ld), C.byref(rt), C.byref(tm)))
		return dict(rank_max=rm.value, rank=r.value, logdet_p=ld.value, residual_trace=rt.value, t_max=tm.value)

	def factor(self) -> dict:
		"""{pivots, L, G, eig, H} as the device holds them (slq_kernel_precond_get, slq_debug_kernel_precond_h): pivots (rank_max, -1
		beyond the rank), L (n x rank_max), G and H = (L^T L + noise I)^-1 (rank_max x rank_max), the eigenvalues of L^T L."""
		self._need_precond("factor")
		r, n = self.info()["rank_max"], self.shape[0]
		piv, Lf, G, eig = np.empty(r, dtype=np.int32), np.empty((n, r), order="F"), np.empty((r, r)), np.empty(r)
		check(_capi.lib().slq_kernel_precond_get(self._h, ptr(piv), ptr(Lf), n, ptr(G), ptr(eig)))
		H = np.empty((r, r))
		check(_capi.lib().slq_debug_kernel_precond_h(self._h, ptr(H)))
		return dict(pivots=piv, L=Lf, G=G, eig=eig, H=H)

	def inv_sqrt(self, X: np.ndarray) -> np.ndarray:
		"""P^{-1/2} X for a host array (slq_kernel_precond_apply)."""
		self._need_precond("inv_sqrt")
		X = np.asfortranarray(np.asarray(X, dtype=np.float64).reshape(self.shape[0], -1))
		Y = np.empty_like(X, order="F")
		check(_capi.lib().slq_kernel_precond_apply(self._h, ptr(X), X.shape[0], ptr(Y), Y.shape[0], X.shape[1]))
		return Y

	def inv_sqrt_dmat(self, IN: "DeviceMatrix", i0: int, OUT: "DeviceMatrix", o0: int, b: int) -> None:
		"""OUT[:, o0:o0+b] = P^{-1/2} IN[:, i0:i0+b] between DeviceMatrix columns, asynchronous on the context stream."""
		self._need_precond("inv_sqrt_dmat")
		check(_capi.lib().slq_kernel_precond_apply_dmat(self._h, IN._h, int(i0), OUT._h, int(o0), int(b)))

	def factor_columns(self, which: int, c0: int, nc: int, OUT: "DeviceMatrix", o0: int = 0) -> None:
		"""OUT[:, o0:o0+nc] = columns [c0, c0 + nc) of L (which = 0: a copy) or of L H (which = 1: on the matrix cores), nc <= 64
		(slq_kernel_precond_columns): the factor as operand columns of a KernelGradAccumulator. Asynchronous."""
		self._need_precond("factor_columns")
		check(_capi.lib().slq_kernel_precond_columns(self._h, int(which), int(c0), int(nc), OUT._h, int(o0)))

	def precond_trace_grad(self, acc: "KernelGradAccumulator", alpha: float = 1.0, beta: float = 0.0) -> None:
		"""acc's values = beta * values + alpha * tr(P^-1 dA/dtheta), exactly (slq_kernel_precond_trace_grad): `acc` is an accumulator
		on this operator's BASE. Deterministic, asynchronous; acc's column count is unchanged."""
		self._need_precond("precond_trace_grad")
		check(_capi.lib().slq_kernel_precond_trace_grad(self._h, acc._h, float(alpha), float(beta)))

	def precond_trace_point_grad(self, acc: "KernelPointGradAccumulator", alpha: float = 1.0, beta: float = 0.0) -> None:
		"""acc's values = beta * values + alpha * tr(P^-1 dA/dx), exactly (slq_kernel_precond_trace_pointgrad): `acc` is a training-form
		point-gradient accumulator on this operator's BASE. Deterministic, asynchronous; acc's column count is unchanged."""
		self._need_precond("precond_trace_point_grad")
		check(_capi.lib().slq_kernel_precond_trace_pointgrad(self._h, acc._h, float(alpha), float(beta)))

	def factor_timing(self) -> dict:
		"""Wall time of the last factorisation in ms: device_ms (the launches up to the synchronisation), host_ms (Jacobi, G, its upload)."""
		self._need_precond("factor_timing")
		out = (C.c_double * 2)()
		check(_capi.lib().slq_debug_kernel_precond_timing(self._h, out))
		return dict(device_ms=float(out[0]), host_ms=float(out[1]))

	def precond_addresses(self) -> tuple:
		"""The device addresses of L, G, the pivots and the residual diagonal (slq_debug_kernel_precond_addresses)."""
		self._need_precond("precond_addresses")
		out = (C.c_uint64 * 4)()
		check(_capi.lib().slq_debug_kernel_precond_addresses(self._h, out))
		return tuple(int(v) for v in out)

	def matmat(self, X: np.ndarray) -> np.ndarray:
		X = np.asfortranarray(X.reshape(self.shape[1], -1), dtype=self.dtype)
		Y = np.empty_like(X, order="F")
		check(_capi.lib().slq_operator_matmat(self._h, ptr(X), X.shape[0], ptr(Y), Y.shape[0], X.shape[1]))
		return Y


BASIS_MODES = {None: 0, "keep": 1, "recompute": 2}


def _basis_arg(keep_basis: bool = False, basis: Optional[str] = None, auto: bool = False) -> Optional[str]:
	"""The plan kind behind (keep_basis, basis): None (ring only), "keep", "recompute", or - where `auto` admits it - "auto".
	Checked before the library is touched."""
	names = ("keep", "recompute") + (("auto",) if auto else ())
	if basis is not None and (not isinstance(basis, str) or basis not in names):
		raise ValueError(f"basis must be one of {names} (or None), not {basis!r}")
	if keep_basis and basis not in (None, "keep"):
		raise ValueError(f"keep_basis=True contradicts basis={basis!r}")
	return "keep" if (keep_basis and basis is None) else basis


def plan_query_bytes(dtype, n: int, nprobes: int, deg: int, orth: int = 0, basis: Optional[str] = None) -> int:
	"""Device bytes of the Lanczos panels a plan of this shape would hold (host arithmetic, nothing is allocated): `basis` None
	the ring of a quadrature plan, "keep" the deg + 1 slots of a kept basis, "recompute" ring + probe stash + output of a
	two-pass plan (independent of deg)."""
	basis = _basis_arg(False, basis)
	b = C.c_size_t()
	if basis == "recompute":
		check(_capi.lib().slq_plan_query_bytes_recompute(_capi.dtype_id(dtype), int(n), int(nprobes), int(deg), int(orth), C.byref(b)))
	else:
		check(_capi.lib().slq_plan_query_bytes(_capi.dtype_id(dtype), int(n), int(nprobes), int(deg), int(orth), int(basis == "keep"), C.byref(b)))
	return int(b.value)


class LanczosPlan(_Handle):
	"""Workspace + state of one batched lock-step Lanczos run over `nprobes` probes.

	`basis` (or the older `keep_basis=True`, which is `basis="keep"`) says what the f(A)v action runs on: "keep" retains all deg
	Lanczos vectors (deg + 1 panels); "recompute" keeps none - `fun_action`, `fun_action_into` and `DiagAccumulator.update`
	replay the run (two-pass Lanczos) and add g_t W_t into an output panel as the vectors pass through a short ring: a
	footprint independent of deg, one more run per action call. None: a quadrature plan (no action)."""

	_destroy = "slq_plan_destroy"

	def __init__(self, op: DeviceOperator, nprobes: int, deg: int, orth: int = 0, keep_basis: bool = False, basis: Optional[str] = None):
		basis = _basis_arg(keep_basis, basis)
		self.op = op
		n = op.shape[0]
		self.nprobes = int(nprobes)
		self.deg = min(int(deg), n)
		self.orth = self.deg if orth < 0 or orth > self.deg else int(orth)
		self.keep_basis = basis == "keep"
		self.basis_kind = basis
		h = C.c_void_p()
		if basis == "recompute":
			check(_capi.lib().slq_plan_create_recompute(op.ctx._h, op._h, self.nprobes, int(deg), int(orth), C.byref(h)))
		else:
			check(_capi.lib().slq_plan_create(op.ctx._h, op._h, self.nprobes, int(deg), int(orth), int(self.keep_basis), C.byref(h)))
		self._h = h

	@property
	def basis_mode(self) -> int:
		"""0 ring only, 1 kept basis, 2 recompute (slq_plan_basis_mode)."""
		return self.basis_info()["mode"]

	def basis_info(self) -> dict:
		"""{mode, ring_slots, acc_cols}: acc_cols = ring columns one accumulation launch of a recompute plan consumes."""
		m, s, a = C.c_int(), C.c_int(), C.c_int()
		check(_capi.lib().slq_plan_basis_mode(self._h, C.byref(m), C.byref(s), C.byref(a)))
		return {"mode": int(m.value), "ring_slots": int(s.value), "acc_cols": int(a.value)}

	@property
	def workspace_bytes(self) -> int:
		b = C.c_size_t()
		check(_capi.lib().slq_plan_workspace_bytes(self._h, C.byref(b)))
		return b.value

	def describe(self) -> dict:
		"""Panel geometry and launch sequence the library chose for this plan (slq_plan_describe)."""
		info = _capi.PlanInfo()
		check(_capi.lib().slq_plan_describe(self._h, C.byref(info)))
		d = {k: getattr(info, k) for k, _ in _capi.PlanInfo._fields_}
		d["sequence"] = {0: "sweeps", 1: "fused", 2: "fused_stored_u", 4: "fused_gram"}[d["sequence"]]
		mode = C.c_int()
		check(_capi.lib().slq_plan_window_verify(self._h, C.byref(mode), None))
		d["omega"] = int(mode.value)  # the window's oldest column is read only where needed (1), verify mode (2), not offered (0)
		kernel, ksplit = C.c_int(), C.c_int()
		check(_capi.lib().slq_plan_dense_path(self._h, C.byref(kernel), C.byref(ksplit)))
		## dense operators: 1 k_dense_panel, 2 k_dense_mfma_3term, 3 k_dense_mfma_tile, 4 k_dense_mfma_lds, 5 k_dense_mfma32_lds (0: not dense); K slabs
		d["dense_kernel"], d["dense_ksplit"] = int(kernel.value), int(ksplit.value)
		return d

	def set_probes(self, X: np.ndarray):
		X = np.asarray(X)
		X = X.reshape(-1, 1) if X.ndim == 1 else X
		assert X.shape == (self.op.shape[1], self.nprobes), f"probes must be {(self.op.shape[1], self.nprobes)}"
		X = np.asfortranarray(X, dtype=self.op.dtype)
		check(_capi.lib().slq_plan_set_probes(self._h, ptr(X), X.shape[0]))

	def set_probes_device(self, dptr: int):
		"""Probes already resident on this GPU: `dptr` is a device address of a contiguous column-major
		n x nprobes array of the operator dtype (e.g. torch_tensor.data_ptr() of a (nprobes, n) C-ordered
		tensor)."""
		check(_capi.lib().slq_plan_set_probes_device(self._h, C.c_void_p(int(dptr)), self.op.shape[0]))

	def generate_probes(self, pdf: str = "rademacher", seed: int = 0, probe_offset: int = 0):
		assert pdf in _capi.PDF_IDS, f"Invalid distribution '{pdf}' supplied."
		check(_capi.lib().slq_plan_generate_probes(self._h, _capi.PDF_IDS[pdf], int(seed), int(probe_offset)))

	def get_probes(self) -> np.ndarray:
		X = np.empty((self.op.shape[0], self.nprobes), dtype=self.op.dtype, order="F")
		check(_capi.lib().slq_plan_get_probes(self._h, ptr(X), X.shape[0]))
		return X

	def get_probes_into(self, out: "DeviceMatrix", o0: int):
		"""The current probes (as used: sphere draws have norm sqrt(n)) into columns [o0, o0 + nprobes) of `out`."""
		check(_capi.lib().slq_plan_get_probes_dmat(self._h, out._h, int(o0)))

	def run(self, rtol: float = 1e-8, upto: Optional[int] = None):
		"""All `deg` steps (slq_plan_run), or with `upto` the steps [steps_done, upto) of a resumable run
		(slq_plan_run_steps): the same launches, the state stays on the device between the stages."""
		if upto is None:
			rc = _capi.lib().slq_plan_run(self._h, float(rtol))
		else:
			rc = _capi.lib().slq_plan_run_steps(self._h, float(rtol), int(upto))
		if rc == _capi.SLQ_ECALLBACK and getattr(self.op, "error", None) is not None:
			raise self.op.error
		check(rc)

	@property
	def steps_done(self) -> int:
		"""Lanczos steps done since the probes were set or generated."""
		c = C.c_int()
		check(_capi.lib().slq_plan_steps_done(self._h, C.byref(c)))
		return int(c.value)

	def quadrature_at(self, m: Optional[int] = None, fun="identity", rule: str = "gauss", endpoint: Optional[float] = None,
					  return_rule: bool = False, return_stage: bool = False, **fun_kwargs):  # fmt: skip
		"""Quadrature of the first `m` steps of the run as it stands (default: all steps done; slq_plan_quadrature_at).
		rule "gauss": the m-point Gauss rule, what a run of degree m returns. rule "radau": the (m+1)-point Gauss-Radau
		rule with a node at `endpoint` <= lambda_min(A), which brackets v^T f(A) v together with the Gauss value for f
		whose derivatives keep one sign. Returns quad, then (nodes, weights) with return_rule, then with return_stage the
		four doubles {sum quad, sum quad^2, sum |quad - gauss|, nprobes} reduced on the device."""
		rid, endpoint = _rule_args(rule, endpoint)
		fid, params = fun_spec(fun, **fun_kwargs)
		if fid is None and return_stage:
			raise ValueError("the stage statistics are reduced on the device: built-in function names only")
		host_fun = fid is None
		m = self.steps_done if m is None else int(m)
		want_rule = return_rule or host_fun
		k = m + rid
		quad = np.zeros(self.nprobes)
		nodes = np.zeros((self.nprobes, k)) if want_rule and k > 0 else None
		weights = np.zeros((self.nprobes, k)) if want_rule and k > 0 else None
		stage = np.zeros(4) if return_stage else None
		check(_capi.lib().slq_plan_quadrature_at(self._h, m, rid, endpoint, 0 if host_fun else fid, ptr(params), ptr(quad), ptr(nodes),
												 ptr(weights), ptr(stage)))  # fmt: skip
		if host_fun:  # (as `quadrature`: the callable on the host over the nodes, ||v||^2 from the identity's value)
			ident = np.sum(nodes * weights, axis=1)
			vn2 = np.divide(quad, ident, out=np.zeros_like(quad), where=ident != 0)
			quad = np.array([np.sum(fun(nodes[i]) * weights[i]) for i in range(self.nprobes)]) * vn2
		out = (quad,) + ((nodes, weights) if return_rule else ()) + ((stage,) if return_stage else ())
		return out[0] if len(out) == 1 else out

	def closing(self) -> dict:
		"""{lazy, pending} (slq_plan_closing_state): runs of this plan leave the update pass of their last step to the first entry that
		asks for beta_deg (`tridiag`, the Gauss-Radau rule at m = deg, the window diagnostics); the last run's is still outstanding."""
		lazy, pending = C.c_int(), C.c_int()
		check(_capi.lib().slq_plan_closing_state(self._h, C.byref(lazy), C.byref(pending)))
		return {"lazy": bool(lazy.value), "pending": bool(pending.value)}

	def tridiag(self) -> tuple:
		"""(alpha, beta, steps): alpha/beta are (nprobes, deg+1) with beta[:, 0] = 0. beta[:, deg] of a plan without a kept
		basis is computed by this call where the run left it out (`closing`)."""
		a = np.zeros((self.nprobes, self.deg + 1), dtype=self.op.dtype)
		b = np.zeros((self.nprobes, self.deg + 1), dtype=self.op.dtype)
		s = np.zeros(self.nprobes, dtype=np.int32)
		check(_capi.lib().slq_plan_get_tridiag(self._h, ptr(a), ptr(b), ptr(s)))
		return a, b, s

	def quadrature(self, fun="identity", return_rule: bool = False, **fun_kwargs):
		"""quad[i] = sum_k f(nodes[i,k]) weights[i,k] ||v_i||^2 ; optionally also (nodes, weights)."""
		fid, params = fun_spec(fun, **fun_kwargs)
		host_fun = fid is None
		want_rule = return_rule or host_fun
		quad = np.zeros(self.nprobes)
		nodes = np.zeros((self.nprobes, self.deg)) if want_rule else None
		weights = np.zeros((self.nprobes, self.deg)) if want_rule else None
		check(
			_capi.lib().slq_plan_quadrature(
				self._h, 0 if host_fun else fid, ptr(params), ptr(quad), ptr(nodes), ptr(weights)
			)
		)
		if host_fun:
			## arbitrary Python callables run on the host over the P x k nodes (operators.py:150);
			## the device returned sum(nodes*weights)*||v||^2, so ||v||^2 is recovered exactly
			ident = np.sum(nodes * weights, axis=1)
			vn2 = np.divide(quad, ident, out=np.zeros_like(quad), where=ident != 0)
			self._vnorm2 = vn2
			quad = np.array([np.sum(fun(nodes[i]) * weights[i]) for i in range(self.nprobes)]) * vn2
		return (quad, nodes, weights) if return_rule else quad

	def fun_action(self, fun="identity", **fun_kwargs) -> np.ndarray:
		"""Y[:, i] = f(A) x_i from the retained basis (basis="keep") or by replaying the run (basis="recompute": every call
		costs one more run); built-in `fun` names only."""
		fid, params = fun_spec(fun, **fun_kwargs)
		assert fid is not None, "fun_action evaluates built-in function names on the device"
		Y = np.zeros((self.op.shape[0], self.nprobes), dtype=self.op.dtype, order="F")
		check(_capi.lib().slq_plan_fun_action(self._h, fid, ptr(params), ptr(Y), Y.shape[0]))
		return Y

	def fun_action_into(self, out: "DeviceMatrix", o0: int, fun="identity", **fun_kwargs):
		"""f(A) X of this run written straight into columns [o0, o0 + nprobes) of a DeviceMatrix."""
		fid, params = fun_spec(fun, **fun_kwargs)
		assert fid is not None
		check(_capi.lib().slq_plan_fun_action_dmat(self._h, fid, ptr(params), out._h, int(o0)))

	def basis(self, probe: int = 0) -> np.ndarray:
		if getattr(self, "basis_kind", None) == "recompute":
			raise ValueError("a recompute plan holds no basis: create the plan with basis='keep'")
		Q = np.zeros((self.op.shape[0], self.deg), dtype=self.op.dtype, order="F")
		check(_capi.lib().slq_plan_get_basis(self._h, int(probe), ptr(Q), Q.shape[0]))
		return Q

	def profile_enable(self, enable: bool = True):
		check(_capi.lib().slq_plan_profile_enable(self._h, int(enable)))

	def profile_read(self, reset: bool = True) -> dict:
		pr = _capi.SlqProfile()
		check(_capi.lib().slq_plan_profile_read(self._h, C.byref(pr), int(reset)))
		return {k: {"ms": pr.ms[i], "launches": pr.launches[i]} for i, k in enumerate(_capi.KERNEL_CLASSES)}

	def sweep_columns(self, reset: bool = True) -> tuple:
		"""(read, offered): ring columns the deep-window update sweeps actually read against the ones their windows hold, summed over launches and panels - the
		sweep skips a column whose projection is below the reference's threshold for every probe of the panel (slq_plan_sweep_columns)."""
		a, b = C.c_uint64(), C.c_uint64()
		check(_capi.lib().slq_plan_sweep_columns(self._h, C.byref(a), C.byref(b), int(reset)))
		return int(a.value), int(b.value)

	def window_columns(self, reset: bool = False) -> dict:
		"""Accounting of the window's oldest column in the Gram sequence (slq_plan_window_columns), summed over steps and panels since the last
		reset: columns offered and read, rescues, verify-mode violations, read -> skip transitions. The last step of a run is counted when
		its closing tail is launched (`closing`): this call and `tridiag` do that, new probes drop it - read the counters after each run
		for sums over every step."""
		out = (C.c_int64 * 5)()
		check(_capi.lib().slq_plan_window_columns(self._h, out, int(reset)))
		return dict(zip(("offered", "read", "rescues", "violations", "transitions"), (int(v) for v in out)))

	def window_verify(self) -> dict:
		"""What SLQ_OMEGA=2 runs have recorded since the counters' last reset (slq_plan_window_verify): the largest one-step innovation in units of
		eps ||A||_inf, the smallest (tol - |measured|) / rho, and the certificate's constants."""
		out = (C.c_double * 5)()
		check(_capi.lib().slq_plan_window_verify(self._h, None, out))
		return dict(zip(("innovation", "margin", "c", "kappa", "norm_inf"), (float(v) for v in out)))

	def window_flags(self) -> tuple:
		"""(read, rescue), each [deg + 1, panels]: where the update pass of step j read the window's oldest column, and where its entry was
		measured by the rescue kernel, in the last run (slq_plan_window_flags; zero rows for steps that were not offered)."""
		panels = self.describe()["panels"]
		rd = np.zeros((self.deg + 1, panels), dtype=np.int32)
		rs = np.zeros((self.deg + 1, panels), dtype=np.int32)
		i32 = C.POINTER(C.c_int32)
		check(_capi.lib().slq_plan_window_flags(self._h, rd.ctypes.data_as(i32), rs.ctypes.data_as(i32), rd.size))
		return rd, rs

	def window_census(self) -> np.ndarray:
		"""[deg + 1, 9, panels] probes with a non-zero projection coefficient per step, window position and panel in the last run
		(plans of the ring-fed Gram sequence created under SLQ_OMEGA=2; slq_plan_window_census)."""
		panels = self.describe()["panels"]
		out = np.zeros((self.deg + 1, 9, panels), dtype=np.int32)
		check(_capi.lib().slq_plan_window_census(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size))
		return out

	def action_columns(self, reset: bool = True) -> tuple:
		"""(read, offered): ring columns the accumulation launches of a recompute plan's replays read against the ones they were offered, summed
		over launches and panels - a column whose coefficient is zero for every probe of a panel is skipped (slq_plan_action_columns)."""
		a, b = C.c_uint64(), C.c_uint64()
		check(_capi.lib().slq_plan_action_columns(self._h, C.byref(a), C.byref(b), int(reset)))
		return int(a.value), int(b.value)


RULE_IDS = {"gauss": 0, "radau": 1}
## stage every DEG_STEP Lanczos steps unless told otherwise (the cost of a stage against a step)
DEG_STEP = 5


class ChebyshevPlan(LanczosPlan):
	"""Workspace + state of one batched Chebyshev run (the kernel polynomial method; slq_plan_create_chebyshev): `nsteps`
	steps w_{j+1} = 2 A~ w_j - w_{j-1}, A~ = (A - c) / h, give the moments mu_k = v^T T_k(A~) v for k = 0 .. 2 nsteps per
	probe. No orthogonality, no eigensolve, no cap at 512 steps (nsteps <= 16384). The probe methods, `describe`,
	`workspace_bytes`, `profile_*` and `close` are LanczosPlan's; its Lanczos entries raise ValueError on such a plan.
	action=True (slq_plan_create_chebyshev_action): the plan also evaluates Y = sum_{k <= nsteps} c_k T_k(A~) X - `action`,
	`action_into` - on a ring of `acc_cols` slots with one output panel behind it, whatever nsteps is; `run`, `moments` and
	`moment_sum` work on it as on a plain plan and give the same bits."""

	def __init__(self, op: DeviceOperator, nprobes: int, nsteps: int, action: bool = False):
		self.op = op
		self.nprobes = int(nprobes)
		self.nsteps = int(nsteps)
		self.nmoments = 2 * self.nsteps + 1
		self.deg, self.orth, self.keep_basis, self.basis_kind = self.nsteps, 0, False, None
		self.bounds = None
		h = C.c_void_p()
		self.is_action = bool(action)
		create = _capi.lib().slq_plan_create_chebyshev_action if self.is_action else _capi.lib().slq_plan_create_chebyshev
		check(create(op.ctx._h, op._h, self.nprobes, self.nsteps, C.byref(h)))
		self._h = h

	def describe(self) -> dict:
		"""LanczosPlan.describe() and `acc_cols`: ring columns one accumulation launch of an action plan consumes (0: a plain plan);
		`ring_slots` is 2 for a plain plan and min(acc_cols, nsteps + 1) for an action plan."""
		d = super().describe()
		d["acc_cols"] = self.basis_info()["acc_cols"]
		return d

	def _action_args(self, bounds, coef) -> tuple:
		if not self.is_action:
			raise ValueError("not an action plan: create it with ChebyshevPlan(op, nprobes, nsteps, action=True)")
		try:
			a, b = (float(v) for v in bounds)
		except (TypeError, ValueError):
			raise ValueError(f"bounds must be a pair (a, b), got {bounds!r}") from None
		if not (np.isfinite(a) and np.isfinite(b) and a < b):
			raise ValueError(f"bounds must be finite with a < b, got {bounds!r}")
		coef = np.ascontiguousarray(coef, dtype=np.float64).ravel()
		if coef.size != self.nsteps + 1:
			raise ValueError(f"{coef.size} coefficients for a plan of {self.nsteps} steps: it takes {self.nsteps + 1} (c_0 .. c_nsteps)")
		if not np.all(np.isfinite(coef)):
			raise ValueError("the coefficients must be finite")
		return a, b, coef

	def _action_rc(self, rc: int, a: float, b: float):
		if rc == _capi.SLQ_ECALLBACK and getattr(self.op, "error", None) is not None:
			raise self.op.error
		if rc == _capi.SLQ_OK or "not inside the bounds" in _capi.lib().slq_last_error().decode(errors="replace"):
			self.bounds = (a, b)  # (the run took place: the moments and flags are those of these bounds)
		check(rc)

	def action(self, bounds, coef, outside_tol: float = 0.0) -> np.ndarray:
		"""Y (n, nprobes), Fortran-ordered: sum_k coef[k] T_k(A~) x_i for the probes set last (slq_plan_chebyshev_action), with
		coef = c_0 .. c_nsteps - the Chebyshev coefficients of f on `bounds` (chebyshev.chebyshev_coefficients) give f(A) x_i.
		One run of nsteps steps; the moments and flags of that run are left behind (`moments`, `moment_sum`). ValueError if the
		bounds miss part of the spectrum (an `outside` flag), and for device-drawn sphere probes."""
		a, b, coef = self._action_args(bounds, coef)
		Y = np.zeros((self.op.shape[0], self.nprobes), dtype=self.op.dtype, order="F")
		rc = _capi.lib().slq_plan_chebyshev_action(self._h, 0.5 * (a + b), 0.5 * (b - a), float(outside_tol), int(coef.size), ptr(coef), ptr(Y), Y.shape[0])
		self._action_rc(rc, a, b)
		return Y

	def action_into(self, bounds, coef, out: "DeviceMatrix", o0: int, outside_tol: float = 0.0):
		"""The same, written straight into columns [o0, o0 + nprobes) of a DeviceMatrix (fp64 plans; slq_plan_chebyshev_action_dmat)."""
		a, b, coef = self._action_args(bounds, coef)
		rc = _capi.lib().slq_plan_chebyshev_action_dmat(self._h, 0.5 * (a + b), 0.5 * (b - a), float(outside_tol), int(coef.size), ptr(coef), out._h, int(o0))
		self._action_rc(rc, a, b)

	def run(self, bounds, outside_tol: float = 0.0):
		"""Enqueue the nsteps steps for the probes set or generated last. bounds = (a, b) must contain the spectrum:
		where it does not, the probe's `outside` flag goes up (|mu_k| > (1 + outside_tol) mu_0; 0: the library's default)."""
		a, b = (float(v) for v in bounds)
		if not (np.isfinite(a) and np.isfinite(b) and a < b):
			raise ValueError(f"bounds must be finite with a < b, got {bounds!r}")
		rc = _capi.lib().slq_plan_run_chebyshev(self._h, 0.5 * (a + b), 0.5 * (b - a), float(outside_tol))
		if rc == _capi.SLQ_ECALLBACK and getattr(self.op, "error", None) is not None:
			raise self.op.error
		check(rc)
		self.bounds = (a, b)

	def moments(self, return_outside: bool = False):
		"""mu (nprobes, 2 nsteps + 1) of the last run, and with return_outside the per-probe flags (slq_plan_get_moments)."""
		mu = np.zeros((self.nprobes, self.nmoments))
		out = np.zeros(self.nprobes, dtype=np.int32)
		check(_capi.lib().slq_plan_get_moments(self._h, ptr(mu), ptr(out)))
		return (mu, out) if return_outside else mu

	def moment_sum(self, coef: np.ndarray, return_stage: bool = False):
		"""quad[i] = sum_k coef[k] mu[i, k], reduced on the device (slq_plan_moment_sum): with the Chebyshev coefficients of f
		on the bounds of the run (chebyshev.chebyshev_coefficients), v_i^T f(A) v_i. ValueError if an `outside` flag is up."""
		coef = np.ascontiguousarray(coef, dtype=np.float64).ravel()
		if not 1 <= coef.size <= self.nmoments:
			raise ValueError(f"{coef.size} coefficients for {self.nmoments} moments")
		quad = np.zeros(self.nprobes)
		stage = np.zeros(4) if return_stage else None
		check(_capi.lib().slq_plan_moment_sum(self._h, int(coef.size), ptr(coef), ptr(quad), ptr(stage)))
		return (quad, stage) if return_stage else quad


def _rule_args(rule, endpoint) -> tuple:
	"""(rule id, endpoint) of `quadrature_at`, checked before any device work."""
	if rule not in RULE_IDS:
		raise ValueError(f"unknown quadrature rule '{rule}' (one of {', '.join(RULE_IDS)})")
	if rule == "radau":
		if endpoint is None:
			raise ValueError("rule='radau' needs endpoint=a with a <= lambda_min(A)")
		endpoint = float(endpoint)
		if not np.isfinite(endpoint):
			raise ValueError(f"endpoint must be finite, got {endpoint!r}")
	return RULE_IDS[rule], (0.0 if rule == "gauss" or endpoint is None else float(endpoint))


def _adaptive_args(deg_max, stages, deg_rtol, endpoint=None, deg_step=None, first=None) -> tuple:
	"""Checks the arguments of the adaptive-degree drivers before any device work; returns (deg_max, stages, deg_rtol,
	endpoint). stages=None: first (default: the step), first + step, ... up to deg_max, with deg_max appended if it is
	not the last."""
	if isinstance(deg_max, bool) or not isinstance(deg_max, (int, np.integer)) or deg_max < 1:
		raise ValueError(f"deg_max must be an integer >= 1, got {deg_max!r}")
	deg_max = int(deg_max)
	if deg_rtol is None:
		raise ValueError("an adaptive degree needs deg_rtol (it has no default)")
	deg_rtol = float(deg_rtol)
	if not (np.isfinite(deg_rtol) and deg_rtol > 0.0):
		raise ValueError(f"deg_rtol must be > 0, got {deg_rtol!r}")
	if endpoint is not None:
		endpoint = float(endpoint)
		if not np.isfinite(endpoint):
			raise ValueError(f"endpoint must be finite, got {endpoint!r}")
	if stages is None:
		step = DEG_STEP if deg_step is None else deg_step
		if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or step < 1:
			raise ValueError(f"deg_step must be an integer >= 1, got {step!r}")
		first = int(step) if first is None else int(first)
		if not 1 <= first <= deg_max:
			raise ValueError(f"the first stage {first} lies outside [1, deg_max = {deg_max}]")
		stages = list(range(first, deg_max + 1, int(step)))
		if stages[-1] != deg_max:
			stages.append(deg_max)
	else:
		if deg_step is not None:
			raise ValueError("give stages or deg_step, not both")
		try:
			given = list(stages)
		except TypeError:
			raise ValueError("stages must be a sequence of integers") from None
		if not given or any(isinstance(m, bool) or not isinstance(m, (int, np.integer)) for m in given):
			raise ValueError(f"stages must be a non-empty sequence of integers, got {stages!r}")
		stages = [int(m) for m in given]
		if any(m < 1 or m > deg_max for m in stages):
			raise ValueError(f"every stage must lie in [1, deg_max = {deg_max}], got {stages}")
		if any(b <= a for a, b in zip(stages[:-1], stages[1:])):
			raise ValueError(f"stages must be strictly increasing, got {stages}")
	return deg_max, stages, deg_rtol, endpoint


def quad_adaptive(
	op: DeviceOperator, X, deg_max: int, orth: int = 0, fun="identity", stages=None, deg_rtol: Optional[float] = None,
	endpoint: Optional[float] = None, rtol: float = 1e-8, nprobes: Optional[int] = None, deg_step: Optional[int] = None,
	plan: Optional[LanczosPlan] = None, **fun_kwargs,
):  # fmt: skip
	"""Lanczos quadrature with the degree chosen by the run itself: a resumable run of capacity `deg_max`, stopped
	after the first stage that meets the rule below. X: the probes (n x P), or (pdf, seed, probe_offset) to draw
	`nprobes` of them on the device. Returns (quad, deg_used, history).

	Stopping rule, from four doubles per stage reduced on the device (S_k = the sum of the Gauss values of stage k):
	without `endpoint`, the first stage k >= 1 with |S_k - S_{k-1}| <= deg_rtol |S_k|; with `endpoint` (a lower bound of
	the spectrum), the first stage with sum_i |radau_i - gauss_i| <= deg_rtol |S_k| - the width of the Gauss / Gauss-Radau
	bracket, an error bar of the quadrature for f whose derivatives keep one sign. If no stage meets it the run ends at
	deg_max. quad: the Gauss values at the stopping stage - what a fixed deg = deg_used, orth = min(orth, deg_used) run
	returns -; with `endpoint` an (P, 2) array, the Radau values beside them. history: [(m, stage)] for every stage
	visited, stage = {sum, sum of squares, sum |quad - gauss|, nprobes} of the Gauss values, with `endpoint` a (2, 4)
	array whose second row holds the same of the Radau values."""
	deg_max, stages, deg_rtol, endpoint = _adaptive_args(deg_max, stages, deg_rtol, endpoint, deg_step)
	fid, _ = fun_spec(fun, **fun_kwargs)
	if fid is None:
		raise ValueError("quad_adaptive takes built-in function names (the stage statistics are reduced on the device)")
	dev = isinstance(X, tuple)
	if dev:
		if len(X) != 3 or X[0] not in _capi.PDF_IDS:
			raise ValueError("device-drawn probes are given as (pdf, seed, probe_offset)")
		if nprobes is None or int(nprobes) < 1:
			raise ValueError("device-drawn probes need nprobes >= 1")
	else:
		X = np.asarray(X)
		X = X.reshape(-1, 1) if X.ndim == 1 else X
		if X.shape[0] != op.shape[0]:
			raise ValueError(f"X has {X.shape[0]} rows, the operator has {op.shape[0]}")
		nprobes = X.shape[1]
	own = plan is None
	if own:
		plan = LanczosPlan(op, int(nprobes), deg_max, orth)
	try:
		if plan.deg < stages[-1]:
			stages = [m for m in stages if m < plan.deg] + [plan.deg]  # (deg_max beyond n: the plan's capacity is n)
		if dev:
			plan.generate_probes(X[0], seed=int(X[1]), probe_offset=int(X[2]))
		else:
			plan.set_probes(X)
		history, s_prev, used = [], None, stages[-1]
		for k, m in enumerate(stages):
			plan.run(rtol, upto=m)
			_, st = plan.quadrature_at(m, fun, return_stage=True, **fun_kwargs)
			s_k = st[0]
			if endpoint is not None:
				_, sr = plan.quadrature_at(m, fun, rule="radau", endpoint=endpoint, return_stage=True, **fun_kwargs)
				history.append((m, np.stack([st, sr])))
				met = sr[2] <= deg_rtol * abs(s_k)
			else:
				history.append((m, st))
				met = k >= 1 and abs(s_k - s_prev) <= deg_rtol * abs(s_k)
			s_prev = s_k
			if met:
				used = m
				break
		quad = plan.quadrature_at(used, fun, **fun_kwargs)
		if endpoint is not None:
			quad = np.stack([quad, plan.quadrature_at(used, fun, rule="radau", endpoint=endpoint, **fun_kwargs)], axis=1)
	finally:
		if own:
			plan.close()
	return quad, used, history


def quad_batch(
	op: DeviceOperator, X: Optional[np.ndarray], deg: int, orth: int = 0, fun="identity", rtol: float = 1e-8,
	nprobes: Optional[int] = None, pdf: str = "rademacher", seed: int = 0, probe_offset: int = 0,
	return_rule: bool = False, **fun_kwargs,
):  # fmt: skip
	"""One call for P probes (C-ABI slq_quad_batch): the batched form of the reference's per-probe
	Python loop (src/primate/operators.py:145-150)."""
	fid, params = fun_spec(fun, **fun_kwargs)
	assert fid is not None, "quad_batch takes built-in function names; use LanczosPlan.quadrature for callables"
	n = op.shape[0]
	deg_eff = min(int(deg), n)
	if X is not None:
		X = np.asarray(X)
		X = X.reshape(-1, 1) if X.ndim == 1 else X
		X = np.asfortranarray(X, dtype=op.dtype)
		if X.shape[0] != n:
			raise ValueError(f"X has {X.shape[0]} rows, the operator has {n}")
		nprobes = X.shape[1]
	quad = np.zeros(nprobes)
	nodes = np.zeros((nprobes, deg_eff)) if return_rule else None
	weights = np.zeros((nprobes, deg_eff)) if return_rule else None
	rc = _capi.lib().slq_quad_batch(
		op.ctx._h, op._h, ptr(X), n, _capi.PDF_IDS[pdf], int(seed), int(probe_offset), int(nprobes), int(deg),
		float(rtol), int(orth), fid, ptr(params), ptr(quad), ptr(nodes), ptr(weights),
	)  # fmt: skip
	if rc == _capi.SLQ_ECALLBACK and getattr(op, "error", None) is not None:
		raise op.error
	check(rc)
	return (quad, nodes, weights) if return_rule else quad


def fun_action_batch(op: DeviceOperator, X: np.ndarray, deg: int, orth: int = 0, fun="identity", rtol: float = 1e-8, basis: str = "keep",
					 return_basis: bool = False, **fun_kwargs) -> np.ndarray:  # fmt: skip
	"""Y = f(A) X for all columns of X in one call (C-ABI slq_fAv_batch_mode): the batched form of
	`MatrixFunction._matvec` (src/primate/operators.py:102-124). basis: "keep" (the full basis of every column, batches sized
	to the free memory), "recompute" (two-pass plans: a footprint independent of deg, twice the runs) or "auto" (the kept
	basis when all columns fit at once, else recompute). With return_basis also the kind taken."""
	basis = _basis_arg(False, basis, auto=True)
	if basis is None:
		raise ValueError("basis must be 'keep', 'recompute' or 'auto'")
	fid, params = fun_spec(fun, **fun_kwargs)
	assert fid is not None, "fun_action_batch takes built-in function names"
	X = np.asarray(X)
	X = np.asfortranarray(X.reshape(-1, 1) if X.ndim == 1 else X, dtype=op.dtype)
	n = op.shape[0]
	if X.shape[0] != n:
		raise ValueError(f"X has {X.shape[0]} rows, the operator has {n}")
	Y = np.zeros((n, X.shape[1]), dtype=op.dtype, order="F")
	used = C.c_int(0)
	rc = _capi.lib().slq_fAv_batch_mode(op.ctx._h, op._h, ptr(X), n, X.shape[1], int(deg), float(rtol), int(orth), fid, ptr(params),
										{"auto": 0, "keep": 1, "recompute": 2}[basis], ptr(Y), n, C.byref(used))  # fmt: skip
	if rc == _capi.SLQ_ECALLBACK and getattr(op, "error", None) is not None:
		raise op.error
	check(rc)
	return (Y, {1: "keep", 2: "recompute"}[used.value]) if return_basis else Y


def quadrature_batch(d: np.ndarray, e: np.ndarray, fun=None, ctx: Optional[Context] = None, **fun_kwargs):
	"""Gauss quadrature rules of a batch of Jacobi matrices on the device (slq_quadrature_batch).
	d, e: (nb, deg) with e[:, 0] ignored. Returns (nodes, weights) or, with `fun`, (quad, nodes, weights)."""
	ctx = ctx or default_context()
	d = np.ascontiguousarray(np.atleast_2d(d), dtype=np.float64)
	e = np.ascontiguousarray(np.atleast_2d(e), dtype=np.float64)
	assert d.shape == e.shape
	nb, deg = d.shape
	nodes, weights = np.zeros((nb, deg)), np.zeros((nb, deg))
	fid, params = (_capi.FUN_NONE, np.zeros(4)) if fun is None else fun_spec(fun, **fun_kwargs)
	quad = np.zeros(nb)
	check(_capi.lib().slq_quadrature_batch(ctx._h, nb, deg, ptr(d), ptr(e), fid, ptr(params), ptr(quad), ptr(nodes), ptr(weights)))
	return (nodes, weights) if fun is None else (quad, nodes, weights)


def quadrature_radau_batch(d: np.ndarray, e: np.ndarray, residual, endpoint: float, fun=None, ctx: Optional[Context] = None, **fun_kwargs):
	"""Gauss-Radau rules with a node at `endpoint` of a batch of m x m Jacobi matrices on the device
	(slq_quadrature_radau_batch). d, e: (nb, m) with e[:, 0] ignored; residual: beta_m per matrix, the coupling to the
	border. Returns (nodes, weights), each (nb, m + 1), or with `fun` (quad, nodes, weights)."""
	if endpoint is None or not np.isfinite(float(endpoint)):
		raise ValueError("the Gauss-Radau rule needs a finite endpoint")
	if residual is None:
		raise ValueError("the Gauss-Radau rule needs residual = beta_m, the norm of the Lanczos residual after m steps")
	d = np.ascontiguousarray(np.atleast_2d(d), dtype=np.float64)
	e = np.ascontiguousarray(np.atleast_2d(e), dtype=np.float64)
	if d.shape != e.shape:
		raise ValueError("d and e must have the same shape")
	nb, m = d.shape
	residual = np.ascontiguousarray(np.broadcast_to(np.asarray(residual, dtype=np.float64).ravel(), (nb,)))
	ctx = ctx or default_context()
	nodes, weights = np.zeros((nb, m + 1)), np.zeros((nb, m + 1))
	fid, params = (_capi.FUN_NONE, np.zeros(4)) if fun is None else fun_spec(fun, **fun_kwargs)
	quad = np.zeros(nb)
	check(_capi.lib().slq_quadrature_radau_batch(ctx._h, nb, m, ptr(d), ptr(e), ptr(residual), float(endpoint), fid, ptr(params), ptr(quad),
												 ptr(nodes), ptr(weights)))  # fmt: skip
	return (nodes, weights) if fun is None else (quad, nodes, weights)


def eigh_tridiag_batch(d: np.ndarray, e: np.ndarray, vectors: bool = True, ctx: Optional[Context] = None):
	"""Eigenvalues (ascending) and, optionally, eigenvectors (columns) of a batch of symmetric tridiagonals on
	the device (slq_eigh_tridiag_batch). d, e: (nb, deg), e[:, 0] ignored."""
	ctx = ctx or default_context()
	d = np.ascontiguousarray(np.atleast_2d(d), dtype=np.float64)
	e = np.ascontiguousarray(np.atleast_2d(e), dtype=np.float64)
	assert d.shape == e.shape
	nb, deg = d.shape
	w = np.zeros((nb, deg))
	Z = np.zeros((nb, deg, deg)) if vectors else None
	check(_capi.lib().slq_eigh_tridiag_batch(ctx._h, nb, deg, ptr(d), ptr(e), ptr(w), ptr(Z)))
	return (w, Z) if vectors else w


def fttr_batch(theta: np.ndarray, alpha: np.ndarray, beta: np.ndarray, k: Optional[int] = None, ctx: Optional[Context] = None) -> np.ndarray:
	"""FTTR quadrature weights on the device (slq_fttr_batch); rows are independent rules."""
	ctx = ctx or default_context()
	theta = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
	alpha = np.ascontiguousarray(np.atleast_2d(alpha), dtype=np.float64)
	beta = np.ascontiguousarray(np.atleast_2d(beta), dtype=np.float64)
	nb, kk = theta.shape
	k = kk if k is None else int(k)
	assert alpha.shape == beta.shape and alpha.shape[0] == nb and k <= kk
	w = np.zeros((nb, k))
	check(_capi.lib().slq_fttr_batch(ctx._h, nb, alpha.shape[1], k, ptr(np.ascontiguousarray(theta[:, :k])), ptr(alpha), ptr(beta), ptr(w)))
	return w


class DiagAccumulator(_Handle):
	"""Device-resident numer / denom / running-mean accumulators of the diagonal estimator."""

	_destroy = "slq_diag_destroy"

	def __init__(self, n: int, ctx: Optional[Context] = None):
		self.ctx = ctx or default_context()
		self.n = int(n)
		h = C.c_void_p()
		check(_capi.lib().slq_diag_create(self.ctx._h, self.n, C.byref(h)))
		self._h = h

	def update(self, plan: LanczosPlan, fun="identity", **fun_kwargs):
		fid, params = fun_spec(fun, **fun_kwargs)
		assert fid is not None, "the device diagonal path takes built-in function names"
		check(_capi.lib().slq_diag_update(self._h, plan._h, fid, ptr(params)))

	def get(self) -> tuple:
		"""(numer, denom, running_mean, count)."""
		nu, de, rm = np.zeros(self.n), np.zeros(self.n), np.zeros(self.n)
		cnt = C.c_int64()
		check(_capi.lib().slq_diag_get(self._h, ptr(nu), ptr(de), ptr(rm), C.byref(cnt)))
		return nu, de, rm, cnt.value


class DensityAccumulator(_Handle):
	"""Device-resident (count, mean, M2) of a spectral density estimate over a fixed grid (slq_density_*): every
	`update(plan)` folds the per-probe values ||v||^2 sum_k tau_k K(x_g, theta_k) of a completed run, in probe order.
	kind: "gaussian" | "lorentzian" (G points, bandwidth bw > 0), "histogram" (G bins: G + 1 edges), "cdf"
	(G thresholds) or "chebyshev" (G points strictly inside the bounds of the runs folded in; bw ignored): the density of
	the kernel polynomial method from the moments of a ChebyshevPlan."""

	_destroy = "slq_density_destroy"

	def __init__(self, kind: str, grid: np.ndarray, bw: float = 0.0, ctx: Optional[Context] = None):
		if kind not in _capi.DENSITY_KINDS:
			raise ValueError(f"unknown density kernel '{kind}' (one of {', '.join(_capi.DENSITY_KINDS)})")
		self.ctx = ctx or default_context()
		self.kind = kind
		self.grid = np.ascontiguousarray(grid, dtype=np.float64).ravel()
		self.ngrid = self.grid.size - (1 if kind == "histogram" else 0)
		h = C.c_void_p()
		check(_capi.lib().slq_density_create(self.ctx._h, _capi.DENSITY_KINDS[kind], int(self.ngrid), ptr(self.grid), float(bw), C.byref(h)))
		self._h = h

	def update(self, plan: LanczosPlan, damping=None, nweights: Optional[int] = None):
		"""Asynchronous on the context stream; the QL of the run is shared with `plan.quadrature`.
		kind "chebyshev": `plan` is a ChebyshevPlan; the first `nweights` moments (default: all, or len(damping)) are folded
		with the damping factors `damping` (None: all ones; chebyshev.damping_factors) - slq_density_update_moments."""
		if self.kind == "chebyshev":
			if not isinstance(plan, ChebyshevPlan):
				raise ValueError("a 'chebyshev' density is updated from a ChebyshevPlan")
			g = None if damping is None else np.ascontiguousarray(damping, dtype=np.float64).ravel()
			k = int(nweights) if nweights is not None else (plan.nmoments if g is None else g.size)
			if g is not None and g.size < k:
				raise ValueError(f"{g.size} damping factors for {k} moments")
			check(_capi.lib().slq_density_update_moments(self._h, plan._h, k, ptr(g)))
			return
		if damping is not None or nweights is not None:
			raise ValueError("damping and nweights belong to the 'chebyshev' kind")
		check(_capi.lib().slq_density_update(self._h, plan._h))

	def get(self) -> tuple:
		"""(mean, M2, outside, count): mean and M2 per grid point, outside = the mean node mass (below, above) the grid."""
		mean, m2, out = np.zeros(self.ngrid), np.zeros(self.ngrid), np.zeros(2)
		cnt = C.c_int64()
		check(_capi.lib().slq_density_get(self._h, ptr(mean), ptr(m2), ptr(out), C.byref(cnt)))
		return mean, m2, out, cnt.value


def _is_torch_csr(A) -> bool:
	return type(A).__module__.split(".")[0] == "torch" and str(getattr(A, "layout", "")) == "torch.sparse_csr"


def sddmm_schedule(indptr) -> dict:
	"""The work items an SddmmAccumulator over this row-pointer array launches, one wave each (slq_debug_sddmm_schedule: no
	device is touched): row0, nrows, kind (0: one lane per row, 1: one long row over the lanes), e0, e1 (the stored nonzeros
	[e0, e1) the item owns), and grid, nlong, long_row, waves."""
	rp = np.ascontiguousarray(indptr, dtype=np.int32).ravel()
	n = rp.size - 1
	L = _capi.lib()
	nitems, info = C.c_int64(), np.zeros(4, dtype=np.int64)
	check(L.slq_debug_sddmm_schedule(n, ptr(rp), None, None, None, None, None, 0, C.byref(nitems), ptr(info)))
	k = nitems.value
	row0, nrows, kind = (np.zeros(k, dtype=np.int32) for _ in range(3))
	e0, e1 = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
	check(L.slq_debug_sddmm_schedule(n, ptr(rp), ptr(row0), ptr(nrows), ptr(kind), ptr(e0), ptr(e1), k, C.byref(nitems), ptr(info)))
	return dict(row0=row0, nrows=nrows, kind=kind, e0=e0, e1=e1, grid=int(info[0]), nlong=int(info[1]), long_row=int(info[2]), waves=int(info[3]))


class SddmmAccumulator(_Handle):
	"""Device-resident values on a CSR pattern (slq_sddmm_*): every `update` folds alpha * sum_j W[row(e), w0 + j] Z[col(e), z0 + j]
	into the value of every stored nonzero e. pattern: a SciPy sparse matrix (its `indptr` / `indices` as given - not sorted, not
	deduplicated; any other format is converted to CSR first) or a torch sparse-CSR tensor on the context's GPU. Only the pattern
	is read; the values come out aligned with `pattern.data` / `pattern.values()`, entry for entry."""

	_destroy = "slq_sddmm_destroy"

	def __init__(self, pattern, ctx: Optional[Context] = None):
		import scipy.sparse as sp

		if not (_is_torch_csr(pattern) or sp.issparse(pattern)):
			raise ValueError("pattern must be a SciPy sparse matrix or a torch sparse-CSR tensor on the GPU")
		self.ctx = ctx or default_context()
		L = _capi.lib()
		h = C.c_void_p()
		if _is_torch_csr(pattern):
			import torch

			if not pattern.is_cuda:
				raise ValueError("a torch sparse-CSR pattern must live on the GPU (use scipy.sparse for host matrices)")
			if pattern.device.index != self.ctx.device:
				raise ValueError(f"the pattern is on {pattern.device}, the context on GPU {self.ctx.device}")
			if pattern.shape[0] != pattern.shape[1]:
				raise ValueError(f"the pattern must be square, got {tuple(pattern.shape)}")
			crow = pattern.crow_indices().to(torch.int32).contiguous()
			col = pattern.col_indices().to(torch.int32).contiguous()
			torch.cuda.synchronize(pattern.device)
			self.n, self.nnz = int(pattern.shape[0]), int(col.numel())
			check(L.slq_sddmm_create_device(self.ctx._h, self.n, self.nnz, C.c_void_p(crow.data_ptr()), C.c_void_p(col.data_ptr()), C.byref(h)))
		elif sp.issparse(pattern):
			M = pattern if pattern.format == "csr" else sp.csr_matrix(pattern)
			if M.shape[0] != M.shape[1]:
				raise ValueError(f"the pattern must be square, got {M.shape}")
			rowptr = np.ascontiguousarray(M.indptr, dtype=np.int32)
			colind = np.ascontiguousarray(M.indices, dtype=np.int32)
			self.n, self.nnz = int(M.shape[0]), int(colind.size)
			check(L.slq_sddmm_create(self.ctx._h, self.n, self.nnz, ptr(rowptr), ptr(colind), C.byref(h)))
		self._h = h

	def update(self, W: "DeviceMatrix", w0: int, Z: "DeviceMatrix", z0: int, m: int, alpha: float = 1.0, beta: float = 1.0, symmetric: bool = False):
		"""vals = beta * vals + alpha * (the sampled product over columns [w0, w0 + m) of W and [z0, z0 + m) of Z); symmetric: its
		symmetric part. Asynchronous on the context stream."""
		check(_capi.lib().slq_sddmm_update(self._h, W._h, int(w0), Z._h, int(z0), int(m), float(alpha), float(beta), 1 if symmetric else 0))

	def get(self) -> tuple:
		"""(vals, count): the nnz values in the pattern's order, the columns folded in."""
		vals = np.zeros(self.nnz)
		cnt = C.c_int64()
		check(_capi.lib().slq_sddmm_get(self._h, ptr(vals) if self.nnz else None, C.byref(cnt)))
		return vals, cnt.value

	def cuda_array(self):
		"""The values as a flat object with `__cuda_array_interface__` (zero-copy; it keeps the accumulator alive)."""
		p = C.c_void_p()
		check(_capi.lib().slq_sddmm_ptr(self._h, C.byref(p)))
		return _CudaArrayView(p.value, self.nnz, self)

	def reset(self):
		check(_capi.lib().slq_sddmm_reset(self._h))


def kernel_grad_schedule(n: int, m: int, num_cus: int = 256) -> dict:
	"""The schedule of one KernelGradAccumulator.update for n points and m columns, as the library cuts it (slq_debug_kernel_grad_schedule;
	host arithmetic, no device): rows per block, row blocks, columns per chunk, chunks (launches), slabs and their bounds."""
	out = (C.c_int64 * 22)()
	check(_capi.lib().slq_debug_kernel_grad_schedule(int(n), int(m), int(num_cus), out, 22))
	v = list(out)
	return dict(rows=v[0], nrb=v[1], chunk_cols=v[2], chunks=v[3], slabs=v[4], begin=v[5 : 5 + v[4] + 1], rest=v[5 + v[4] + 1 :])


class KernelGradAccumulator(_Handle):
	"""Device-resident hyperparameter gradients of a kernel operator (slq_kernel_grad_*): every `update` folds
	alpha * sum_c Z_c^T (dA/dtheta) W_c, for theta = the d lengthscales, the outputscale and the noise, into d + 2 values. op: a
	DeviceOperator of kind "kernel" in fp64. The accumulator keeps `op` alive, as a plan does, and reads its parameters as they are at
	each update: `set_kernel_parameters` between two updates is honoured by the second, and values accumulated across such a change
	mix two operators."""

	_destroy = "slq_kernel_grad_destroy"

	def __init__(self, op: DeviceOperator):
		if getattr(op, "kind", None) != "kernel":
			raise ValueError(f"KernelGradAccumulator needs a kernel operator, not kind '{getattr(op, 'kind', None)}'")
		if np.dtype(op.dtype) != np.float64:
			raise ValueError(f"KernelGradAccumulator is fp64 only (the device matrices are fp64): the operator is {np.dtype(op.dtype)}")
		self.op, self.ctx = op, op.ctx
		self.n, self.d = int(op.shape[0]), int(op.nnz // op.shape[0])
		h = C.c_void_p()
		check(_capi.lib().slq_kernel_grad_create(self.ctx._h, op._h, C.byref(h)))
		self._h = h

	def update(self, Z: "DeviceMatrix", z0: int, W: "DeviceMatrix", w0: int, m: int, alpha: float = 1.0, beta: float = 1.0):
		"""vals = beta * vals + alpha * (the d + 2 sums over columns [z0, z0 + m) of Z and [w0, w0 + m) of W). Asynchronous on the
		context stream."""
		check(_capi.lib().slq_kernel_grad_update(self._h, Z._h, int(z0), W._h, int(w0), int(m), float(alpha), float(beta)))

	def get(self) -> tuple:
		"""(vals, count): [0, d) the lengthscale gradients per dimension, [d] the outputscale's, [d + 1] the noise's; the columns
		folded in."""
		vals = np.zeros(self.d + 2)
		cnt = C.c_int64()
		check(_capi.lib().slq_kernel_grad_get(self._h, ptr(vals), self.d + 2, C.byref(cnt)))
		return vals, cnt.value

	def reset(self):
		check(_capi.lib().slq_kernel_grad_reset(self._h))


def kernel_cross_schedule(nrows: int, nsum: int, b: int, num_cus: int = 256) -> dict:
	"""The schedule of one cross-covariance product with `nrows` output rows, `nsum` summed points and `b` columns, as the library
	cuts it (slq_debug_kernel_cross_schedule; host arithmetic, no device): rows per block, row blocks, 16-column tiles per workgroup,
	256-column chunks, slabs of the summed points, tiles of 16 points per slab and the slabs' bounds."""
	out = (C.c_int64 * 71)()
	check(_capi.lib().slq_debug_kernel_cross_schedule(int(nrows), int(nsum), int(b), int(num_cus), out, 71))
	v = list(out)
	return dict(rows=v[0], nrb=v[1], col_blocks=v[2], chunks=v[3], slabs=v[4], tiles_per_slab=v[5], begin=v[6 : 6 + v[4] + 1], rest=v[6 + v[4] + 1 :])


class KernelCross(_Handle):
	"""The cross-covariance C = s phi(r2(X*, X)) between `Xnew` (m x d) and the points of a kernel operator, never formed
	(slq_kernel_cross_*): `matmat(W)` is C W (m x b), `matmat(U, trans=True)` is C^T U (n x b). z* is taken with
	the operator's own centre and its lengthscales of now; no diagonal rule, no noise term. op: a DeviceOperator of kind "kernel"; the
	object takes its dtype and keeps it alive, as a plan does. `Xnew`: a NumPy array, or a torch tensor on the context's GPU.
	`set_kernel_parameters` on the operator is honoured by the next product (the library re-derives z* on the stream)."""

	_destroy = "slq_kernel_cross_destroy"

	def __init__(self, op: DeviceOperator, Xnew):
		if getattr(op, "kind", None) != "kernel":
			raise ValueError(f"KernelCross needs a kernel operator, not kind '{getattr(op, 'kind', None)}'")
		self.op, self.ctx = op, op.ctx
		self.dtype = np.dtype(op.dtype)
		self.n, self.d = int(op.shape[0]), int(op.nnz // op.shape[0])
		L = _capi.lib()
		h = C.c_void_p()
		if type(Xnew).__module__.split(".")[0] == "torch" and Xnew.is_cuda:
			import torch

			if Xnew.device.index != self.ctx.device:
				raise ValueError(f"the new points are on {Xnew.device}, the context on GPU {self.ctx.device}")
			Xt = Xnew.detach()
			Xt = Xt.reshape(-1, 1) if Xt.ndim == 1 else Xt
			if Xt.ndim != 2 or Xt.shape[1] != self.d or Xt.shape[0] < 1:
				raise ValueError(f"the new points must be an (m, {self.d}) array with m >= 1, got shape {tuple(Xt.shape)}")
			Xt = Xt.to(torch.float64 if self.dtype == np.float64 else torch.float32).contiguous()
			torch.cuda.synchronize(Xt.device)
			self.m = int(Xt.shape[0])
			check(L.slq_kernel_cross_create_device(self.ctx._h, op._h, self.m, C.c_void_p(Xt.data_ptr()), self.d, C.byref(h)))
		else:
			if type(Xnew).__module__.split(".")[0] == "torch":
				Xnew = Xnew.detach().cpu().numpy()
			X = np.asarray(Xnew)
			X = X.reshape(-1, 1) if X.ndim == 1 else X
			if X.ndim != 2 or X.shape[1] != self.d or X.shape[0] < 1:
				raise ValueError(f"the new points must be an (m, {self.d}) array with m >= 1, got shape {X.shape}")
			X = np.ascontiguousarray(X, dtype=self.dtype)
			self.m = int(X.shape[0])
			check(L.slq_kernel_cross_create(self.ctx._h, op._h, self.m, ptr(X), self.d, C.byref(h)))
		self.shape = (self.m, self.n)
		self._h = h

	def matmat(self, X: np.ndarray, trans: bool = False) -> np.ndarray:
		"""C X (trans=False: X is n x b) or C^T X (X is m x b) for a host array, in the operator's dtype."""
		rin, rout = (self.m, self.n) if trans else (self.n, self.m)
		X = np.asarray(X)
		X = X.reshape(-1, 1) if X.ndim == 1 else X
		if X.ndim != 2 or X.shape[0] != rin or X.shape[1] < 1:
			raise ValueError(f"dimension mismatch: the product with trans={bool(trans)} reads {rin} rows, the operand has shape {X.shape}")
		X = np.asfortranarray(X, dtype=self.dtype)
		Y = np.empty((rout, X.shape[1]), dtype=self.dtype, order="F")
		check(_capi.lib().slq_kernel_cross_matmat(self._h, int(bool(trans)), ptr(X), rin, ptr(Y), rout, X.shape[1]))
		return Y

	def matmat_dmat(self, IN: "DeviceMatrix", i0: int, OUT: "DeviceMatrix", o0: int, b: int, trans: bool = False):
		"""OUT[:, o0:o0+b] = C IN[:, i0:i0+b] (or C^T ...) between DeviceMatrix columns: fp64 only, asynchronous on the context stream."""
		check(_capi.lib().slq_kernel_cross_dmat(self._h, int(bool(trans)), IN._h, int(i0), OUT._h, int(o0), int(b)))

	def scaled_points(self) -> tuple:
		"""(z*, |z*|^2): m x d and m, as the device holds them (slq_debug_kernel_cross_points), in the operator's dtype. Sets
		`padding_is_zero`: whether everything beyond d and m in the device arrays is 0, as the kernel relies on."""
		dpad, mpad = (self.d + 3) // 4 * 4, (self.m + 15) // 16 * 16
		zt = np.empty((dpad, mpad), dtype=self.dtype)
		nrm = np.empty(mpad, dtype=self.dtype)
		check(_capi.lib().slq_debug_kernel_cross_points(self._h, ptr(zt), ptr(nrm)))
		self.padding_is_zero = bool(not zt[self.d :].any() and not zt[:, self.m :].any() and not nrm[self.m :].any())
		return np.ascontiguousarray(zt[: self.d, : self.m].T), nrm[: self.m].copy()


def kernel_feature_schedule(nrows: int, num_features: int, b: int, num_cus: int = 256, dtype=np.float64) -> dict:
	"""The schedule of one feature product with `nrows` row points, `num_features` frequencies and `b` columns, as the library cuts it
	(slq_debug_kernel_feature_schedule; host arithmetic, no device), in the form of `kernel_cross_schedule`: the column chunks are 128
	wide in float64 and 256 in float32."""
	out = (C.c_int64 * 71)()
	check(_capi.lib().slq_debug_kernel_feature_schedule(int(nrows), int(num_features), int(b), int(num_cus), int(np.dtype(dtype) == np.float64), out, 71))
	v = list(out)
	return dict(rows=v[0], nrb=v[1], col_blocks=v[2], chunks=v[3], slabs=v[4], tiles_per_slab=v[5], begin=v[6 : 6 + v[4] + 1], rest=v[6 + v[4] + 1 :])


def kernel_feature_adjoint_schedule(num_features: int, nrows: int, b: int, num_cus: int = 256, dtype=np.float64) -> dict:
	"""The schedule of one adjoint feature product Phi^T U with `num_features` frequencies (the row blocks), `nrows` row points (the
	slabs) and `b` columns, as the library cuts it (slq_debug_kernel_feature_adjoint_schedule; host arithmetic, no device), in the form
	of `kernel_feature_schedule`: the column chunks are 128 wide in float64 and 256 in float32."""
	out = (C.c_int64 * 71)()
	check(_capi.lib().slq_debug_kernel_feature_adjoint_schedule(int(num_features), int(nrows), int(b), int(num_cus), int(np.dtype(dtype) == np.float64), out, 71))
	v = list(out)
	return dict(rows=v[0], nrb=v[1], col_blocks=v[2], chunks=v[3], slabs=v[4], tiles_per_slab=v[5], begin=v[6 : 6 + v[4] + 1], rest=v[6 + v[4] + 1 :])


GRAM_CHUNK = 128  # identity columns of one forward + adjoint pair of KernelFeatureMap.gram: the fp64 column chunk of both kernels


class KernelFeatureMap(_Handle):
	"""Random Fourier features of a kernel operator's profile on the GPU, never formed (slq_kernel_feature_*):
	`matmat(W)` is Phi W with Phi(z) = sqrt(s / F2) [cos(Omega z) | sin(Omega z)] at the operator's scaled points - or, with
	`rows=` a KernelCross of the same operator, at its new points - for W of 2 F2 rows. `omega`: F2 x d, rounded once to the operator's
	dtype (the map is defined on the rounded values, `self.omega`). op: a DeviceOperator of kind "kernel"; the object takes its dtype
	and keeps it alive, as a plan does. `set_kernel_parameters` on the operator is honoured by the next product."""

	_destroy = "slq_kernel_feature_destroy"

	def __init__(self, op: DeviceOperator, omega):
		if getattr(op, "kind", None) != "kernel":
			raise ValueError(f"KernelFeatureMap needs a kernel operator, not kind '{getattr(op, 'kind', None)}'")
		self.op, self.ctx = op, op.ctx
		self.dtype = np.dtype(op.dtype)
		self.n, self.d = int(op.shape[0]), int(op.nnz // op.shape[0])
		om = np.asarray(omega)
		om = om.reshape(-1, 1) if om.ndim == 1 else om
		if om.ndim != 2 or om.shape[1] != self.d or om.shape[0] < 1:
			raise ValueError(f"the frequencies must be an (F2, {self.d}) array with F2 >= 1, got shape {om.shape}")
		self.omega = np.ascontiguousarray(om, dtype=self.dtype)
		self.num_features = int(self.omega.shape[0])
		h = C.c_void_p()
		check(_capi.lib().slq_kernel_feature_create(self.ctx._h, op._h, self.num_features, ptr(self.omega), self.d, C.byref(h)))
		self._h = h

	def _rows(self, rows) -> tuple:
		if rows is None:
			return None, self.n
		if not isinstance(rows, KernelCross):
			raise ValueError("rows must be None (the operator's points) or a KernelCross")
		return rows._h, rows.m

	def matmat(self, W: np.ndarray, rows: Optional["KernelCross"] = None) -> np.ndarray:
		"""Phi W for a host array W (2 F2 x b), in the operator's dtype: n x b, or m x b at the new points of `rows`."""
		rh, rout = self._rows(rows)
		W = np.asarray(W)
		W = W.reshape(-1, 1) if W.ndim == 1 else W
		if W.ndim != 2 or W.shape[0] != 2 * self.num_features or W.shape[1] < 1:
			raise ValueError(f"dimension mismatch: the product reads {2 * self.num_features} rows (2 F2), the operand has shape {W.shape}")
		W = np.asfortranarray(W, dtype=self.dtype)
		Y = np.empty((rout, W.shape[1]), dtype=self.dtype, order="F")
		check(_capi.lib().slq_kernel_feature_matmat(self._h, rh, ptr(W), W.shape[0], ptr(Y), rout, W.shape[1]))
		return Y

	def matmat_dmat(self, IN: "DeviceMatrix", i0: int, OUT: "DeviceMatrix", o0: int, b: int, rows: Optional["KernelCross"] = None):
		"""OUT[:, o0:o0+b] = Phi IN[:, i0:i0+b] between DeviceMatrix columns: fp64 only, asynchronous on the context stream."""
		rh, _ = self._rows(rows)
		check(_capi.lib().slq_kernel_feature_dmat(self._h, rh, IN._h, int(i0), OUT._h, int(o0), int(b)))

	def rmatmat(self, U: np.ndarray, rows: Optional["KernelCross"] = None) -> np.ndarray:
		"""Phi^T U for a host array U (n x b, or m x b with the new points of `rows`), in the operator's dtype: 2 F2 x b, the cosine rows
		first (slq_kernel_feature_rmatmat)."""
		rh, rin = self._rows(rows)
		U = np.asarray(U)
		U = U.reshape(-1, 1) if U.ndim == 1 else U
		if U.ndim != 2 or U.shape[0] != rin or U.shape[1] < 1:
			raise ValueError(f"dimension mismatch: the adjoint product reads {rin} rows, the operand has shape {U.shape}")
		U = np.asfortranarray(U, dtype=self.dtype)
		rout = 2 * self.num_features
		Z = np.empty((rout, U.shape[1]), dtype=self.dtype, order="F")
		check(_capi.lib().slq_kernel_feature_rmatmat(self._h, rh, ptr(U), U.shape[0], ptr(Z), rout, U.shape[1]))
		return Z

	def rmatmat_dmat(self, IN: "DeviceMatrix", i0: int, OUT: "DeviceMatrix", o0: int, b: int, rows: Optional["KernelCross"] = None):
		"""OUT[:, o0:o0+b] = Phi^T IN[:, i0:i0+b] between DeviceMatrix columns: fp64 only, asynchronous on the context stream."""
		rh, _ = self._rows(rows)
		check(_capi.lib().slq_kernel_feature_rdmat(self._h, rh, IN._h, int(i0), OUT._h, int(o0), int(b)))

	def gram(self, rows: Optional["KernelCross"] = None, chunk: int = GRAM_CHUNK) -> np.ndarray:
		"""Phi^T Phi (2 F2 x 2 F2, host float64) formed on the device without Phi: for each `chunk` of identity columns a forward product
		into an nrows x chunk scratch DeviceMatrix, the adjoint of that into 2 F2 x chunk, and that block read back. fp64 only. Returns
		the symmetrised (G + G^T) / 2; `gram_asymmetry` is the largest |G - G^T| seen."""
		if self.dtype != np.float64:
			raise ValueError(f"gram is fp64 only (the device matrices are fp64): the feature map is {self.dtype}")
		chunk = int(chunk)
		if chunk < 1:
			raise ValueError(f"chunk = {chunk} must be >= 1")
		_, nrows = self._rows(rows)
		m2 = 2 * self.num_features
		chunk = min(chunk, m2)
		G = np.empty((m2, m2))
		live = []
		try:
			Id = DeviceMatrix(m2, chunk, ctx=self.ctx)
			live.append(Id)
			T = DeviceMatrix(nrows, chunk, ctx=self.ctx)
			live.append(T)
			Zd = DeviceMatrix(m2, chunk, ctx=self.ctx)
			live.append(Zd)
			for c0 in range(0, m2, chunk):
				cb = min(chunk, m2 - c0)
				E = np.zeros((m2, cb))
				E[c0 + np.arange(cb), np.arange(cb)] = 1.0
				Id.set(0, E)
				self.matmat_dmat(Id, 0, T, 0, cb, rows=rows)
				self.rmatmat_dmat(T, 0, Zd, 0, cb, rows=rows)
				G[:, c0 : c0 + cb] = Zd.get(0, cb)
		finally:
			for obj in reversed(live):
				obj.close()
		self.gram_asymmetry = float(np.max(np.abs(G - G.T)))
		return 0.5 * (G + G.T)

	def frequencies(self) -> np.ndarray:
		"""Omega (F2 x d) as the device holds it (slq_debug_kernel_feature_frequencies), in the operator's dtype. Sets
		`padding_is_zero`: whether everything beyond d and F2 in the device array is 0, as the kernel relies on."""
		dpad, fpad = (self.d + 3) // 4 * 4, (self.num_features + 15) // 16 * 16
		omt = np.empty((dpad, fpad), dtype=self.dtype)
		check(_capi.lib().slq_debug_kernel_feature_frequencies(self._h, ptr(omt)))
		self.padding_is_zero = bool(not omt[self.d :].any() and not omt[:, self.num_features :].any())
		return np.ascontiguousarray(omt[: self.d, : self.num_features].T)


def kernel_pointgrad_schedule(nrows: int, nsum: int, num_cus: int = 256) -> dict:
	"""The schedule of one pass of a KernelPointGradAccumulator.update with `nrows` row points and `nsum` summed points, as the library
	cuts it (slq_debug_kernel_pointgrad_schedule; host arithmetic, no device): rows per block, row blocks, factor columns per launch,
	slabs of the summed points, tiles of 16 points per slab and the slabs' bounds."""
	out = (C.c_int64 * 70)()
	check(_capi.lib().slq_debug_kernel_pointgrad_schedule(int(nrows), int(nsum), int(num_cus), out, 70))
	v = list(out)
	return dict(rows=v[0], nrb=v[1], chunk_cols=v[2], slabs=v[3], tiles_per_slab=v[4], begin=v[5 : 5 + v[3] + 1], rest=v[5 + v[3] + 1 :])


class KernelPointGradAccumulator(_Handle):
	"""Device-resident gradients of a kernel operator with respect to the points (slq_kernel_pointgrad_*).
	On a DeviceOperator of kind "kernel" in fp64 (the training form) every `update` folds alpha * sum_c Z_c^T (dA/dx_ak) W_c into n x d
	values; on a KernelCross of such an operator (the cross form) alpha * d/dx*_ak sum_c U_c^T K(X*, X) W_c into m x d values, U on the
	new points and W on the training points. The accumulator keeps what it borrows alive - the operator, and the cross object - and
	reads the operator's parameters as they are at each update, as a KernelGradAccumulator does; a cross-form accumulator follows a
	`set_kernel_parameters` as a cross product does."""

	_destroy = "slq_kernel_pointgrad_destroy"

	def __init__(self, op_or_cross):
		cross = op_or_cross if isinstance(op_or_cross, KernelCross) else None
		op = cross.op if cross is not None else op_or_cross
		if getattr(op, "kind", None) != "kernel":
			raise ValueError(f"KernelPointGradAccumulator needs a kernel operator or a KernelCross, not kind '{getattr(op, 'kind', None)}'")
		if np.dtype(op.dtype) != np.float64:
			raise ValueError(f"KernelPointGradAccumulator is fp64 only (the device matrices are fp64): the operator is {np.dtype(op.dtype)}")
		self.op, self.cross, self.ctx = op, cross, op.ctx
		self.n, self.d = int(op.shape[0]), int(op.nnz // op.shape[0])
		self.rows = int(cross.m) if cross is not None else self.n
		h = C.c_void_p()
		if cross is not None:
			check(_capi.lib().slq_kernel_pointgrad_create_cross(self.ctx._h, cross._h, C.byref(h)))
		else:
			check(_capi.lib().slq_kernel_pointgrad_create(self.ctx._h, op._h, C.byref(h)))
		self._h = h

	def update(self, Z: "DeviceMatrix", z0: int, W: "DeviceMatrix", w0: int, m: int, alpha: float = 1.0, beta: float = 1.0):
		"""vals = beta * vals + alpha * (the rows x d sums over columns [z0, z0 + m) of Z - U, on the new points, in the cross form - and
		[w0, w0 + m) of W). Asynchronous on the context stream."""
		check(_capi.lib().slq_kernel_pointgrad_update(self._h, Z._h, int(z0), W._h, int(w0), int(m), float(alpha), float(beta)))

	def get(self) -> tuple:
		"""(vals, count): rows x d, shaped like the points; the columns folded in."""
		vals = np.zeros((self.rows, self.d))
		cnt = C.c_int64()
		check(_capi.lib().slq_kernel_pointgrad_get(self._h, ptr(vals), self.d, C.byref(cnt)))
		return vals, cnt.value

	def reset(self):
		check(_capi.lib().slq_kernel_pointgrad_reset(self._h))


class _CudaArrayView:
	"""Flat fp64 device array described by the CUDA array interface (v2); keeps its owner alive."""

	def __init__(self, dptr: int, count: int, owner, shape=None, dtype=np.float64, device: Optional[int] = None):
		self._owner = owner
		## the GPU that owns the memory (the owner's Context); consumers must not assume torch's current device
		ctx = getattr(owner, "ctx", None)
		self.device_index = int(device) if device is not None else (int(ctx.device) if ctx is not None else None)
		self.__cuda_array_interface__ = {
			"shape": tuple(int(v) for v in shape) if shape is not None else (int(count),),
			"typestr": "<f8" if np.dtype(dtype) == np.float64 else "<f4", "data": (int(dptr), False), "version": 2,
		}  # fmt: skip


class DeviceMatrix(_Handle):
	"""Column-major n x cols fp64 matrix on the GPU with the two tall-skinny products of the
	exchangeable estimators (slq_dmat_*: fp64 MFMA)."""

	_destroy = "slq_dmat_destroy"

	def __init__(self, n: int, cols: int, ctx: Optional[Context] = None):
		self.ctx = ctx or default_context()
		self.n, self.cols = int(n), int(cols)
		h = C.c_void_p()
		check(_capi.lib().slq_dmat_create(self.ctx._h, self.n, self.cols, C.byref(h)))
		self._h = h

	def set(self, c0: int, X: np.ndarray):
		X = np.asfortranarray(np.asarray(X, dtype=np.float64).reshape(self.n, -1))
		check(_capi.lib().slq_dmat_set(self._h, int(c0), X.shape[1], ptr(X), self.n))

	def get(self, c0: int = 0, nc: Optional[int] = None) -> np.ndarray:
		nc = self.cols - c0 if nc is None else int(nc)
		X = np.empty((self.n, nc), order="F")
		check(_capi.lib().slq_dmat_get(self._h, int(c0), nc, ptr(X), self.n))
		return X

	def col_ptr(self, c0: int) -> int:
		p = C.c_void_p()
		check(_capi.lib().slq_dmat_ptr(self._h, int(c0), C.byref(p)))
		return p.value

	def generate(self, c0: int, nc: int, pdf: str = "rademacher", seed: int = 0, probe_offset: int = 0):
		"""Isotropic probes into columns [c0, c0+nc): the device Philox stream, probe ids probe_offset + column."""
		assert pdf in _capi.PDF_IDS, f"Invalid distribution '{pdf}' supplied."
		check(_capi.lib().slq_dmat_generate(self._h, int(c0), int(nc), _capi.PDF_IDS[pdf], int(seed), int(probe_offset)))

	def copy_from(self, d0: int, src: "DeviceMatrix", s0: int, nc: int):
		"""self[:, d0:d0+nc] = src[:, s0:s0+nc] (device to device)."""
		check(_capi.lib().slq_dmat_copy(self._h, int(d0), src._h, int(s0), int(nc)))

	def copy_rows_from(self, d0: int, dr0: int, src: "DeviceMatrix", s0: int, sr0: int, nrows: int, nc: int):
		"""self[dr0:dr0+nrows, d0:d0+nc] = src[sr0:sr0+nrows, s0:s0+nc] (device to device; the matrices may differ in height)."""
		check(_capi.lib().slq_dmat_copy_rows(self._h, int(d0), int(dr0), src._h, int(s0), int(sr0), int(nrows), int(nc)))

	def cuda_array(self, c0: int, nc: int):
		"""Columns [c0, c0+nc) as a flat object with `__cuda_array_interface__` (zero-copy view for
		torch.as_tensor(..., device="cuda"): the RCCL collectives of primate_amd.distributed)."""
		assert 0 <= c0 and nc > 0 and c0 + nc <= self.cols
		return _CudaArrayView(self.col_ptr(c0), self.n * int(nc), self)

	def tn(self, a0: int, ma: int, B: "DeviceMatrix", b0: int, mb: int) -> np.ndarray:
		"""self[:, a0:a0+ma].T @ B[:, b0:b0+mb]  (ma x mb, on the host)."""
		out = np.zeros((ma, mb))
		check(_capi.lib().slq_dmat_gemm_tn(self._h, int(a0), int(ma), B._h, int(b0), int(mb), ptr(out)))
		return out

	def add_product(self, o0: int, A: "DeviceMatrix", a0: int, Cm: np.ndarray, alpha: float = 1.0, beta: float = 1.0):
		"""self[:, o0:o0+mb] = beta * self[:, o0:o0+mb] + alpha * A[:, a0:a0+ma] @ Cm."""
		Cm = np.ascontiguousarray(Cm, dtype=np.float64)
		ma, mb = Cm.shape
		check(_capi.lib().slq_dmat_gemm_nn(self._h, int(o0), A._h, int(a0), ma, ptr(Cm), mb, float(alpha), float(beta)))
