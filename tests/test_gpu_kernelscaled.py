"""The diagonally scaled kernel operator on the device (slq_kernelop.hpp: k_kernel_diag_scale, k_kernel_panel_scaled)
against the long-double model of tests/_kernelscaled_ref.py, elementwise within its forward bound; c == 1 against the unscaled
operator bit for bit (which pins the summation order and the schedule to the existing ones); the unscaled operator's own bits
across a set-then-clear; one plan through unscaled, scaled, other values and cleared under graph replay; and the refusals of the
entries that are not built for a scaled operator, through the raw ABI.

The shapes are those of tests/test_gpu_kernelop.py: n at both sides of the 16-point tile and the 128-row block, one slab and
several, d at both sides of the padding to 4 and past 16, P at both sides of every panel width. Each item prints its worst ratio
to the bar before it asserts (`-s` shows them)."""

import ctypes as C

import numpy as np
import pytest

import _kernelop_ref as R
import _kernelscaled_ref as S

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
LD = np.longdouble

## (dtype, n, d, P, profile, lengthscale, outputscale, noise): every value of every axis of the issue at least once; the four profiles
## spread over the cases as tests/test_gpu_kernelop.py spreads them
PER3, PER5 = (0.4, 0.6, 0.8), (0.5, 0.6, 0.7, 0.8, 0.9)
CASES = [
	(F64, 1, 1, 1, "rbf", 0.3, 1.0, 0.1),
	(F64, 15, 3, 16, "matern12", 0.5, 1.3, 0.0),
	(F64, 17, 5, 33, "matern32", PER5, 0.7, 0.05),
	(F64, 65, 5, 130, "matern52", 0.7, 2.0, 0.01),
	(F64, 257, 17, 260, "matern32", 1.5, 1.0, 0.1),
	(F64, 1000, 3, 16, "rbf", 0.5, 1.0, 0.0),
	(F32, 1, 1, 1, "matern12", 0.3, 1.0, 0.1),
	(F32, 15, 5, 33, "matern52", 0.7, 1.3, 0.0),
	(F32, 17, 3, 16, "rbf", PER3, 0.7, 0.05),
	(F32, 65, 17, 260, "matern32", 1.5, 2.0, 0.01),
	(F32, 257, 5, 130, "matern52", 1.0, 1.0, 0.0),
	(F32, 1000, 3, 16, "rbf", 0.5, 1.0, 0.1),
]


def _id(c):
	return f"{np.dtype(c[0]).name}-n{c[1]}-d{c[2]}-P{c[3]}-{c[4]}" + ("-perdim" if isinstance(c[5], tuple) else "")


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


_cache = {}


def case_data(c):
	"""Points, probes, the rounded z and c, the model's (Y, bar) and the operator object: computed once per case, read-only."""
	if c not in _cache:
		from primate_amd.operators import KernelOperator

		dtype, n, d, P, name, ell, s, noise = c
		X = R.points(n, d, seed=n + d, dtype=dtype)
		W = R.probes(n, P, seed=n + P, dtype=dtype)
		z = R.scaled_points(X, ell, dtype)
		cs = S.scale(n, n + d, dtype)
		Y, bar = S.model(z, name, s, noise, cs, W)
		for Z in (X, W, z, cs, Y, bar):
			Z.setflags(write=False)
		_cache[c] = (X, W, z, cs, Y, bar, KernelOperator(X, name, lengthscale=ell, outputscale=s, noise=noise, dtype=dtype, diag_scale=cs.astype(F64)))
	return _cache[c]


def device_scale(op, n, dtype):
	"""The npad words of the scale as the product kernel reads them (slq_debug_kernel_diag_scale)."""
	from primate_amd import _capi

	out = np.full((n + 15) // 16 * 16, np.nan, dtype)
	_capi.check(_capi.lib().slq_debug_kernel_diag_scale(op._h, _capi.ptr(out)))
	return out


def run_plan(eng, op, V, deg, orth=0):
	"""(alpha, beta) of a fresh plan's run on the probes V."""
	plan = eng.LanczosPlan(op, V.shape[1], deg, orth)
	try:
		plan.set_probes(V)
		plan.run()
		a, b = plan.tridiag()[:2]
		return np.array(a), np.array(b)
	finally:
		plan.close()


@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_product_at_every_edge(eng, c):
	"""The scale on the device is the rounded c, bit for bit, zeros in the padding. T = A W through slq_operator_matmat is elementwise
	within the model's bar; one Lanczos step's alpha_0 = v^T A v / |v|^2 within the bar carried through the dot product, as
	tests/test_gpu_kernelop.py carries it; and W^T (A V) = (A W)^T V within the summed bars: the operator is symmetric."""
	dtype, n, d, P, name, ell, s, noise = c
	X, W, z, cs, Y, bar, K = case_data(c)
	ratio = R.check_condition(Y, bar, dtype)
	op = eng.DeviceOperator(K)
	try:
		assert op.kind == "kernel" and op.kernel_parameters()["scaled"]
		got_c = device_scale(op, n, dtype)
		assert np.array_equal(got_c[:n], cs) and not got_c[n:].any()
		assert np.array_equal(op.kernel_diag_scale(), cs.astype(F64))
		got = op.matmat(W)
		w_mat = S.worst(got, Y, bar)
		deg = min(2, n)
		plan = eng.LanczosPlan(op, P, deg, 0)
		plan.set_probes(W)
		plan.run()
		a = plan.tridiag()[0][:, 0].astype(LD)
		plan.close()
		Wl = W.astype(LD)
		v2 = np.sum(Wl * Wl, axis=0)
		eps = LD(R.eps_of(dtype))
		want = np.sum(Wl * Y, axis=0) / v2
		abar = (np.sum(np.abs(Wl) * bar, axis=0) + LD(2 * n + 8) * eps * np.sum(np.abs(Wl) * np.abs(Y), axis=0)) / v2
		w_plan = float(np.max(np.abs(a - want) / abar))
		## symmetry: a second panel V of the same width; W^T (A V) against (A W)^T V
		V = R.probes(n, P, seed=n + P + 1, dtype=dtype)
		YV, barV = S.model(z, name, s, noise, cs, V)
		gotV = op.matmat(V)
		Vl = V.astype(LD)
		lhs, rhs = Wl.T @ gotV.astype(LD), (got.astype(LD)).T @ Vl
		sbar = np.abs(Wl).T @ barV + bar.T @ np.abs(Vl)
		w_sym = float(np.max(np.abs(lhs - rhs) / sbar))
		print(f"[kernelscaled] {_id(c)} bar/max|Y| {ratio:.2e} matmat {w_mat:.3f} plan-alpha {w_plan:.3f} symmetry {w_sym:.3f}")
		assert w_mat <= 1.0 and w_plan <= 1.0 and w_sym <= 1.0
	finally:
		op.close()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
@pytest.mark.parametrize("n", [257, 1000])
def test_unit_scale_equals_the_unscaled_operator_bitwise(eng, dtype, n):
	"""c == 1: matmat and a 10-step plan's tridiagonal carry the unscaled operator's bits - multiplying by 1 rounds nothing, so any
	difference would be another summation order or another schedule."""
	from primate_amd.operators import KernelOperator

	d, P = 3, 32
	X = R.points(n, d, seed=n, dtype=dtype)
	W = R.probes(n, P, seed=n, dtype=dtype)
	kw = dict(lengthscale=0.5, outputscale=1.3, noise=0.1, dtype=dtype)
	a, b = eng.DeviceOperator(KernelOperator(X, "matern32", **kw)), eng.DeviceOperator(KernelOperator(X, "matern32", diag_scale=np.ones(n), **kw))
	try:
		assert not a.kernel_parameters()["scaled"] and b.kernel_parameters()["scaled"]
		Ya, Yb = a.matmat(W), b.matmat(W)
		assert np.all(np.isfinite(Ya)) and np.array_equal(Ya, Yb)
		(aa, ba), (ab, bb) = run_plan(eng, a, W, 10, 3), run_plan(eng, b, W, 10, 3)
		assert np.all(np.isfinite(aa)) and np.array_equal(aa, ab) and np.array_equal(ba, bb)
	finally:
		a.close()
		b.close()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
def test_unscaled_bits_do_not_move(eng, dtype):
	"""An operator that never had a scale, and the same operator after set-then-clear: identical bits for matmat and a plan run."""
	from primate_amd.operators import KernelOperator

	n, d, P = 300, 4, 16
	X = R.points(n, d, seed=8, dtype=dtype)
	W = R.probes(n, P, seed=8, dtype=dtype)
	K = KernelOperator(X, "matern52", lengthscale=0.6, noise=0.05, dtype=dtype)
	fresh, used = eng.DeviceOperator(K), eng.DeviceOperator(K)
	try:
		used.set_kernel_diag_scale(S.scale(n, 8, dtype).astype(F64))
		scaled = used.matmat(W)
		used.set_kernel_diag_scale(None)
		assert used.kernel_diag_scale() is None and not used.kernel_parameters()["scaled"]
		Y0, Y1 = fresh.matmat(W), used.matmat(W)
		assert np.array_equal(Y0, Y1) and not np.array_equal(Y0, scaled)
		(a0, b0), (a1, b1) = run_plan(eng, fresh, W, 12, 3), run_plan(eng, used, W, 12, 3)
		assert np.array_equal(a0, a1) and np.array_equal(b0, b1)
	finally:
		fresh.close()
		used.close()


def test_graph_replay_through_set_change_clear(eng):
	"""ONE plan with the default switches (its runs replay captured graphs) runs unscaled, with a scale, with other values, with the
	scale cleared: each result equals, bitwise, a fresh plan's on a fresh operator in that state, and the last equals the first. Scaled
	and unscaled are different kernels: the state is part of the plan's graph key; new values reach a captured graph through the fixed
	address of the scale."""
	from primate_amd.operators import KernelOperator

	n, d, P, deg = 300, 3, 16, 20
	X = R.points(n, d, seed=9)
	V = R.probes(n, P, seed=9)
	kw = dict(lengthscale=0.5, outputscale=1.0, noise=0.1)
	c1, c2 = S.scale(n, 1, F64), S.scale(n, 2, F64, zeros=False)
	K = KernelOperator(X, "matern52", **kw)
	op = eng.DeviceOperator(K)
	plan = eng.LanczosPlan(op, P, deg, 3)

	def quad(pl):
		pl.set_probes(V)
		pl.run()
		return pl.quadrature("log"), np.array(pl.tridiag()[0])

	def fresh(c):
		o = eng.DeviceOperator(KernelOperator(X, "matern52", diag_scale=c, **kw))
		p = eng.LanczosPlan(o, P, deg, 3)
		try:
			return quad(p)
		finally:
			p.close()
			o.close()

	try:
		got = []
		for c in (None, c1, c2, None):
			K.set_diag_scale(c)  # (forwarded to the live device operator)
			first = quad(plan)
			again = quad(plan)  # (the second run replays the graph of this state)
			assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
			got.append(first)
			want = fresh(c)
			assert np.all(np.isfinite(want[0])) and np.array_equal(first[0], want[0]) and np.array_equal(first[1], want[1])
		assert np.array_equal(got[0][0], got[3][0]) and np.array_equal(got[0][1], got[3][1])
		assert not np.array_equal(got[0][0], got[1][0]) and not np.array_equal(got[1][0], got[2][0])
	finally:
		plan.close()
		op.close()


def test_bitwise_reproducible(eng):
	c = CASES[4]
	X, W, z, cs, Y, bar, K = case_data(c)
	op = eng.DeviceOperator(K)
	try:
		assert np.array_equal(op.matmat(W), op.matmat(W))
		plan = eng.LanczosPlan(op, 16, 20, 3)
		q = []
		for _ in range(2):
			plan.set_probes(W[:, :16])
			plan.run()
			q.append(plan.quadrature("log"))
		plan.close()
		assert np.all(np.isfinite(q[0])) and np.array_equal(q[0], q[1])
	finally:
		op.close()


def test_refusals_through_the_raw_abi(eng):
	from primate_amd import _capi
	from primate_amd.operators import KernelOperator

	L, ctx = _capi.lib(), eng.default_context()
	msg = lambda: L.slq_last_error().decode()  # noqa: E731
	n, d = 200, 3
	X = R.points(n, d, seed=2)
	W = R.probes(n, 8, seed=2)
	c = S.scale(n, 2, F64)
	scaled = eng.DeviceOperator(KernelOperator(X, "rbf", lengthscale=0.4, noise=0.1, diag_scale=c))
	plain = eng.DeviceOperator(KernelOperator(X, "rbf", lengthscale=0.4, noise=0.1))
	dense = eng.DeviceOperator(np.eye(4))
	h = C.c_void_p()
	try:
		## validation through the entry itself: the first bad index and value, the length, the kind
		bad = c.copy()
		bad[5], bad[9] = -0.5, np.nan
		assert L.slq_kernel_set_diag_scale(plain._h, _capi.ptr(bad), n) == _capi.SLQ_EINVAL and "diag_scale[5] = -0.5" in msg()
		bad[5] = np.inf
		assert L.slq_kernel_set_diag_scale(plain._h, _capi.ptr(bad), n) == _capi.SLQ_EINVAL and "diag_scale[5] = inf" in msg()
		assert L.slq_kernel_set_diag_scale(plain._h, _capi.ptr(c), n - 1) == _capi.SLQ_EINVAL and f"{n - 1} entries" in msg()
		assert L.slq_kernel_set_diag_scale(dense._h, _capi.ptr(c), 4) == _capi.SLQ_EINVAL
		assert plain.kernel_diag_scale() is None  # (a refused change changes nothing)
		out = np.empty(n)
		assert L.slq_kernel_get_diag_scale(plain._h, _capi.ptr(out), n, None) == _capi.SLQ_EINVAL
		assert L.slq_kernel_get_diag_scale(scaled._h, _capi.ptr(out), n - 1, None) == _capi.SLQ_EINVAL
		assert L.slq_debug_kernel_diag_scale(plain._h, _capi.ptr(out)) == _capi.SLQ_EINVAL
		## gradients, point gradients of the training form and the preconditioner: refused at creation on a scaled operator
		for who, call in (
			("slq_kernel_grad_create", lambda: L.slq_kernel_grad_create(ctx._h, scaled._h, C.byref(h))),
			("slq_kernel_pointgrad_create", lambda: L.slq_kernel_pointgrad_create(ctx._h, scaled._h, C.byref(h))),
			("slq_kernel_precond_create", lambda: L.slq_kernel_precond_create(ctx._h, scaled._h, 16, 0.0, C.byref(h))),
		):
			assert call() == _capi.SLQ_EINVAL and who in msg() and "diagonal scale" in msg() and "not built" in msg()
			assert h.value is None
		## ... and at every use: objects created on the unscaled operator refuse once it is scaled, and work again once it is cleared
		acc, pacc = eng.KernelGradAccumulator(plain), eng.KernelPointGradAccumulator(plain)
		Z = eng.DeviceMatrix(n, 8, ctx=ctx)
		Z.set(0, W)
		pre = eng.DeviceOperator(KernelOperator(X, "rbf", lengthscale=0.4, noise=0.1).preconditioned(16), ctx=ctx)
		base = pre.base
		plan = eng.LanczosPlan(pre, 8, 10, 3)
		try:
			plan.set_probes(W)
			plan.run()
			q0 = plan.quadrature("log")
			plain.set_kernel_diag_scale(c)
			base.set_kernel_diag_scale(c)
			for call in (lambda: acc.update(Z, 0, Z, 0, 8), lambda: pacc.update(Z, 0, Z, 0, 8), pre.refresh, lambda: pre.inv_sqrt(W)):
				with pytest.raises(ValueError, match="diagonal scale"):
					call()
			plan.set_probes(W)
			with pytest.raises(ValueError, match="diagonal scale"):
				plan.run()
			plain.set_kernel_diag_scale(None)
			base.set_kernel_diag_scale(None)
			acc.update(Z, 0, Z, 0, 8)
			pacc.update(Z, 0, Z, 0, 8)
			pre.refresh()
			plan.set_probes(W)
			plan.run()
			assert np.array_equal(plan.quadrature("log"), q0)
		finally:
			for obj in (plan, pre, Z, pacc, acc):
				obj.close()
		## a cross product over the training points ignores the scale: the unscaled operator's bits
		ca, cb = eng.KernelCross(scaled, X), eng.KernelCross(plain, X)
		try:
			assert np.array_equal(ca.matmat(W), cb.matmat(W)) and np.array_equal(ca.matmat(W, trans=True), cb.matmat(W, trans=True))
		finally:
			ca.close()
			cb.close()
	finally:
		for op in (scaled, plain, dense):
			op.close()
