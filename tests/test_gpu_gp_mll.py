"""The marginal likelihood with gradients through the preconditioner on the device (k_precond_columns,
slq_kernel_precond_trace_grad, gp.logdet_grad, gp.mll, autograd.gp_mll_fun): the factor's columns L and L H against the factor read
back, the exact part tr(P^-1 dA/dtheta) against the dense inverse at 1.0 of the bar of tests/_gp_mll_ref.py (the CPU emulation is held
to half of it), the estimator on explicit probes against the dense evaluation of the same formula, its statistics, the marginal
likelihood by its parts, posterior's bits against the parent commit's fingerprint, staleness and the torch function. Each item prints
its measured figures before it asserts (`-s` shows them; §4.19 quotes them)."""

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import _gp_mll_ref as M
import _kernelgrad_ref as G
import _kernelop_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
LD = np.longdouble
EPS = float(M.EPS)


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def fold(v, d):
	"""(..., d + 2) per-dimension values to a scalar lengthscale's (..., 3)."""
	v = np.asarray(v)
	return np.concatenate([v[..., :d].sum(axis=-1, keepdims=True), v[..., d:]], axis=-1)


def vec(grads):
	return np.concatenate([np.ravel(grads["lengthscale"]), [grads["outputscale"]], [grads["noise"]]])


## ---- 1. the columns -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 15, 17, 65, 1000))
def test_factor_columns(eng, n):
	"""factor_columns against L (bit for bit) and L @ H (long double, within (rpad + 8) eps sum_j |L_ij| |H_jc| elementwise) of the
	factor read back, at rank 1, 37, 64, 128, 256 (clamped to n), chunks c0 = 0, 64, 192 with 1, 63, 64 columns where they fit, an
	offset into OUT, and two calls with equal bits. Nothing but the columns asked for is written."""
	from primate_amd.operators import KernelOperator

	K = KernelOperator(R.points(n, 2, seed=n), "rbf", lengthscale=0.3, outputscale=1.0, noise=1e-3)
	worst = 0.0
	for rank in sorted({min(r, n) for r in (1, 37, 64, 128, 256)}):  # (rank_max is clamped to n)
		op = eng.DeviceOperator(K.preconditioned(rank))
		f = op.factor()
		r = f["L"].shape[1]
		rpad = (r + 15) // 16 * 16
		Lp, Hp = np.zeros((n, rpad)), np.zeros((rpad, rpad))
		Lp[:, :r], Hp[:r, :r] = f["L"], f["H"]
		assert np.array_equal(f["H"], f["H"].T)
		OUT = eng.DeviceMatrix(n, 70, ctx=op.ctx)
		sentinel = np.full((n, 70), -7.25)

		def columns(which, c0, nc, o0):
			OUT.set(0, sentinel)
			op.factor_columns(which, c0, nc, OUT, o0)
			got = OUT.get()
			assert np.all(got[:, :o0] == -7.25) and np.all(got[:, o0 + nc :] == -7.25), "a column outside the range was written"
			return got[:, o0 : o0 + nc]

		for c0 in (0, 64, 192):
			for nc in (1, 63, 64):
				if c0 + nc > rpad:
					continue
				cols = slice(c0, c0 + nc)
				assert np.array_equal(columns(0, c0, nc, 0), Lp[:, cols]), f"n {n} rank {rank} c0 {c0} nc {nc}: L is not copied bit for bit"
				got = columns(1, c0, nc, 3)
				assert np.array_equal(columns(1, c0, nc, 3), got), "two calls must give identical bits"
				ref = Lp.astype(LD) @ Hp[:, cols].astype(LD)
				bar = LD(rpad + 8) * M.EPS * (np.abs(Lp).astype(LD) @ np.abs(Hp[:, cols]).astype(LD))
				err = np.abs(got.astype(LD) - ref)
				ok = bar > 0
				assert np.all(err[~ok] == 0)
				if ok.any():
					worst = max(worst, float(np.max(err[ok] / bar[ok])))
		OUT.close()
		op.close()
	print(f"[gp-mll-columns] n {n}: worst |L H - ref| / ((rpad + 8) eps |L||H|) {worst:.3f}")
	assert worst <= 1.0


def test_column_and_trace_grad_refusals(eng):
	from primate_amd import _capi
	from primate_amd.operators import KernelOperator

	L = _capi.lib()
	msg = lambda: L.slq_last_error().decode()  # noqa: E731
	X = R.points(40, 2, seed=2)
	K = KernelOperator(X, "rbf", lengthscale=0.3, noise=1e-2)
	K2 = KernelOperator(X, "rbf", lengthscale=0.3, noise=1e-2)
	base, other = eng.DeviceOperator(K), eng.DeviceOperator(K2)
	pre = K.preconditioned(20)
	op = eng.DeviceOperator(pre)  # (its base is its own device operator of K)
	OUT, short = eng.DeviceMatrix(40, 64, ctx=op.ctx), eng.DeviceMatrix(39, 64, ctx=op.ctx)
	acc, foreign = eng.KernelGradAccumulator(op.base), eng.KernelGradAccumulator(other)
	try:
		cols = lambda o, which, c0, nc, out, o0: L.slq_kernel_precond_columns(o._h, which, c0, nc, out._h, o0)  # noqa: E731
		assert cols(base, 0, 0, 1, OUT, 0) == _capi.SLQ_EINVAL and "'kernel'" in msg()
		assert cols(op, 2, 0, 1, OUT, 0) == _capi.SLQ_EINVAL and "which" in msg()
		for c0, nc in ((-1, 1), (0, 0), (0, 65), (30, 3), (32, 1)):  # rpad = 32
			assert cols(op, 1, c0, nc, OUT, 0) == _capi.SLQ_EINVAL and "column range" in msg(), (c0, nc)
		assert cols(op, 1, 0, 4, OUT, 61) == _capi.SLQ_EINVAL and "outside" in msg()
		assert cols(op, 1, 0, 4, short, 0) == _capi.SLQ_EINVAL and "row mismatch" in msg()
		tg = lambda o, a: L.slq_kernel_precond_trace_grad(o._h, a._h, 1.0, 0.0)  # noqa: E731
		assert tg(base, acc) == _capi.SLQ_EINVAL and "'kernel'" in msg()
		assert tg(op, foreign) == _capi.SLQ_EINVAL and "another operator" in msg()
		assert L.slq_kernel_precond_trace_grad(op._h, None, 1.0, 0.0) == _capi.SLQ_EINVAL
		assert L.slq_kernel_precond_trace_grad(op._h, acc._h, float("nan"), 0.0) == _capi.SLQ_EINVAL and "finite" in msg()
		with pytest.raises(ValueError, match="preconditioned kernel operator"):
			base.factor_columns(0, 0, 1, OUT)
		with pytest.raises(ValueError, match="preconditioned kernel operator"):
			base.precond_trace_grad(acc)
		## stale: the raw entries say so until the refresh; the accumulator is untouched
		op.precond_trace_grad(acc, 1.0, 0.0)
		before, cnt = acc.get()
		assert cnt == 0, "the exact part folds no probe in: the column count stays"
		K.set_parameters(lengthscale=0.4)
		assert cols(op, 1, 0, 4, OUT, 0) == _capi.SLQ_EINVAL and "stale" in msg()
		assert tg(op, acc) == _capi.SLQ_EINVAL and "stale" in msg()
		assert np.array_equal(acc.get()[0], before)
		op.refresh()
		assert cols(op, 1, 0, 4, OUT, 0) == _capi.SLQ_OK and tg(op, acc) == _capi.SLQ_OK
		assert not np.array_equal(acc.get()[0], before)
		## the existing refusal stays: no accumulator on the preconditioned operator itself
		h = C.c_void_p()
		assert L.slq_kernel_grad_create(op.ctx._h, op._h, C.byref(h)) == _capi.SLQ_EINVAL and "kernel_precond" in msg()
	finally:
		for x in (acc, foreign, OUT, short, op, base, other):
			x.close()


## ---- 2. the exact part ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", M.CASES, ids=[M.case_id(c) for c in M.CASES])
def test_exact_part(eng, c):
	"""precond_trace_grad against tr(P^-1 D) of the dense inverse of the device's own L, at 1.0 of the bar; alpha and beta are honoured
	and two calls give equal bits."""
	n, d, name, ell, s, sigma2, rank, note = c
	K = M.operator(c)
	op = eng.DeviceOperator(K.preconditioned(rank))
	acc = eng.KernelGradAccumulator(op.base)
	try:
		f = op.factor()
		g, bar, trD = M.exact_model(c, np.array(f["L"]), np.array(f["H"]))
		if n > 1:
			G.check_condition(g, bar)
		op.precond_trace_grad(acc, 1.0, 0.0)
		got, cnt = acc.get()
		frac = G.worst(got, g, bar)
		each = np.array(np.abs(got.astype(LD) - g) / np.where(bar > 0, bar, LD(1)), dtype=float)
		print(f"[gp-mll-exact] {M.case_id(c)}: rank {op.info()['rank']} error / bar {frac:.3f} (lengthscales {np.max(each[:d]):.3f}, outputscale {each[d]:.3f}, noise {each[d + 1]:.3f})")
		assert cnt == 0
		op.precond_trace_grad(acc, 1.0, 0.0)
		assert np.array_equal(acc.get()[0], got), "two calls must give identical bits"
		op.precond_trace_grad(acc, -0.5, 2.0)  # 2 g - 0.5 g
		assert np.allclose(acc.get()[0], 1.5 * got, rtol=1e-12, atol=0)
		assert frac <= 1.0
	finally:
		acc.close()
		op.close()


## ---- 3., 4. the estimator on explicit probes, and its statistics ------------------------------------------------------------------
N3, D3, ELL3, S23 = 400, 2, 0.3, 1e-4
_est = {}


def estimator_setup(eng, rank):
	"""The issue's case (n = 400, rbf, d = 2, lengthscale 0.3, sigma2 = 1e-4) at a rank: the preconditioned operator (kept: a training
	loop's form), the device's L, the dense A, D, M of that L and 64 Rademacher probes. Once per rank, read-only."""
	if rank not in _est:
		from primate_amd.operators import KernelOperator

		K = KernelOperator(R.points(N3, D3, seed=400), "rbf", lengthscale=ELL3, outputscale=1.0, noise=S23)
		B = K.preconditioned(rank)
		from primate_amd.lanczos import _as_device_operator

		L = np.array(_as_device_operator(B, dtype=np.float64).factor()["L"])
		z = K.scaled_points().astype(np.float64)
		A = M.dense_a(z, "rbf", 1.0, S23).astype(np.float64)
		D = M.dense_D(z, "rbf", ELL3, 1.0)
		Minv, condP = M.minv_dense(L, S23)
		exact = M.trace_inv(M.inv_ld(M.dense_p(L, S23)), D).astype(np.float64)
		full = M.trace_inv(M.inv_ld(A.astype(LD)), D).astype(np.float64)
		W = M.rademacher(N3, 64, seed=17)
		_est[rank] = dict(K=K, B=B, L=L, A=A, D=D.astype(np.float64), Minv=Minv, condP=condP, exact=exact, full=full, W=W)
	return _est[rank]


def oracle_inverse_action(oracle, deg, orth=3):
	"""B^-1 W as `deg` steps of the oracle's Lanczos give it: ||w|| Q T^-1 e_1 per probe."""

	def act(Bd, W):
		n = Bd.shape[0]
		out = np.empty_like(W)
		Bf = np.asfortranarray(Bd)
		for c in range(W.shape[1]):
			a, b, Q = np.zeros(deg + 1), np.zeros(deg + 1), np.zeros((n, deg), order="F")
			k = oracle.lanczos(Bf, W[:, c], deg, 0.0, orth, a, b, Q)
			T = np.diag(a[:k]) + np.diag(b[1:k], 1) + np.diag(b[1:k], -1)
			out[:, c] = np.linalg.norm(W[:, c]) * (Q[:, :k] @ np.linalg.solve(T, np.eye(k)[:, 0]))
		return out

	return act


@pytest.mark.parametrize("rank,deg,auto_on", ((64, 20, True), (40, 30, False)))
def test_estimator_on_explicit_probes(eng, oracle, rank, deg, auto_on):
	"""logdet_grad on 64 host Rademacher probes in batches of 8 against the dense evaluation of the same formula on the same probes and
	the device's L: `auto` decides as the Ritz values say, each forced mode is checked, the bar is 100 cond(P) eps S_theta, S_theta =
	(1/N) sum_c |U_c|^T |D_theta| |Vm_c|, plus the model's own Lanczos truncation (the oracle's degree-`deg` inverse action on the dense
	B against the exact solve) plus, with the control variate on, the exact part's bar. The value is gp.logdet's on the same probes,
	bit for bit."""
	from primate_amd import gp

	E = estimator_setup(eng, rank)
	K, B, W, D, d = E["K"], E["B"], E["W"], E["D"], D3
	runs = {}
	for mode in ("auto", True, False):
		runs[mode] = gp.logdet_grad(B, deg=deg, count=64, batch=8, probes=W, control_variate=mode)
	value, grads, info = runs["auto"]
	print(f"[gp-mll-estimator] rank {rank} deg {deg}: ritz_max {info['ritz_max']:.4f} -> control variate {info['control_variate']}")
	assert info["control_variate"] is auto_on and (info["ritz_max"] <= 2.0) is auto_on
	assert runs[True][2]["control_variate"] is True and runs[False][2]["control_variate"] is False
	same = runs[auto_on]
	assert value == same[0] and np.array_equal(vec(grads), vec(same[1])), "auto is the mode it chose, bit for bit"
	assert runs[False][2]["grad_exact"] is None and runs[True][2]["grad_exact"] is not None
	exact_bar = fold(np.array(M.exact_model((N3, D3, "rbf", ELL3, 1.0, S23, rank, ""), E["L"], _device_h(B))[1], dtype=float), d)
	for on in (True, False):
		v, g, inf = runs[on]
		terms, U, Vm = M.estimator_terms(E["A"], E["Minv"], D, W, on)
		trunc_terms, _, _ = M.estimator_terms(E["A"], E["Minv"], D, W, on, Binv_action=oracle_inverse_action(oracle, deg))
		model = fold(terms.mean(axis=0) + (E["exact"] if on else 0.0), d)
		trunc = np.abs(fold(trunc_terms.mean(axis=0) - terms.mean(axis=0), d))
		S = fold(np.array([np.mean(np.einsum("ic,ic->c", np.abs(U), np.abs(Dk) @ np.abs(Vm))) for Dk in D]), d)
		bar = 100.0 * E["condP"] * np.finfo(np.float64).eps * S + trunc + (exact_bar if on else 0.0)
		err = np.abs(vec(g) - model)
		print(f"[gp-mll-estimator] rank {rank} deg {deg} control variate {on}: error / bar {err / bar} (truncation share of the bar {trunc / bar}); grads {vec(g)}")
		assert np.all(err <= bar)
		assert inf["count"] == 64 and inf["batches"] == 8 and inf["grad_std_error"] is not None
	## the value: gp.logdet through hutch on the same probes, handed out batch by batch
	served = [0]

	def pdf(size):
		c0 = served[0]
		served[0] += size[1]
		return W[:, c0 : c0 + size[1]]

	want, linfo = gp.logdet(K, rank=rank, deg=deg, count=64, batch=8, pdf=pdf)
	assert served[0] == 64
	assert value == want and info["trace"] == linfo["trace"] and info["std_error"] == linfo["std_error"], "the value is gp.logdet's, bit for bit"


def _device_h(B):
	from primate_amd.lanczos import _as_device_operator

	return np.array(_as_device_operator(B, dtype=np.float64).factor()["H"])


def test_statistics_at_rank_64(eng):
	"""Every component within 4 grad_std_error of the dense tr(A^-1 D); the control variate cuts grad_std_error to a tenth or less on
	the same probes (the CPU's exact solves gave 1/29 ... 1/55 on 32 probes)."""
	from primate_amd import gp

	E = estimator_setup(eng, 64)
	full = fold(E["full"], D3)
	on = gp.logdet_grad(E["B"], deg=20, count=64, batch=8, probes=E["W"], control_variate=True)
	off = gp.logdet_grad(E["B"], deg=20, count=64, batch=8, probes=E["W"], control_variate=False)
	se_on, se_off = vec(on[2]["grad_std_error"]), vec(off[2]["grad_std_error"])
	print(f"[gp-mll-statistics] tr(A^-1 D) {full}; on {vec(on[1])} +- {se_on}; off {vec(off[1])} +- {se_off}; ratio {se_on / se_off}")
	assert np.all(np.abs(vec(on[1]) - full) <= 4 * se_on)
	assert np.all(np.abs(vec(off[1]) - full) <= 4 * se_off)
	assert np.all(se_on <= se_off / 10)


## ---- 5. the marginal likelihood -----------------------------------------------------------------------------------------------------
def test_mll_by_its_parts(eng):
	"""n = 300, matern52, d = 3, sigma2 = 1e-3, rank 100, y with a zero column: the data-fit value and gradient against the dense
	solve within 100 cond(A) eps (relative to the largest component), the log-determinant part equal to logdet_grad's on the same
	seed bit for bit, and the total assembled from the two. The solve takes 150 steps (solve_deg): at matern52 a rank-100 factor leaves
	cond(B) in the tens, and 20 steps - enough for the log-determinant's quadrature - leave alpha at 8e-5 (measured), which is a property
	of the degree, not an error."""
	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	n, d, s, sigma2 = 300, 3, 1.2, 1e-3
	rng = np.random.default_rng(719)
	X = rng.random((n, d))
	y = np.zeros((n, 2))
	y[:, 0] = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(n)
	K = KernelOperator(X, "matern52", lengthscale=0.4, outputscale=s, noise=sigma2)
	value, grads, info = gp.mll(K, y, rank=100, deg=20, solve_deg=150, count=32, batch=8, seed=5)
	z = K.scaled_points().astype(np.float64)
	A = M.dense_a(z, "matern52", s, sigma2)
	Dm = M.dense_D(z, "matern52", 0.4, s)
	alpha = M.inv_ld(A) @ y[:, 0].astype(LD)
	fit = float(-0.5 * (y[:, 0].astype(LD) @ alpha))
	fit_grad = fold(np.array([0.5 * (alpha @ (Dk @ alpha)) for Dk in Dm], dtype=float), d)
	bar = 100.0 * float(np.linalg.cond(A.astype(np.float64))) * float(np.finfo(np.float64).eps)
	e_val = abs(info["datafit"] - fit) / abs(fit)
	e_grad = float(np.max(np.abs(vec(info["datafit_grad"]) - fit_grad)) / np.max(np.abs(fit_grad)))
	print(f"[gp-mll-mll] cond(A) {np.linalg.cond(A.astype(np.float64)):.2e} bar {bar:.2e}: data fit within {e_val:.2e}, its gradient within {e_grad:.2e}; steps {info['steps']}")
	assert e_val <= bar and e_grad <= bar
	assert info["q"] == 2 and info["zero_columns"] == [1]
	ld, ld_grads, ld_info = gp.logdet_grad(K, rank=100, deg=20, count=32, batch=8, seed=5)
	assert info["logdet"] == ld and np.array_equal(vec(info["logdet_grad"]), vec(ld_grads))
	q = 2
	assert value == info["datafit"] - 0.5 * q * ld - 0.5 * n * q * float(np.log(2.0 * np.pi))
	assert np.array_equal(vec(grads), vec(info["datafit_grad"]) - 0.5 * q * vec(ld_grads))
	assert np.array_equal(vec(info["grad_std_error"]), 0.5 * q * vec(ld_info["grad_std_error"]))
	## the sampled part is an estimate of the truth: 5 standard errors, and the log-determinant within 5 of its own
	full = fold(M.trace_inv(M.inv_ld(A), Dm).astype(np.float64), d)
	assert np.all(np.abs(vec(ld_grads) - full) <= 5 * vec(ld_info["grad_std_error"]))
	assert abs(ld - float(np.linalg.slogdet(A.astype(np.float64))[1])) <= 5 * ld_info["std_error"] + 1e-6
	## a vector y is the one-column case; all-zero observations leave the log-determinant terms alone
	v1, g1, i1 = gp.mll(K, y[:, 0], rank=100, deg=20, solve_deg=150, count=32, batch=8, seed=5)
	assert i1["q"] == 1 and i1["datafit"] == info["datafit"] and v1 == info["datafit"] - 0.5 * ld - 0.5 * n * float(np.log(2.0 * np.pi))
	v0, g0, i0 = gp.mll(K, np.zeros(n), rank=100, deg=20, count=32, batch=8, seed=5)
	assert i0["datafit"] == 0.0 and i0["steps"] is None and np.array_equal(vec(g0), -0.5 * vec(ld_grads))


def test_posterior_keeps_the_parent_commits_bits(eng):
	"""posterior without and with the preconditioner - its solve helper is now shared with mll - gives the lines
	scripts/op_fingerprint.py --posterior printed on the parent commit (profiles/gp_mll_posterior_fingerprint.txt)."""
	want = [ln for ln in (ROOT / "profiles" / "gp_mll_posterior_fingerprint.txt").read_text().splitlines() if ln.startswith("posterior ")]
	assert len(want) == 2
	assert M.posterior_fingerprint_lines() == want


## ---- 6. staleness -----------------------------------------------------------------------------------------------------------------
def test_lazy_refresh_equals_a_fresh_operator(eng):
	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	X = R.points(200, 2, seed=9)
	K = KernelOperator(X, "matern32", lengthscale=0.3, outputscale=1.0, noise=1e-3)
	B = K.preconditioned(48)
	first = gp.logdet_grad(B, deg=20, count=16, batch=8, seed=3, control_variate=True)
	K.set_parameters(lengthscale=0.35, outputscale=1.1, noise=2e-3)
	again = gp.logdet_grad(B, deg=20, count=16, batch=8, seed=3, control_variate=True)  # (the same device operator, refreshed lazily)
	K2 = KernelOperator(X, "matern32", lengthscale=0.35, outputscale=1.1, noise=2e-3)
	fresh = gp.logdet_grad(K2.preconditioned(48), deg=20, count=16, batch=8, seed=3, control_variate=True)
	assert again[0] == fresh[0] and np.array_equal(vec(again[1]), vec(fresh[1])), "a refreshed factor gives a fresh operator's bits"
	assert again[0] != first[0]
	assert np.array_equal(vec(again[2]["grad_exact"]), vec(fresh[2]["grad_exact"]))


## ---- 7. torch -----------------------------------------------------------------------------------------------------------------------
def test_gp_mll_fun_backward(eng):
	import torch

	from primate_amd import gp
	from primate_amd.autograd import gp_mll_fun
	from primate_amd.operators import KernelOperator

	rng = np.random.default_rng(3)
	X = rng.random((150, 2))
	y = np.cos(4.0 * X[:, 0]) + 0.05 * rng.standard_normal(150)
	ls0, s0, v0 = np.array([0.3, 0.5]), 1.1, 1e-3
	K = KernelOperator(X, "matern52", lengthscale=ls0, outputscale=s0, noise=v0)
	value, grads, _ = gp.mll(K, y, rank=40, deg=20, count=16, batch=8, seed=2)
	for scale in (1.0, 3.0):
		ls = torch.tensor(ls0, dtype=torch.float64, requires_grad=True)
		s = torch.tensor(s0, dtype=torch.float64, requires_grad=True)
		v = torch.tensor(v0, dtype=torch.float64, requires_grad=True)
		out = gp_mll_fun(torch.from_numpy(X), torch.from_numpy(y), "matern52", ls, s, v, rank=40, deg=20, count=16, seed=2, batch=8)
		assert float(out.detach()) == value
		(scale * out).backward()
		assert np.array_equal(ls.grad.numpy(), scale * grads["lengthscale"]) and float(s.grad) == scale * grads["outputscale"] and float(v.grad) == scale * grads["noise"]
	with pytest.raises(ValueError, match="unknown arguments"):
		gp_mll_fun(X, y, "rbf", 0.3, 1.0, 1e-3, orth=3)
