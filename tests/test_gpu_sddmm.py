"""The sampled dense-dense product on a CSR pattern (slq_sddmm_*, engine.SddmmAccumulator) and the gradient of tr f(A) built on it
(primate_amd.grad.trace_grad, primate_amd.autograd.trace_fun) on the device, against the NumPy model
tests/_sddmm_ref.py (validated on the CPU by tests/test_sddmm_cpu.py). Every test needs a real MI355X (`-m gpu`).

The kernel rule, per stored entry e and per update: |vals_dev[e] - vals_ld[e]| <= bar[e] = 2 (T + 2) 2^-53 (|alpha| sum_j |W_rj| |Z_cj|
+ |beta| |old_e|), T = m (2 m when symmetric), with `old` the device's own values before the update - so every update of a sequence
is held to the bar of one update."""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import _sddmm_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


_PATTERNS = {}


def pattern(which):
	if which not in _PATTERNS:
		P = {"grid": R.grid_pattern, "random": R.random_pattern}[which]()
		_PATTERNS[which] = (P, *R.pattern_rows_cols(P))
	return _PATTERNS[which]


## ---- 1. the kernel against the model ------------------------------------------------------------------------------------
W0, Z0, COLS = 3, 5, 80  # the updates read columns [3, 3 + m) of W and [5, 5 + m) of Z, inside matrices of 80 columns


def run_sequence(eng, P, Wh, Zh, m, symmetric, alias):
	"""Two updates with beta = 1, then one with beta = 0, on a fresh accumulator: the values after each."""
	n = P.shape[0]
	Wd = eng.DeviceMatrix(n, COLS)
	Wd.set(0, Wh)
	Zd = Wd if alias else eng.DeviceMatrix(n, COLS)
	if not alias:
		Zd.set(0, Zh)
	acc = eng.SddmmAccumulator(P)
	out = []
	for alpha, beta in ((0.75, 1.0), (-1.5, 1.0), (2.0, 0.0)):
		acc.update(Wd, W0, Zd, Z0, m, alpha=alpha, beta=beta, symmetric=symmetric)
		out.append(acc.get())
	for d in {id(Wd): Wd, id(Zd): Zd}.values():
		d.close()
	acc.close()
	return out


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("which", ["grid", "random"])
def test_kernel_against_the_model(eng, which, symmetric):
	P, rows, cols = pattern(which)
	n = P.shape[0]
	rng = np.random.default_rng(11)
	Wh, Zh = rng.standard_normal((n, COLS)), rng.standard_normal((n, COLS))
	for m in (1, 7, 64, 70):
		for alias in (False, True):
			Zm = Wh if alias else Zh
			Wc, Zc = Wh[:, W0 : W0 + m], Zm[:, Z0 : Z0 + m]
			seq = run_sequence(eng, P, Wh, Zh, m, symmetric, alias)
			old, count = np.zeros(P.nnz), 0
			for (alpha, beta), (got, cnt) in zip(((0.75, 1.0), (-1.5, 1.0), (2.0, 0.0)), seq):
				count += m
				assert cnt == count
				want = R.vals_ld(rows, cols, Wc, Zc, alpha, beta, old, symmetric)
				bar = R.bar(rows, cols, Wc, Zc, alpha, beta, old, symmetric)
				err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
				worst = int(np.argmax(err - bar))
				print(f"{which} m={m} sym={symmetric} alias={alias} alpha={alpha} beta={beta}: max err/bar {np.max(err / np.maximum(bar, 1e-300)):.3f}")
				assert np.all(err <= bar), f"{which} m={m} alias={alias} (alpha, beta)=({alpha}, {beta}): entry {worst} err {err[worst]:.3e} > bar {bar[worst]:.3e}"
				old = got
			again = run_sequence(eng, P, Wh, Zh, m, symmetric, alias)
			for (a, _), (b, _) in zip(seq, again):
				assert np.array_equal(a, b), "two identical sequences must give identical bits"


def test_device_pattern_reset_and_zero_copy_view(eng):
	"""A torch CSR pattern on the GPU (slq_sddmm_create_device) gives the bits of the host pattern; reset; the CUDA view; nnz = 0."""
	import torch

	P, rows, cols = pattern("random")
	n = P.shape[0]
	rng = np.random.default_rng(12)
	Wh = rng.standard_normal((n, 9))
	Wd = eng.DeviceMatrix(n, 9)
	Wd.set(0, Wh)
	T = torch.sparse_csr_tensor(torch.from_numpy(P.indptr.astype(np.int64)), torch.from_numpy(P.indices.astype(np.int64)), torch.from_numpy(P.data), size=P.shape).cuda()
	a, b = eng.SddmmAccumulator(P), eng.SddmmAccumulator(T)
	for acc in (a, b):
		acc.update(Wd, 0, Wd, 2, 7, alpha=0.5)
	va, ca = a.get()
	vb, cb = b.get()
	assert np.array_equal(va, vb) and ca == cb == 7
	view = torch.as_tensor(b.cuda_array(), device="cuda")
	assert view.shape == (P.nnz,) and view.dtype == torch.float64 and np.array_equal(view.cpu().numpy(), vb)
	b.reset()
	vz, cz = b.get()
	assert cz == 0 and not vz.any()
	e = eng.SddmmAccumulator(R.empty_pattern(n))
	e.update(Wd, 0, Wd, 0, 9)
	ve, ce = e.get()
	assert ve.size == 0 and ce == 9
	bad = torch.sparse_csr_tensor(torch.tensor([0, 1, 2]), torch.tensor([0, 2]), torch.tensor([1.0, 1.0], dtype=torch.float64), size=(2, 2), check_invariants=False).cuda()
	with pytest.raises(ValueError, match="row 1"):
		eng.SddmmAccumulator(bad)
	for d in (a, b, e, Wd):
		d.close()


## ---- 2. guards ----------------------------------------------------------------------------------------------------------
def test_guards_return_einval_and_leave_the_values(eng):
	from primate_amd import _capi
	from primate_amd._capi import ptr

	L = _capi.lib()
	ctx = eng.default_context()
	P, rows, cols = pattern("grid")
	n = P.shape[0]
	h = C.c_void_p()
	rp, ci = P.indptr.astype(np.int32), P.indices.astype(np.int32)
	bad_rp = rp.copy()
	bad_rp[5], bad_rp[6] = rp[6], rp[5]  # rows 4 and 5: rowptr goes down at row 5
	assert L.slq_sddmm_create(ctx._h, n, P.nnz, ptr(bad_rp), ptr(ci), C.byref(h)) == _capi.SLQ_EINVAL and not h.value
	assert b"row 5" in L.slq_last_error()
	bad_ci = ci.copy()
	bad_ci[rp[9]] = n  # a column index equal to n, in row 9
	assert L.slq_sddmm_create(ctx._h, n, P.nnz, ptr(rp), ptr(bad_ci), C.byref(h)) == _capi.SLQ_EINVAL and not h.value
	assert b"row 9" in L.slq_last_error()
	short_rp = rp.copy()
	short_rp[-1] -= 1  # rowptr[n] != nnz
	assert L.slq_sddmm_create(ctx._h, n, P.nnz, ptr(short_rp), ptr(ci), C.byref(h)) == _capi.SLQ_EINVAL and not h.value

	rng = np.random.default_rng(13)
	Wd, tall = eng.DeviceMatrix(n, 8), eng.DeviceMatrix(n + 1, 8)
	Wd.set(0, rng.standard_normal((n, 8)))
	acc = eng.SddmmAccumulator(P)
	acc.update(Wd, 0, Wd, 0, 8)
	before, cnt = acc.get()
	other = eng.Context(device=ctx.device)
	foreign = eng.DeviceMatrix(n, 8, ctx=other)
	for args, what in [((tall, 0, Wd, 0, 8), "rows"), ((Wd, 0, tall, 0, 8), "rows"), ((Wd, 4, Wd, 0, 8), "outside"), ((Wd, 0, Wd, -1, 4), "outside"),
					   ((Wd, 0, Wd, 0, 0), "outside"), ((foreign, 0, Wd, 0, 8), "another context"), ((Wd, 0, foreign, 0, 8), "another context")]:  # fmt: skip
		rc = L.slq_sddmm_update(acc._h, args[0]._h, args[1], args[2]._h, args[3], args[4], 1.0, 1.0, 0)
		assert rc == _capi.SLQ_EINVAL, what
		assert what.encode() in L.slq_last_error(), (what, L.slq_last_error())
	with pytest.raises(ValueError):
		acc.update(Wd, 0, Wd, 0, 8, alpha=float("nan"))
	after, cnt2 = acc.get()
	assert np.array_equal(before, after) and cnt2 == cnt == 8
	for d in (acc, Wd, tall, foreign):
		d.close()
	other.close()


## ---- 3. exact end to end, Lanczos ------------------------------------------------------------------------------------------
def orthogonal_probes(n, seed):
	"""sqrt(n) Q: (1/n) sum_i v_i v_i^T = I exactly, so the Hutchinson sums are the exact trace and the exact f'(A)."""
	Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
	return np.asfortranarray(np.sqrt(n) * Q)


def propagated_bar(E, V, Y, rows, cols, n, batch, symmetric=True):
	"""(1/n) sum_i E[r, i] |V[c, i]| (its symmetric part) - what an elementwise error E on the columns of Y = f'(A) V leaves on
	the gradient - plus the kernel's own bar over the batches of `batch` columns, every batch an update with beta = 1."""
	aV = np.abs(V)
	out = np.sum(E[rows, :] * aV[cols, :], axis=1)
	if symmetric:
		out = 0.5 * (out + np.sum(E[cols, :] * aV[rows, :], axis=1))
	out = out / n
	old = np.zeros(len(rows), dtype=np.longdouble)
	for c0 in range(0, V.shape[1], batch):
		Yb, Vb = Y[:, c0 : c0 + batch], V[:, c0 : c0 + batch]
		out = out + R.bar(rows, cols, Yb, Vb, 1.0 / n, 1.0, old, symmetric)
		old = R.vals_ld(rows, cols, Yb, Vb, 1.0 / n, 1.0, old, symmetric)
	return out


@pytest.mark.parametrize("fun,kw", [("log", {}), ("exp", {"t": -0.3})])
def test_exact_gradient_lanczos(fun, kw):
	from primate_amd.grad import trace_grad
	from primate_amd.operators import MatrixFunction

	rng = np.random.default_rng(1234)
	n = 60
	B = rng.standard_normal((n, n))
	A = B @ B.T / n + 0.5 * np.eye(n)
	ew, ev = np.linalg.eigh(A)
	t = kw.get("t", 1.0)
	f, fa, scale = (np.log, (lambda x: 1.0 / x), 1.0) if fun == "log" else ((lambda x: np.exp(t * x)), (lambda x: np.exp(t * x)), t)
	P = sp.csr_matrix(np.ones((n, n)))
	rows, cols = R.pattern_rows_cols(P)
	V = orthogonal_probes(n, 99)
	M = MatrixFunction(A, fun, deg=n, orth=n, **kw)
	est, grad, info = trace_grad(M, probes=V, batch=25, pattern=P)
	assert info["count"] == n and info["acc_count"] == n and info["quad"].shape == (n,)
	want_est = float(np.sum(f(ew)))
	print(f"{fun}: est err {abs(est - want_est):.3e}, bar {1e-8 * np.sum(np.abs(f(ew))):.3e}")
	assert abs(est - want_est) <= 1e-8 * np.sum(np.abs(f(ew)))  # (mean_i v_i^T f(A) v_i = sum_i q_i^T f(A) q_i = tr f(A))
	FA = (ev * fa(ew)) @ ev.T  # what the library's action evaluates; f'(A) = scale * FA
	Y = FA @ V
	E = abs(scale) * (1e-8 * np.abs(Y) + 1e-9)
	bar = propagated_bar(E, V, scale * Y, rows, cols, n, 25)
	want = (scale * 0.5 * (FA + FA.T))[rows, cols]
	err = np.abs(grad - want)
	print(f"{fun}: grad max err {err.max():.3e}, max err/bar {np.max(err / bar):.3e}")
	assert np.all(err <= bar), f"{fun}: max err/bar {np.max(err / bar):.3f}"


## ---- 4. exact end to end, Chebyshev ---------------------------------------------------------------------------------------
def test_exact_gradient_chebyshev():
	from _cheb_action_ref import action_bar, action_recurrence, action_recurrence_ld, coefficient_weight
	from primate_amd.chebyshev import ChebyshevFunction, chebyshev_coefficients, spectral_bounds
	from primate_amd.grad import trace_grad

	A = R.grid_pattern()
	n = A.shape[0]
	rows, cols = R.pattern_rows_cols(A)
	bounds = spectral_bounds(A, "gershgorin")
	f, df = (lambda x: x**3), (lambda x: 3.0 * x**2)
	V = orthogonal_probes(n, 98)
	M = ChebyshevFunction(A, f, deg=4, bounds=bounds)
	est, grad, info = trace_grad(M, probes=V, batch=64, dfun=df)
	M.close()
	assert info["acc_count"] == n
	eps = np.finfo(np.float64).eps
	Ad = A.toarray()
	coef = chebyshev_coefficients(f, 5, bounds)
	bar_est = 8.0 * eps * coefficient_weight(coef) * n  # per probe eps sum_k (k + 1) |c_k| ||v||^2, ||v||^2 = n; est is their mean
	want_est = np.trace(Ad @ Ad @ Ad)
	print(f"cheb: est err {abs(est - want_est):.3e} bar {bar_est:.3e}")
	assert abs(est - want_est) <= bar_est
	dcoef = chebyshev_coefficients(df, 5, bounds)
	Y_ld = action_recurrence_ld(A, V, dcoef, bounds)
	Y_F = action_recurrence(A, V, dcoef, bounds, np.float64)
	col_bar, _, _ = action_bar(Y_ld, Y_F, V, dcoef, eps)
	E = np.broadcast_to(col_bar[None, :], (n, n))  # a column's 2-norm bar bounds each of its entries
	bar = propagated_bar(E, V, Y_ld.astype(np.float64), rows, cols, n, 64)
	want = (3.0 * (Ad @ Ad))[rows, cols]
	err = np.abs(grad - want)
	print(f"cheb: grad max err {err.max():.3e}, max err/bar {np.max(err / bar):.3e}")
	assert np.all(err <= bar), f"max err/bar {np.max(err / bar):.3f}"


## ---- 5. statistics -------------------------------------------------------------------------------------------------------
STAT_SEED = 2024


def test_gradient_statistics():
	"""log det of (grid Laplacian + I): the gradient estimate is within 5 standard errors of inv(A) on the pattern for at least
	99 % of the entries; the standard error from the per-entry variance (A^-1)_rr (A^-1)_cc + (A^-1)_rc^2, halved off the diagonal
	by the symmetric part, over `count`. (NumPy's own estimator from the same probes - the draw of random.isotropic for this seed -
	meets the condition: 100 % of the entries, largest deviation 4.4 standard errors.)"""
	from primate_amd.grad import trace_grad
	from primate_amd.operators import MatrixFunction

	A = (R.grid_pattern() + sp.identity(143)).tocsr()
	A.sort_indices()
	rows, cols = R.pattern_rows_cols(A)
	count = 512
	M = MatrixFunction(A, "log", deg=40)
	est, grad, info = trace_grad(M, pdf="rademacher", count=count, batch=128, seed=STAT_SEED)
	Ai = np.linalg.inv(A.toarray())
	var = Ai[rows, rows] * Ai[cols, cols] + Ai[rows, cols] ** 2
	var = np.where(rows == cols, var, 0.5 * var)
	z = np.abs(grad - Ai[rows, cols]) / np.sqrt(var / count)
	share = float(np.mean(z <= 5.0))
	print(f"statistics: {100 * share:.2f} % within 5 s.e., max {z.max():.2f} s.e.")
	assert share >= 0.99
	logdet = np.linalg.slogdet(A.toarray())[1]
	assert abs(est - logdet) <= 5.0 * np.std(info["quad"], ddof=1) / np.sqrt(count)


## ---- 6. torch ------------------------------------------------------------------------------------------------------------
def test_torch_backward_matches_trace_grad():
	import torch

	from primate_amd.autograd import trace_fun
	from primate_amd.grad import trace_grad
	from primate_amd.operators import MatrixFunction

	A = (R.grid_pattern() + sp.identity(143)).tocsr()
	A.sort_indices()
	crow, col = torch.from_numpy(A.indptr.astype(np.int64)).cuda(), torch.from_numpy(A.indices.astype(np.int64)).cuda()
	values = torch.from_numpy(A.data.copy()).cuda().requires_grad_(True)
	make = lambda: torch.sparse_csr_tensor(crow, col, values, size=A.shape)  # noqa: E731  (a backward frees the graph of the tensor it went through)
	loss = trace_fun(make(), "log", deg=20, count=64, seed=5)
	loss.backward()
	assert values.grad is not None and values.grad.device == values.device and values.grad.dtype == torch.float64
	Td = torch.sparse_csr_tensor(crow, col, values.detach().clone(), size=A.shape)
	est, grad, _ = trace_grad(MatrixFunction(Td, "log", deg=20), pdf="device:rademacher", count=64, seed=5, pattern=Td)
	assert np.array_equal(values.grad.cpu().numpy(), grad), "backward must leave trace_grad's gradient, bit for bit"
	assert loss.device == values.device and float(loss.detach()) == est
	values.grad = None
	(2 * trace_fun(make(), "log", deg=20, count=64, seed=5)).backward()
	assert np.array_equal(values.grad.cpu().numpy(), 2.0 * grad)
	## the Chebyshev route, through the same wrapper
	values.grad = None
	trace_fun(make(), "log", deg=30, count=64, seed=5, method="chebyshev", bounds=(0.5, 9.5)).backward()  # (the spectrum lies in (1, 9))
	Ai = np.linalg.inv(A.toarray())
	rows, cols = R.pattern_rows_cols(A)
	assert np.max(np.abs(values.grad.cpu().numpy() - Ai[rows, cols])) < 0.5  # (a sampled estimate: the statistics are item 5's)


## ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
	from scipy.sparse.linalg import aslinearoperator

	from primate_amd.chebyshev import ChebyshevFunction
	from primate_amd.grad import trace_grad
	from primate_amd.operators import MatrixFunction

	A = (R.grid_pattern() + sp.identity(143)).tocsr()
	with pytest.raises(ValueError, match="Chebyshev"):
		trace_grad(MatrixFunction(A, "numrank", deg=10), count=8)
	Mc = ChebyshevFunction(A, "log", deg=10)
	with pytest.raises(ValueError, match="device:sphere"):
		trace_grad(Mc, pdf="device:sphere", count=8)
	with pytest.raises(ValueError, match="dfun"):
		trace_grad(ChebyshevFunction(A, "abs", deg=10), count=8)
	Mc.close()
	with pytest.raises(ValueError, match="pattern= is required"):
		trace_grad(MatrixFunction(aslinearoperator(A), "log", deg=10), count=8)
	with pytest.raises(ValueError, match="fp64"):
		trace_grad(MatrixFunction(A.astype(np.float32), "log", deg=10, dtype=np.float32), count=8)
	## identity: the exact answer, no sampling
	est, grad, info = trace_grad(MatrixFunction(A, "identity", deg=10), count=8, batch=8, seed=1)
	rows, cols = R.pattern_rows_cols(A)
	assert np.array_equal(grad, (rows == cols).astype(np.float64)) and info["acc_count"] == 0
