"""Gradients of the kernel operator with respect to the points, without a device: the long-double model of
`_kernelpointgrad_ref` against central differences of sum C (.) A(X) through centring; the vanishing column sums; the float64 emulation of
the difference form inside the bar for every GPU case, and three faults far outside it; the schedule through its debug entry; the raw
entries on NULL handles. (scripts/kernelpointgrad_check.cpp runs the host part of csrc/slq_kernelpointgrad.hpp under the host
sanitizers as a program of its own.)"""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _kernelcross_ref as XR
import _kernelgrad_ref as G
import _kernelop_ref as R
import _kernelpointgrad_ref as PG
from primate_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
LD = np.longdouble
NEW_SYMBOLS = ("slq_kernel_pointgrad_create", "slq_kernel_pointgrad_create_cross", "slq_kernel_pointgrad_update", "slq_kernel_pointgrad_get",
			   "slq_kernel_pointgrad_reset", "slq_kernel_pointgrad_destroy", "slq_kernel_precond_trace_pointgrad",
			   "slq_debug_kernel_pointgrad_schedule")  # fmt: skip


def test_symbols_are_declared_exported_and_bound():
	hdr = (ROOT / "include" / "slq.h").read_text()
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint {s}\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"
	assert L.slq_version() == 100


## ---- the model against central differences ---------------------------------------------------------------------------------------
def _bilinear(X, name, ls, s, noise, Z, W) -> LD:
	"""sum C (.) A(X) in long double, A the dense matrix on the rounded, CENTRED z of `_kernelop_ref`."""
	z = R.scaled_points(X, ls, np.float64)
	A = LD(s) * R.phi(name, R.r2_exact(z))
	A[np.diag_indices_from(A)] += LD(noise)
	return np.sum((Z.astype(LD) @ W.astype(LD).T) * A)


def _bilinear_cross(X, Xn, name, ls, s, U, W) -> LD:
	z, zn = R.scaled_points(X, ls, np.float64), XR.scaled_new_points(X, Xn, ls, np.float64)
	return np.sum((U.astype(LD) @ W.astype(LD).T) * (LD(s) * R.phi(name, XR.r2_cross(zn, z))))


def _central(f, x: float, h: float):
	"""(derivative, its own error): the central difference at step h, and the h^2 remainder estimated from the step 2 h -
	|D(h) - D(2h)| / 3 - plus the rounding of the differenced values, eps |f| / h (`test_kernelgrad_cpu`)."""
	f1, f2 = (f(x + h) - f(x - h)) / (2 * h), (f(x + 2 * h) - f(x - 2 * h)) / (4 * h)
	return f1, abs(f1 - f2) / 3 + 4 * R.eps_of(np.float64) * abs(f(x)) / h


@pytest.mark.parametrize("per_dim", [False, True], ids=["scalar", "perdim"])
@pytest.mark.parametrize("name", R.PROFILES)
@pytest.mark.parametrize("d", [1, 3, 17])
def test_the_model_is_the_derivative_of_the_dense_matrix(name, d, per_dim):
	"""Moving one coordinate of one point moves the centre too, and the rounding of z makes sum C (.) A(X) a staircase at the scale
	eps: the differences see that as noise eps |f| / h, part of their own error. The tolerance is that error, with a factor 4 on the
	remainder estimate; the column sums vanish (a translation changes nothing) up to the bar's own sum."""
	n, m = 40, 3
	X = R.points(n, d, seed=d)
	base = 0.4 * np.sqrt(d)
	ls = base * (1.0 + np.arange(d) / d) if per_dim else base
	s, noise = 1.3, 0.1
	rng = np.random.default_rng(d)
	Z, W = rng.standard_normal((n, m)), rng.standard_normal((n, m))
	P, bar = PG.model(R.scaled_points(X, ls, np.float64), name, ls, s, Z, W)
	h = 1e-4
	for a, k in sorted({(0, 0), (n // 2, d // 2), (n - 1, d - 1)}):
		def f(v, a=a, k=k):
			X2 = X.copy()
			X2[a, k] = v
			return _bilinear(X2, name, ls, s, noise, Z, W)
		fd, err = _central(f, X[a, k], h)
		print(f"{name} d={d} x[{a},{k}]: model {float(P[a, k]):.12e} differences {float(fd):.12e} +- {float(err):.2e}")
		assert abs(fd - P[a, k]) <= 4 * err + 1e-18, (name, d, a, k, float(fd - P[a, k]), float(err))
	assert np.all(np.abs(P.sum(axis=0)) <= bar.sum(axis=0) + n * G.EPS * np.abs(P).sum(axis=0)), "the column sums of P must vanish"
	## the cross form: the new points move, the training centre does not
	mnew, b = 7, 2
	Xn = R.points(mnew, d, seed=90 + d)
	U, Wc = rng.standard_normal((mnew, b)), rng.standard_normal((n, b))
	Rm, _ = PG.model(R.scaled_points(X, ls, np.float64), name, ls, s, U, Wc, znew=XR.scaled_new_points(X, Xn, ls, np.float64))
	for a, k in sorted({(0, 0), (mnew - 1, d - 1)}):
		def f(v, a=a, k=k):
			X2 = Xn.copy()
			X2[a, k] = v
			return _bilinear_cross(X, X2, name, ls, s, U, Wc)
		fd, err = _central(f, Xn[a, k], h)
		assert abs(fd - Rm[a, k]) <= 4 * err + 1e-18, (name, d, "cross", a, k, float(fd - Rm[a, k]), float(err))


def test_the_training_form_is_the_sum_of_the_two_one_sided_forms():
	n, d, m = 33, 3, 4
	X = R.points(n, d, seed=1)
	z = R.scaled_points(X, 0.5, np.float64)
	rng = np.random.default_rng(1)
	Z, W = rng.standard_normal((n, m)), rng.standard_normal((n, m))
	P, bar = PG.model(z, "matern52", 0.5, 1.3, Z, W)
	a, _ = PG.model(z, "matern52", 0.5, 1.3, Z, W, one_sided=True)
	b, _ = PG.model(z, "matern52", 0.5, 1.3, W, Z, one_sided=True)
	assert PG.worst((a + b).astype(np.float64), P, bar) <= 1.0


## ---- the condition, and an emulation inside the bar, for every GPU case ------------------------------------------------------------
@pytest.mark.parametrize("case", G.GPU_CASES, ids=[G.case_id(c) for c in G.GPU_CASES])
def test_condition_and_emulation_for_every_gpu_case(case):
	(X, ls, s, noise, Z, W), z, P, bar = PG.case_model(case)
	ratio = PG.check_condition(P, bar)
	w = PG.worst(PG.emulate(z, case[3], ls, s, Z, W), P, bar)
	print(f"{G.case_id(case)}: bar / max |P| = {ratio:.2e}, emulation / bar = {w:.4f}")
	assert np.all(np.isfinite(P.astype(np.float64))) and w <= 0.5, (case, w)


@pytest.mark.parametrize("case", PG.CROSS_CASES, ids=[PG.cross_id(c) for c in PG.CROSS_CASES])
def test_condition_and_emulation_for_every_cross_case(case):
	(X, Xn, ls, s, noise, U, W, copies), z, zn, P, bar = PG.cross_model(case)
	ratio = PG.check_condition(P, bar)
	w = PG.worst(PG.emulate(z, case[4], ls, s, U, W, znew=zn), P, bar)
	print(f"{PG.cross_id(case)}: bar / max |R| = {ratio:.2e}, emulation / bar = {w:.4f}")
	assert np.all(np.isfinite(P.astype(np.float64))) and w <= 0.5, (case, w)
	assert all(np.array_equal(zn[a], z[a % case[1]]) for a in copies), "the copies must be bitwise copies after scaling too"


def test_the_expanded_form_fails_where_the_difference_form_passes():
	"""Duplicate rows at an offset of 1e4 under matern12: chi is huge at a near-zero r2 and multiplies a cancelled difference."""
	case = (257, 3, 16, "matern12", False, 1e4, True)
	(X, ls, s, noise, Z, W), z, P, bar = PG.case_model(case)
	good, bad = PG.worst(PG.emulate(z, "matern12", ls, s, Z, W), P, bar), PG.worst(PG.emulate(z, "matern12", ls, s, Z, W, expanded=True), P, bar)
	print(f"difference form {good:.4f} bars, expanded form {bad:.3e} bars")
	assert good <= 0.5 and bad > 1e2


def test_the_bar_notices_a_dropped_remainder_tile():
	case = (257, 8, 65, "rbf", False, 0.0, False)
	(X, ls, s, noise, Z, W), z, P, bar = PG.case_model(case)
	assert PG.worst(PG.emulate(z, "rbf", ls, s, Z, W, jmax=256), P, bar) > 1e3


def test_the_bar_notices_a_wrong_sign_of_one_difference():
	case = (257, 8, 65, "rbf", False, 0.0, False)
	(X, ls, s, noise, Z, W), z, P, bar = PG.case_model(case)
	bad, _ = PG.model(z, "rbf", ls, s, Z, W, flip=(40, 41, 2))
	assert PG.worst(bad.astype(np.float64), P, bar) > 1e3
	assert np.array_equal(bad[:, 0], P[:, 0]) and np.array_equal(bad[41], P[41])  # (one element only)


def test_the_bar_notices_an_omitted_transposed_term():
	case = (257, 8, 65, "rbf", False, 0.0, False)
	(X, ls, s, noise, Z, W), z, P, bar = PG.case_model(case)
	bad, _ = PG.model(z, "rbf", ls, s, Z, W, one_sided=True)
	assert PG.worst(bad.astype(np.float64), P, bar) > 1e3


## ---- the schedule ------------------------------------------------------------------------------------------------------------------
SIZES = [1, 15, 16, 17, 127, 128, 129, 1000, 20000]


@pytest.mark.parametrize("nrows", SIZES)
def test_schedule_partitions_rows_and_points(nrows):
	from primate_amd.engine import kernel_pointgrad_schedule

	for nsum in SIZES:
		for cus in (256, 8, 1):
			S = kernel_pointgrad_schedule(nrows, nsum, cus)
			assert S["rows"] == 128 and S["nrb"] == -(-nrows // 128) and S["chunk_cols"] == 64
			owners = np.zeros(nrows, dtype=int)
			for b in range(S["nrb"]):
				owners[b * S["rows"] : min(nrows, (b + 1) * S["rows"])] += 1
			assert np.all(owners == 1)
			b, tps = S["begin"], S["tiles_per_slab"]
			assert 1 <= S["slabs"] <= 64 and b[0] == 0 and b[-1] == nsum and all(x < y for x, y in zip(b, b[1:]))
			assert all(x % 16 == 0 for x in b[:-1]) and all(v == -1 for v in S["rest"]) and S["slabs"] <= -(-nsum // 16)
			owners = np.zeros(nsum, dtype=int)
			for x, y in zip(b, b[1:]):
				owners[x:y] += 1
			assert np.all(owners == 1)
			## what the kernel computes from its slab index and tiles_per_slab is the schedule's range
			ntiles = -(-nsum // 16)
			for zi in range(S["slabs"]):
				first = min(ntiles, zi * tps)
				last = min(ntiles, first + tps)
				assert first * 16 == b[zi] and min(nsum, last * 16) == b[zi + 1], (nrows, nsum, cus, zi)
			assert min(ntiles, S["slabs"] * tps) == ntiles
			## the addition limit the bar assumes: a lane's run over its slab's padded points, the slabs, the fold, the second pass' fold
			assert max(y - x for x, y in zip(b, b[1:])) + 15 + (S["slabs"] - 1) + 2 <= nsum + 80


def test_schedule_entry_checks_its_arguments():
	L = _capi.lib()
	out = (C.c_int64 * 70)()
	assert L.slq_debug_kernel_pointgrad_schedule(100, 100, 256, out, 69) == _capi.SLQ_EINVAL
	assert L.slq_debug_kernel_pointgrad_schedule(100, 100, 256, None, 70) == _capi.SLQ_EINVAL
	for args in ((0, 64, 256), (100, 0, 256), (100, 64, 0), (1 << 31, 64, 256), (64, 1 << 31, 256)):
		assert L.slq_debug_kernel_pointgrad_schedule(*args, out, 70) == _capi.SLQ_EINVAL, args
	assert L.slq_debug_kernel_pointgrad_schedule(100, 100, 256, out, 70) == _capi.SLQ_OK


def test_raw_entries_refuse_null_handles_without_a_device():
	L = _capi.lib()
	h = C.c_void_p()
	cnt = C.c_int64()
	vals = np.zeros(3)
	assert L.slq_kernel_pointgrad_create(None, None, C.byref(h)) == _capi.SLQ_EINVAL
	assert L.slq_kernel_pointgrad_create(None, None, None) == _capi.SLQ_EINVAL
	assert L.slq_kernel_pointgrad_create_cross(None, None, C.byref(h)) == _capi.SLQ_EINVAL
	assert L.slq_kernel_pointgrad_update(None, None, 0, None, 0, 1, 1.0, 1.0) == _capi.SLQ_EINVAL
	assert L.slq_kernel_pointgrad_get(None, _capi.ptr(vals), 3, C.byref(cnt)) == _capi.SLQ_EINVAL
	assert L.slq_kernel_pointgrad_reset(None) == _capi.SLQ_EINVAL
	assert L.slq_kernel_pointgrad_destroy(None) == _capi.SLQ_OK
	assert L.slq_kernel_precond_trace_pointgrad(None, None, 1.0, 0.0) == _capi.SLQ_EINVAL


def test_the_chebyshev_route_and_other_operators_are_refused_before_the_library():
	from primate_amd.grad import kernel_point_grad

	with pytest.raises(ValueError, match="KernelOperator"):
		kernel_point_grad(np.eye(3), np.ones(3))
