"""The matrix-free kernel operator, what needs no GPU: the host products of KernelOperator against closed forms,
the model of the GPU tests and its bar against NumPy emulations of the device evaluation, every refusal raised before the library
is touched, the C-ABI symbols, and the host schedule of the product kernel (slq_debug_kernel_schedule: rows and j slabs covered
exactly once)."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _kernelop_ref as R
from primate_amd import _capi
from primate_amd.operators import KernelOperator, MatrixFunction

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_kernel_create", "slq_kernel_create_device", "slq_kernel_set_parameters", "slq_kernel_get_parameters",
			   "slq_debug_kernel_points", "slq_debug_kernel_schedule")  # fmt: skip

## five points on a line and in the plane whose distances are known without arithmetic
X5 = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 1.0], [6.0, 8.0], [3.0, 4.0]])
D5 = np.array([[0, 5, 1, 10, 5], [5, 0, np.sqrt(18), 5, 0], [1, np.sqrt(18), 0, np.sqrt(85), np.sqrt(18)], [10, 5, np.sqrt(85), 0, 5], [5, 0, np.sqrt(18), 5, 0]])


def closed_form(name, r):
	if name == "rbf":
		return np.exp(-r * r / 2)
	if name == "matern12":
		return np.exp(-r)
	if name == "matern32":
		return (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r)
	return (1 + np.sqrt(5) * r + 5 * r * r / 3) * np.exp(-np.sqrt(5) * r)


def test_symbols_are_declared_exported_and_bound():
	hdr = (ROOT / "include" / "slq.h").read_text()
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint {s}\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"
	assert "OP_KERNEL = 5" in (ROOT / "primate_amd" / "csrc" / "slq_plan_shape.hpp").read_text()


@pytest.mark.parametrize("name", R.PROFILES)
def test_host_products_equal_the_closed_form(name):
	ell, s, noise = 2.0, 1.5, 0.25
	K = KernelOperator(X5, name, lengthscale=ell, outputscale=s, noise=noise)
	assert K.shape == (5, 5) and K.dtype == np.float64 and K._slq_kind == "kernel"
	want = s * closed_form(name, D5 / ell) + noise * np.eye(5)
	got = K @ np.eye(5)
	assert np.max(np.abs(got - want)) < 1e-13
	v = np.arange(1.0, 6.0)
	assert np.max(np.abs(K @ v - want @ v)) < 1e-12
	## symmetric; the diagonal is s + sigma2; duplicate points (1 and 4) give r2 = 0: the full value off the diagonal
	assert np.array_equal(got, got.T)
	assert np.array_equal(np.diag(got), np.full(5, s + noise))
	assert got[1, 4] == s and got[4, 1] == s
	## a per-dimension lengthscale
	Kd = KernelOperator(X5, name, lengthscale=[3.0, 4.0])
	r = np.sqrt((((X5[:, None, :] - X5[None, :, :]) / np.array([3.0, 4.0])) ** 2).sum(-1))
	assert np.max(np.abs(Kd @ np.eye(5) - closed_form(name, r))) < 1e-13


def test_set_parameters_changes_the_products():
	K = KernelOperator(X5, "rbf", lengthscale=2.0)
	a = K @ np.eye(5)
	K.set_parameters(lengthscale=1.0, outputscale=3.0, noise=0.5)
	b = K @ np.eye(5)
	assert np.max(np.abs(b - (3.0 * closed_form("rbf", D5) + 0.5 * np.eye(5)))) < 1e-13 and not np.allclose(a, b)
	K.set_parameters(noise=0.0)  # (None: unchanged)
	assert np.max(np.abs(K @ np.eye(5) - 3.0 * closed_form("rbf", D5))) < 1e-13
	assert np.array_equal(K.lengthscale, [1.0]) and K.outputscale == 3.0


def test_scaled_points_are_the_models():
	for dt in (np.float32, np.float64):
		X = R.points(130, 3, seed=1, offset=1e4, dtype=dt)
		K = KernelOperator(X, "matern32", lengthscale=[0.5, 1.0, 2.0], dtype=dt)
		z = K.scaled_points()
		assert z.dtype == dt and np.array_equal(z, R.scaled_points(X, [0.5, 1.0, 2.0], dt))
		assert np.max(np.abs(z.astype(np.float64).mean(axis=0))) < 1e-4 * (1 if dt == np.float64 else 100)


def test_every_refusal():
	bad = X5.copy()
	bad[3, 1] = np.nan
	with pytest.raises(ValueError, match=r"point 3, coordinate 1"):
		KernelOperator(bad)
	bad[3, 1] = np.inf
	bad[2, 0] = -np.inf
	with pytest.raises(ValueError, match=r"point 2, coordinate 0"):  # (the first bad value)
		KernelOperator(bad)
	for ell in (0.0, -1.0, np.nan, [1.0, 0.0]):
		with pytest.raises(ValueError, match="lengthscale"):
			KernelOperator(X5, lengthscale=ell)
	with pytest.raises(ValueError, match=r"lengthscale\[1\]"):
		KernelOperator(X5, lengthscale=[1.0, -2.0])
	with pytest.raises(ValueError, match="3 lengthscales"):
		KernelOperator(X5, lengthscale=[1.0, 2.0, 3.0])
	with pytest.raises(ValueError, match="d = 65"):
		KernelOperator(np.zeros((4, 65)))
	with pytest.raises(ValueError, match="unknown profile"):
		KernelOperator(X5, "periodic")
	with pytest.raises(ValueError, match="outputscale"):
		KernelOperator(X5, outputscale=0.0)
	with pytest.raises(ValueError, match="noise"):
		KernelOperator(X5, noise=-1e-3)
	with pytest.raises(ValueError, match="Only 32- or 64-bit"):
		KernelOperator(X5, dtype=np.float16)
	K = KernelOperator(X5)
	with pytest.raises(ValueError, match="dimension mismatch"):  # non-square use
		K @ np.ones((4, 2))
	with pytest.raises(ValueError, match="dimension mismatch"):
		K @ np.ones(6)
	with pytest.raises(ValueError, match="lengthscale"):
		K.set_parameters(lengthscale=-1.0)
	assert np.array_equal(K.lengthscale, [1.0])  # (a refused change changes nothing)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", R.CPU_CASES)
def test_the_bar_holds_an_emulation_and_stays_small(case, dtype):
	"""An fp32 / fp64 NumPy emulation of the norms-plus-dot evaluation stays within 0.10 of the bar, and the bar within 3e-4 (fp32) /
	1e-11 (fp64) of max |Y|: a wrong tile, a dropped remainder or a swapped operand is off by orders of magnitude.
	One cell of the table is looser, and says so: matern12 on the line (d = 1). exp(-sqrt(r2)) has a cusp at r2 = 0, 257 points on a
	line have near neighbours, and there the error of r2 goes through the square root. Over the seeds 0..15 of these inputs the
	emulation measured 0.05 .. 0.26 of the bar in fp32 (0.05 .. 0.12 in fp64) and the bar 2e-4 .. 8e-4 of max |Y| (1e-12 .. 6e-10 in
	fp64, the last with two points 1e-7 apart), so for that cell the test asks what a bound promises - the emulation inside the bar,
	with a factor 2 to spare - and the condition of the GPU tests (1e-3 / 1e-10), not the tighter figures of the other fifteen cells."""
	n, d, ell = case
	X = R.points(n, d, seed=d, dtype=dtype)
	z = R.scaled_points(X, ell, dtype)
	W = R.probes(n, 5, seed=d, dtype=dtype)
	for name in R.PROFILES:
		cusp = name == "matern12" and d == 1
		Y, bar = R.model(z, name, 1.3, 0.1, W)
		ratio = R.check_condition(Y, bar, dtype)
		if not cusp:
			assert ratio <= (3e-4 if dtype == np.float32 else 1e-11), (name, ratio)
		w = R.worst(R.emulate(z, name, 1.3, 0.1, W), Y, bar)
		assert w <= (0.5 if cusp else 0.10), (name, w)
		## ... and the KernelOperator's own host product (float64 arithmetic on the same rounded z) is inside it too
		K = KernelOperator(X, name, lengthscale=ell, outputscale=1.3, noise=0.1, dtype=dtype)
		assert R.worst(K @ W, Y, bar) <= 1.0, name


def test_the_bar_notices_a_dropped_tile():
	n, d, ell = R.CPU_CASES[1]
	z = R.scaled_points(R.points(n, d), ell, np.float64)
	W = R.probes(n, 3)
	Y, bar = R.model(z, "rbf", 1.0, 0.0, W)
	Wcut = W.copy()
	Wcut[256:] = 0.0  # the remainder tile dropped
	assert R.worst(R.emulate(z, "rbf", 1.0, 0.0, Wcut), Y, bar) > 1e6


## ---- the schedule -------------------------------------------------------------------------------------------------
def schedule(n, pw, npan, cus=256):
	out = (C.c_int64 * 22)()
	rc = _capi.lib().slq_debug_kernel_schedule(n, pw, npan, cus, out, 22)
	assert rc == _capi.SLQ_OK, _capi.lib().slq_last_error()
	v = list(out)
	return dict(rows=v[0], nrb=v[1], cb=v[2], chunks=v[3], slabs=v[4], begin=v[5 : 5 + v[4] + 1], rest=v[5 + v[4] + 1 :])


PANELS = [(16, 1), (32, 1), (64, 1), (128, 1), (128, 2), (256, 1), (256, 2), (128, 3), (16, 3)]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257, 1000, 20000])
def test_schedule_covers_every_row_and_column_once(n):
	for pw, npan in PANELS:
		for cus in (256, 8, 1):
			S = schedule(n, pw, npan, cus)
			## the row blocks are a partition of [0, n)
			assert S["rows"] == 128 and S["nrb"] == -(-n // 128)
			owners = np.zeros(n, dtype=int)
			for b in range(S["nrb"]):
				owners[b * S["rows"] : min(n, (b + 1) * S["rows"])] += 1
			assert np.all(owners == 1)
			## the column chunks cover the NP * PW columns once, with tiles the kernels are instantiated for
			assert S["cb"] in (1, 2, 4, 8, 16) and (S["chunks"] - 1) * 16 * S["cb"] < pw * npan <= S["chunks"] * 16 * S["cb"]
			## the slabs partition [0, n) in order, on tile boundaries, none empty
			b = S["begin"]
			assert 1 <= S["slabs"] <= 16 and b[0] == 0 and b[-1] == n and all(x < y for x, y in zip(b, b[1:]))
			assert all(x % 16 == 0 for x in b[:-1]) and all(v == -1 for v in S["rest"])
			assert S["slabs"] <= -(-n // 16)
	## an operator whose row blocks fill the chip many times over needs no split; a small one is split
	assert schedule(262144, 128, 1)["slabs"] == 1 and schedule(1000, 128, 1)["slabs"] > 1 and schedule(1, 16, 1)["slabs"] == 1


def test_schedule_entry_checks_its_arguments():
	L = _capi.lib()
	out = (C.c_int64 * 22)()
	assert L.slq_debug_kernel_schedule(100, 64, 1, 256, out, 21) == _capi.SLQ_EINVAL
	assert L.slq_debug_kernel_schedule(100, 64, 1, 256, None, 22) == _capi.SLQ_EINVAL
	for args in ((0, 64, 1, 256), (100, 48, 1, 256), (100, 8, 1, 256), (100, 64, 0, 256), (100, 64, 1, 0)):
		assert L.slq_debug_kernel_schedule(*args, out, 22) == _capi.SLQ_EINVAL, args


def test_raw_entries_refuse_null_handles_without_a_device():
	L = _capi.lib()
	ls = np.ones(1)
	h = C.c_void_p()
	assert L.slq_kernel_create(None, _capi.SLQ_F64, 5, 2, _capi.ptr(X5), 2, 0, _capi.ptr(ls), 1, 1.0, 0.0, C.byref(h)) == _capi.SLQ_EINVAL
	assert L.slq_kernel_set_parameters(None, _capi.ptr(ls), 1, 1.0, 0.0) == _capi.SLQ_EINVAL
	assert L.slq_kernel_get_parameters(None, None, None, None, 0, None, None) == _capi.SLQ_EINVAL
	assert L.slq_debug_kernel_points(None, None, None, None) == _capi.SLQ_EINVAL


def test_gradients_refuse_the_kind():
	from primate_amd import autograd, grad

	K = KernelOperator(X5, noise=0.1)
	M = MatrixFunction.__new__(MatrixFunction)  # (no device here: the refusal comes before anything is run)
	M._A, M.dtype, M.shape = K, np.dtype(np.float64), K.shape
	with pytest.raises(ValueError, match="hyperparameter gradients"):
		grad.trace_grad(M)
	with pytest.raises(ValueError, match="hyperparameter gradients"):
		autograd.trace_fun(K)
