"""The Toeplitz operator without a GPU: the five ABI symbols, the host ToeplitzOperator against the long-double model
of tests/_toeplitz_ref.py, from_kernel against KernelOperator on the grid, the validation messages, the pass structure at every size the
GPU test runs (slq_debug_toeplitz_plan), the host symbol transform against numpy.fft.fft (through scripts/toeplitz_check.cpp, built
here), the pass structure replayed on the host by the same program, and the conditions the error bar carries on the whole case list."""

import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _toeplitz_ref as R
from primate_amd import _capi
from primate_amd.operators import KernelOperator, Toeplitz, ToeplitzOperator

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_toeplitz_create", "slq_toeplitz_set_values", "slq_toeplitz_get_values", "slq_debug_toeplitz_plan", "slq_debug_toeplitz_symbol")


def test_symbols_are_declared_exported_bound_and_cited():
	hdr = (ROOT / "include" / "slq.h").read_text()
	doc = (ROOT / "INTEGRATION.md").read_text()
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint {s}\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"
		assert s in doc, f"{s} is not cited in INTEGRATION.md"
	assert L.slq_toeplitz_create(None, 1, 4, None, None, None) == _capi.SLQ_EINVAL
	assert L.slq_toeplitz_set_values(None, None, None, 0) == _capi.SLQ_EINVAL
	assert L.slq_toeplitz_get_values(None, None, None, 0, None) == _capi.SLQ_EINVAL
	assert L.slq_debug_toeplitz_plan(4, 1, 16, None, 0) == _capi.SLQ_EINVAL
	assert L.slq_debug_toeplitz_symbol(None, None) == _capi.SLQ_EINVAL


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "general"])
def test_host_operator_against_the_model(symmetric, dtype):
	"""The host _matmat / _matvec (NumPy FFTs in double on the rounded values) within the bar of the operator's dtype; the adjoint swaps c and r."""
	for n in (1, 3, 64, 513):
		c, r = R.values(n, symmetric, dtype)
		X = R.inputs(n, 5, dtype)
		T = ToeplitzOperator(c.astype(np.float64), r.astype(np.float64), dtype=dtype)
		assert T.symmetric == symmetric or n == 1
		assert T.dtype == np.dtype(dtype) and np.array_equal(T.c, c) and np.array_equal(T.r, r) and T._slq_kind == "toeplitz" and isinstance(T, Toeplitz)
		Y, bars = R.model(c, r, X), R.bar(c, r, X, dtype)
		half_ulp = R.LD(R.eps_of(dtype)) * np.sqrt(np.sum(Y * Y, axis=0))  # (the result is rounded to the dtype once more)
		assert np.all(np.sqrt(np.sum((T._matmat(X).astype(R.LD) - Y) ** 2, axis=0)) <= bars + half_ulp)
		assert np.all(np.abs((T @ X[:, 0]).astype(R.LD) - Y[:, 0]) <= bars[0] + half_ulp[0])
		Yt = R.model(r, c, X)
		assert np.all(np.sqrt(np.sum(((T.T @ X).astype(R.LD) - Yt) ** 2, axis=0)) <= bars + half_ulp)


def test_the_plain_toeplitz_stays_the_host_plugin():
	assert getattr(Toeplitz(np.ones(4)), "_slq_kind", None) is None


@pytest.mark.parametrize("name", ["rbf", "matern12", "matern32", "matern52"])
def test_from_kernel_is_the_kernel_operator_on_the_grid(name):
	n, h, ell, s, noise = 40, 0.37, 1.3, 2.5, 0.05
	T = ToeplitzOperator.from_kernel(name, n, h, lengthscale=ell, outputscale=s, noise=noise)
	K = KernelOperator(h * np.arange(n), name, lengthscale=ell, outputscale=s, noise=noise)
	A = K.rows(np.arange(n))
	assert T.symmetric
	assert np.max(np.abs(A[:, 0] - T.c)) <= 1e-13 * np.max(np.abs(A))
	from scipy.linalg import toeplitz

	assert np.max(np.abs(A - toeplitz(T.c))) <= 1e-13 * np.max(np.abs(A))


def test_validation_messages():
	c = 0.5 ** np.arange(20)
	for bad, val in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
		cb = c.copy()
		cb[7], cb[11] = bad, np.nan  # (the FIRST bad entry is named)
		with pytest.raises(ValueError, match=rf"c\[7\] = {re.escape(val)}"):
			ToeplitzOperator(cb)
		with pytest.raises(ValueError, match=rf"r\[7\] = {re.escape(val)}"):
			ToeplitzOperator(c, cb)
	with pytest.raises(ValueError, match="r has shape"):
		ToeplitzOperator(c, c[:-1])
	with pytest.raises(ValueError, match="at least 1"):
		ToeplitzOperator(np.zeros(0))
	with pytest.raises(ValueError, match="exceeds the supported maximum"):
		ToeplitzOperator(np.zeros(R.plan(1, np.float64)["max_n"] + 1))
	assert ToeplitzOperator.MAX_N == R.plan(1, np.float64)["max_n"] >= 1 << 20
	with pytest.raises(ValueError, match="32- or 64-bit"):
		ToeplitzOperator(c, dtype=np.float16)
	big = c.copy()
	big[2] = 1e300  # finite in float64, not in float32
	ToeplitzOperator(big)
	with pytest.raises(ValueError, match=r"c\[2\]"):
		ToeplitzOperator(big, dtype=np.float32)
	T = ToeplitzOperator(c)
	with pytest.raises(ValueError, match="21 entries, the operator n = 20"):
		T.set_values(np.ones(21))
	with pytest.raises(ValueError, match="symmetry"):
		T.set_values(c, 0.3 ** np.arange(20))
	assert np.array_equal(T.c, c) and T.symmetric  # (a refused change changes nothing)
	T.set_values(0.25 ** np.arange(20))
	assert T.c[1] == 0.25
	with pytest.raises(ValueError, match="unknown profile"):
		ToeplitzOperator.from_kernel("cubic", 5, 0.1)
	## r[0] is ignored
	r = c.copy()
	r[0] = 77.0
	assert ToeplitzOperator(c, r).symmetric
	## the library's own checks that need no device
	L = _capi.lib()
	out = (C.c_int64 * 10)()
	for n in (0, R.plan(1, np.float64)["max_n"] + 1):
		assert L.slq_debug_toeplitz_plan(n, 1, 16, out, 10) == _capi.SLQ_EINVAL
		assert f"n = {n}" in L.slq_last_error().decode()
	assert L.slq_debug_toeplitz_plan(8, 7, 16, out, 10) == _capi.SLQ_EINVAL
	assert L.slq_debug_toeplitz_plan(8, 1, 24, out, 10) == _capi.SLQ_EINVAL


def test_set_values_commits_the_host_state_last():
	"""A device operator that fails its set leaves the host object unchanged, and the device operators already changed are put back."""
	import weakref

	class Dev:
		_h = 1

		def __init__(self, fail):
			self.fail, self.calls = fail, []

		def set_toeplitz_values(self, c, r):
			if self.fail:
				raise RuntimeError("device set failed")
			self.calls.append(np.array(c))

	c0, c1 = 0.5 ** np.arange(8), 0.25 ** np.arange(8)
	T = ToeplitzOperator(c0)
	good, bad = Dev(False), Dev(True)
	T._device_ops = [weakref.ref(good), weakref.ref(bad)]
	with pytest.raises(RuntimeError, match="device set failed"):
		T.set_values(c1)
	assert np.array_equal(T.c, c0) and np.array_equal(T._symbol, ToeplitzOperator(c0)._symbol)
	assert len(good.calls) == 2 and np.array_equal(good.calls[0], c1) and np.array_equal(good.calls[1], c0)
	T._device_ops = [weakref.ref(good)]
	T.set_values(c1)
	assert np.array_equal(T.c, c1) and np.array_equal(good.calls[-1], c1)


def test_pass_structure_at_every_size():
	single_max, further = R.structure_sizes()
	assert R.plan(single_max, np.float64)["levels"] == 1 and R.plan(single_max + 1, np.float64)["levels"] == 2
	seen = set()
	for n in R.sizes() + (R.plan(1, np.float64)["max_n"],):
		for dtype, pws in ((np.float64, (16, 32, 64, 128)), (np.float32, (32, 64, 128, 256))):
			for pw in pws:
				p = R.plan(n, dtype, pw)
				assert p["L"] >= 2 * n and p["L"] < 4 * n and p["L"] & (p["L"] - 1) == 0
				assert int(np.prod(p["lengths"])) == p["L"] and all(m <= 1024 for m in p["lengths"])
				assert sum(m > 1 for m in p["lengths"]) == p["levels"] or p["L"] <= 2
				assert p["lds"] <= 160 * 1024
				assert p["cg"] * 2 * np.dtype(dtype).itemsize == 128
				assert p["launches"] == 2 * p["levels"] - 1
				assert p["ws"] == (0 if p["levels"] == 1 else p["L"] * pw * np.dtype(dtype).itemsize)
				if n in R.sizes():
					seen.add(p["levels"])
	## every structure the implementation has is hit by the GPU list, at the smallest L that uses it
	every = {R.plan(1 << k, np.float64)["levels"] for k in range(0, 23)}
	assert seen == every == {1, 2, 3}
	for lv, n in zip((2, 3), further):
		assert R.plan(n, np.float64)["levels"] == lv and R.plan(n - 1, np.float64)["levels"] == lv - 1 and n in R.sizes()


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
	cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
	exe = tmp_path_factory.mktemp("toeplitz") / "toeplitz_check"
	subprocess.run([cxx, "-O2", "-std=c++17", str(ROOT / "scripts" / "toeplitz_check.cpp"), "-o", str(exe)], check=True)
	return exe


def test_host_symbol_transform_against_numpy(check_program):
	"""toeplitz_host_fft / toeplitz_symbol of the HIP-free header against numpy.fft.fft in double, to 1e-13 |e|_1."""
	for n, pc, pr in ((1, 0.5, 0.5), (2, 0.5, 0.3), (3, 0.5, 0.3), (64, 0.5, 0.5), (513, 0.9, 0.3), (2049, 0.999, 0.99), (70000, 0.5, 0.3)):
		raw = subprocess.run([str(check_program), "symbol", str(n), repr(pc), repr(pr)], check=True, capture_output=True).stdout
		L = int(np.frombuffer(raw[:8], dtype=np.float64)[0])
		got = np.frombuffer(raw[8:], dtype=np.complex128)
		assert L == R.plan(n, np.float64)["L"] and got.size == L
		k = np.arange(n, dtype=np.float64)
		e = np.zeros(L)
		e[:n] = pc**k
		e[L - n + 1 :] = (pr**k)[:0:-1]
		assert np.max(np.abs(got - np.fft.fft(e))) <= 1e-13 * np.sum(np.abs(e))


def test_pass_structure_replayed_on_the_host(check_program):
	"""The tiles, index arithmetic and tables of the kernels, replayed by the host program in the operator's precision at every structure
	(it exits 1 when a column misses the bar, 2 when an index leaves its array), the five-kernel one included."""
	single_max, further = R.structure_sizes()
	for n in (1, 2, 3, 17, single_max, further[0], 5000) + further[1:]:
		for extra in ([], ["f32"]) if n <= 5000 else ([],):  # (the five-kernel structure in fp64: a few seconds)
			res = subprocess.run([str(check_program), "passes", str(n)] + extra, capture_output=True, text=True)
			assert res.returncode == 0, res.stdout + res.stderr


def test_the_bar_discriminates_on_the_whole_case_list():
	"""On every case the GPU test runs: the bar is <= 1e-3 (fp32) / 1e-11 (fp64) of the result, and the host path at the operator's dtype
	(scipy.fft, the same pairing) stays within HALF of it - a device transform gets about 3 x pocketfft's worst case and no more."""
	worst = {}
	for case in R.cases():
		n, b, symmetric, dtype = case
		c, r, X, Y, bars = R.case_data(*case)
		frac = R.check_condition(Y, bars, dtype)
		ratio = float(np.max(R.ratios(R.host_path(c, r, X, dtype), Y, bars)))
		assert ratio <= 0.5, f"{case}: the host path is at {ratio:.3f} of the bar"
		key = np.dtype(dtype).name
		worst[key] = max(worst.get(key, (0.0, 0.0)), (ratio, frac))
	print(f"[toeplitz] host path worst ratio / bar fraction: {worst}")


def test_the_bar_notices_a_wrong_symbol():
	"""c shifted by one place, or r taken for c, is orders of magnitude outside the bar."""
	c, r, X, Y, bars = R.case_data(64, 3, False, np.float64)
	assert np.min(R.ratios(R.model(r, c, X).astype(np.float64), Y, bars)) > 1e6
	assert np.min(R.ratios(R.model(np.roll(c, 1), r, X).astype(np.float64), Y, bars)) > 1e6
