"""The dense operator's product kernels at every variant and edge (slq_kernels.hpp: k_dense_panel, k_dense_mfma_3term,
k_dense_mfma_tile, k_dense_mfma_lds, k_dense_mfma32_lds, k_3term_slabs), chosen in slq.hip by panel width, the parity of the
leading dimension and the SLQ_DENSE_* switches. Every item first asserts WHICH kernel its plan launches (slq_plan_dense_path):
a switch that is silently ignored would turn the item into a repeat of the default path.

 (a) integer operands: every partial sum is an exact float, so the product equals the int64 product bit for bit whatever the
     summation order, K split or instruction; A is not symmetric, so A^T X fails.
 (b) standard-normal operands against a long-double product, elementwise within (n + 18) u |A| |X|: an fma chain of at
     most n terms per slab, at most 16 slab or wave sums, the unit scale. A lost or doubled term is ~1/n of |A| |X|.
 (c) the fused three-term epilogue and the alpha partials: alpha, beta of EVERY column against oracle.lanczos, the log
     quadrature against oracle.quad_batch, f = identity against v^T A v.
 (d) a leading dimension above n through the C-ABI, padding rows NaN.
 (e) the fp64 kernels and the K splits against each other; a repeat of the same variant bitwise.

The shapes are the smallest that reach each piece of index logic: n around the lone k-quad, the 16-, 32-, 128- and 256-row
tiles and the 16-deep LDS stage, odd n (the one-row tail of the row-pair loads); P at both sides of every panel width,
and two and three panels with a nearly empty last one. Each item prints its worst ratio to the bar before it asserts
(`-s` shows them)."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
NS = (1, 2, 3, 4, 5, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300, 301)
PS = (1, 16, 17, 32, 33, 64, 65, 128, 129, 257)
PMAX = max(PS)
SWITCHES = ("SLQ_DENSE_MFMA", "SLQ_DENSE_TILE16", "SLQ_DENSE_LDS", "SLQ_DENSE_KSPLIT")
V64 = (
	[{}, {"SLQ_DENSE_LDS": "0"}, {"SLQ_DENSE_TILE16": "1"}, {"SLQ_DENSE_MFMA": "0"}]
	+ [{"SLQ_DENSE_KSPLIT": str(k)} for k in (1, 2, 7, 16)]
	+ [{"SLQ_DENSE_KSPLIT": str(k), "SLQ_DENSE_LDS": "0"} for k in (1, 2, 7, 16)]
)
V32 = [{}, {"SLQ_DENSE_MFMA": "0"}, {"SLQ_DENSE_KSPLIT": "1"}, {"SLQ_DENSE_KSPLIT": "16"}]
CASES = [(F64, v, P) for v in V64 for P in PS] + [(F32, v, P) for v in V32 for P in PS]
KERNEL_NAMES = {1: "k_dense_panel", 2: "k_dense_mfma_3term", 3: "k_dense_mfma_tile", 4: "k_dense_mfma_lds", 5: "k_dense_mfma32_lds"}


def _vid(v):
	return ",".join(f"{k[10:]}={x}" for k, x in v.items()) or "default"


def _ids(cases):
	return [f"{np.dtype(c[0]).name}-{_vid(c[1])}-P{c[2]}" for c in cases]


def ns_of(dtype):
	return NS + ((517,) if dtype == F32 else ())


def unit(dtype):
	return 2.0**-53 if dtype == F64 else 2.0**-24


def expected_path(dtype, variant, lda, P):
	"""(kernel, ksplit) as the switch table states them, written down independently of slq.hip; ksplit None = chosen
	by the plan, 1..16. lda is the leading dimension of the operator's device copy, which is n however the host array is strided (slq_dense_create
	uploads it compactly): k_dense_mfma_lds needs 16-byte aligned row pairs."""
	V = 2 if dtype == F64 else 4
	lpr = 8
	while lpr < 64 and lpr * V < P:
		lpr *= 2
	pw = lpr * V
	forced = int(variant.get("SLQ_DENSE_KSPLIT", 0)) or None
	if variant.get("SLQ_DENSE_MFMA") == "0":
		return 1, 0
	if dtype == F32:
		return 5, forced
	if pw == 16 or variant.get("SLQ_DENSE_TILE16") == "1":
		return 2, 0
	if pw >= 64 and variant.get("SLQ_DENSE_LDS") != "0" and lda % 2 == 0:
		return 4, forced
	return 3, forced


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


@pytest.fixture
def variant_env(monkeypatch):
	def set_variant(variant):
		for k in SWITCHES:
			monkeypatch.delenv(k, raising=False)
		for k, x in variant.items():
			monkeypatch.setenv(k, x)

	return set_variant


def assert_path(eng, op, dtype, variant, P, what=""):
	"""The kernel and K split of the plan DeviceOperator.matmat builds for P columns; returns the kernel id."""
	want_k, want_ks = expected_path(dtype, variant, op.shape[0], P)
	plan = eng.LanczosPlan(op, P, 1, 0)
	d = plan.describe()
	plan.close()
	assert d["dense_kernel"] == want_k, f"{what} n={op.shape[0]} P={P} {variant}: kernel {d['dense_kernel']}, expected {want_k} ({KERNEL_NAMES[want_k]})"
	if want_ks is None:
		assert 1 <= d["dense_ksplit"] <= 16, (what, op.shape[0], P, variant, d)
	else:
		assert d["dense_ksplit"] == want_ks, f"{what} n={op.shape[0]} P={P} {variant}: K split {d['dense_ksplit']}, expected {want_ks}"
	V = 2 if dtype == F64 else 4
	assert d["panels"] == -(-P // d["panel_width"]) and d["panel_width"] in (8 * V, 16 * V, 32 * V, 64 * V)
	return want_k


## ---- inputs and references: computed once per (dtype, n) for PMAX columns, sliced per P, never written to -------------
_cache = {}


def exact_case(dtype, n):
	"""Integer A (not symmetric), X and the int64 product."""
	key = ("exact", np.dtype(dtype).name, n)
	if key not in _cache:
		rng = np.random.default_rng(1000 * n + (dtype == F32))
		lim = 1000 if dtype == F64 else 64
		A = rng.integers(-lim, lim + 1, (n, n))
		X = rng.integers(-lim, lim + 1, (n, PMAX))
		ref = A.astype(np.int64) @ X.astype(np.int64)
		assert n * lim * lim < (2**53 if dtype == F64 else 2**24)  # every partial sum is an exact float
		for Z in (A, X, ref):
			Z.setflags(write=False)
		_cache[key] = (A, X, ref)
	return _cache[key]


def longdouble_matmul(A, X):
	if np.finfo(np.longdouble).eps < 2.0**-60:
		return A.astype(np.longdouble) @ X.astype(np.longdouble)
	import mpmath  # a host whose long double is a double: 100-bit products and sums

	mpmath.mp.prec = 100
	out = np.empty((A.shape[0], X.shape[1]), dtype=np.float64)
	for i in range(A.shape[0]):
		for j in range(X.shape[1]):
			out[i, j] = float(mpmath.fsum(mpmath.mpf(float(a)) * mpmath.mpf(float(x)) for a, x in zip(A[i], X[:, j])))
	return out


def rounded_case(dtype, n):
	"""Standard-normal A (not symmetric), X, the extended-precision product and |A| |X|."""
	key = ("rounded", np.dtype(dtype).name, n)
	if key not in _cache:
		rng = np.random.default_rng(2000 * n + (dtype == F32))
		A = rng.standard_normal((n, n)).astype(dtype)
		X = rng.standard_normal((n, PMAX)).astype(dtype)
		ref = longdouble_matmul(A, X)
		mag = np.abs(A).astype(np.float64) @ np.abs(X).astype(np.float64)
		for Z in (A, X, ref, mag):
			Z.setflags(write=False)
		_cache[key] = (A, X, ref, mag)
	return _cache[key]


def bound_ratio(Y, ref, mag, n, dtype):
	"""max |Y - ref| / ((n + 18) u |A||X|), elementwise (the difference taken in the reference's precision)."""
	err = np.abs(Y.astype(ref.dtype) - ref).astype(np.float64)
	return float(np.max(err / ((n + 18) * unit(dtype) * mag)))


## ---- (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,variant,P", CASES, ids=_ids(CASES))
def test_exact_integer_product(eng, variant_env, dtype, variant, P):
	variant_env(variant)
	kernels = set()
	for n in ns_of(dtype):
		A, X, ref = exact_case(dtype, n)
		Af, Xf = A.astype(dtype), X[:, :P].astype(dtype)
		## C-ordered matrix with F-ordered columns, then F-ordered matrix with C-ordered columns
		for Aop, Xop in ((np.ascontiguousarray(Af), np.asfortranarray(Xf)), (np.asfortranarray(Af), np.ascontiguousarray(Xf))):
			op = eng.DeviceOperator(Aop)
			kernels.add(assert_path(eng, op, dtype, variant, P, what="exact"))
			Y = op.matmat(Xop)
			op.close()
			if not np.array_equal(Y, ref[:, :P]):
				bad = np.argwhere(Y != ref[:, :P])
				transposed = np.array_equal(Y, (A.T.astype(np.int64) @ X[:, :P].astype(np.int64)))
				pytest.fail(
					f"n={n} P={P} {variant} ({'C' if Aop.flags.c_contiguous else 'F'}-ordered A): {len(bad)} of {Y.size} entries differ; rows "
					f"{bad[:, 0].min()}..{bad[:, 0].max()}, columns {bad[:, 1].min()}..{bad[:, 1].max()}, first {tuple(bad[0])}: got {Y[tuple(bad[0])]}, "
					f"exact {ref[tuple(bad[0])]}{'; the product is A^T X' if transposed else ''}"
				)
	print(f"[dense-parity] check=a dtype={np.dtype(dtype).name} variant={_vid(variant)} P={P} kernels={sorted(kernels)} exact")


## ---- (b) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,variant,P", CASES, ids=_ids(CASES))
def test_rounded_product_within_the_derived_bound(eng, variant_env, dtype, variant, P):
	variant_env(variant)
	worst = {}
	for n in ns_of(dtype):
		A, X, ref, mag = rounded_case(dtype, n)
		op = eng.DeviceOperator(A)
		k = assert_path(eng, op, dtype, variant, P, what="rounded")
		Y = op.matmat(np.asfortranarray(X[:, :P]))
		op.close()
		assert np.all(np.isfinite(Y)), f"n={n} P={P} {variant}"
		r = bound_ratio(Y, ref[:, :P], mag[:, :P], n, dtype)
		if r > worst.get(k, (-1.0, 0))[0]:
			worst[k] = (r, n)
	for k, (r, n) in sorted(worst.items()):
		print(f"[dense-parity] check=b dtype={np.dtype(dtype).name} variant={_vid(variant)} P={P} kernel={k} worst={r:.4f} n={n}")
	for k, (r, n) in worst.items():
		assert r <= 1.0, f"n={n} P={P} {variant} {KERNEL_NAMES[k]}: |Y - ref| reaches {r:.3g} x (n + 18) u |A||X|"


## ---- (c) ------------------------------------------------------------------------------------------------------------------
LANCZOS_NS = (5, 33, 129, 256, 301)
LANCZOS_PS = (1, 17, 33, 65, 129, 257)
LANCZOS_CASES = [(F64, v, P) for v in V64 for P in LANCZOS_PS] + [(F32, v, P) for v in V32 for P in LANCZOS_PS]


def lanczos_case(oracle, dtype, n, orth):
	"""SPD A = B B^T / n + I, Rademacher probes, and the oracle's alpha, beta (per column) and log quadrature for all PMAX columns."""
	key = ("lanczos", np.dtype(dtype).name, n, orth)
	if key not in _cache:
		rng = np.random.default_rng(3000 * n)
		B = rng.standard_normal((n, n))
		A = B @ B.T / n + np.eye(n)
		A = np.asfortranarray(((A + A.T) / 2).astype(dtype))
		V = np.asfortranarray((np.floor(rng.random((n, PMAX)) * 2) * 2 - 1).astype(dtype))
		deg = min(12, n)
		al, be = np.zeros((PMAX, deg + 1), dtype), np.zeros((PMAX, deg + 1), dtype)
		steps = np.zeros(PMAX, dtype=np.int32)
		for c in range(PMAX):
			Q = np.zeros((n, max(orth, 2)), dtype, order="F")
			steps[c] = oracle.lanczos(A, V[:, c].copy(), deg, 1e-8, min(orth, deg), al[c], be[c], Q)
		quad = oracle.quad_batch(A, V, deg, orth, fun="log", fresh_q=True)
		vAv = np.einsum("ij,ij->j", V.astype(np.float64), A.astype(np.float64) @ V.astype(np.float64))
		for Z in (A, V, al, be, steps, quad, vAv):
			Z.setflags(write=False)
		_cache[key] = (A, V, deg, al, be, steps, quad, vAv)
	return _cache[key]


@pytest.mark.parametrize("dtype,variant,P", LANCZOS_CASES, ids=_ids(LANCZOS_CASES))
def test_three_term_epilogue_and_alpha_partials_through_lanczos(oracle, eng, variant_env, dtype, variant, P):
	"""Bars: alpha, beta within 1e-10 (fp64) / 3e-4 (fp32) of the tridiagonal's largest entry, for every column; the log quadrature within the
	same bar relative to its value; f = identity within 1e-11 (fp64; fp32: its bar) of v^T A v."""
	variant_env(variant)
	bar = 1e-10 if dtype == F64 else 3e-4
	bar_id = 1e-11 if dtype == F64 else 3e-4
	worst = {"tridiag": (0.0, None), "log": (0.0, None), "identity": (0.0, None)}
	kernels = set()
	failures = []
	for n in LANCZOS_NS:
		for orth in (0, 3):
			A, V, deg, al, be, steps, quad, vAv = lanczos_case(oracle, dtype, n, orth)
			op = eng.DeviceOperator(A)
			kernels.add(assert_path(eng, op, dtype, variant, P, what="lanczos"))
			plan = eng.LanczosPlan(op, P, deg, orth)
			d = plan.describe()
			assert d["dense_kernel"] in kernels, d
			plan.set_probes(np.asfortranarray(V[:, :P]))
			plan.run()
			a, b, st = plan.tridiag()
			q_log = plan.quadrature("log")
			q_id = plan.quadrature("identity")
			plan.close()
			op.close()
			where = f"n={n} orth={orth} P={P} {variant}"
			assert np.array_equal(st, steps[:P]), f"{where}: steps {st} against the oracle's {steps[:P]}"
			scale = np.max(np.abs(al[:P, :deg]), axis=1, keepdims=True).astype(np.float64)
			e_tri = max(np.max(np.abs(a[:, :deg].astype(np.float64) - al[:P, :deg]) / scale), np.max(np.abs(b[:, :deg].astype(np.float64) - be[:P, :deg]) / scale))
			e_log = np.max(np.abs(q_log / quad[:P] - 1.0))
			e_id = np.max(np.abs(q_id / vAv[:P] - 1.0))
			for name, e, lim in (("tridiag", e_tri, bar), ("log", e_log, bar), ("identity", e_id, bar_id)):
				if not e <= lim:  # (NaN fails)
					failures.append(f"{where}: {name} error {e:.3e} above {lim:g}")
				if not e / lim <= worst[name][0]:
					worst[name] = (float(e / lim), (n, orth))
	print(f"[dense-parity] check=c dtype={np.dtype(dtype).name} variant={_vid(variant)} P={P} kernels={sorted(kernels)} " + " ".join(f"{k}={r:.4g}@n{w[0]}o{w[1]}" for k, (r, w) in worst.items() if w))
	assert not failures, "\n".join(failures)


## ---- (d) ------------------------------------------------------------------------------------------------------------------
def strided_operator(eng, A, pad=3):
	"""slq_dense_create on an F-ordered (n + pad) x n buffer whose padding rows hold NaN; returns (operator, lda)."""
	from primate_amd import _capi

	n = A.shape[0]
	buf = np.full((n + pad, n), np.nan, dtype=A.dtype, order="F")
	buf[:n, :] = A
	ctx = eng.default_context()
	h = C.c_void_p()
	_capi.check(_capi.lib().slq_dense_create(ctx._h, _capi.dtype_id(A.dtype), n, _capi.ptr(buf), n + pad, C.byref(h)))
	op = object.__new__(eng.DeviceOperator)  # the C handle under the Python surface (DeviceOperator itself always passes lda = n)
	op.ctx, op.dtype, op.shape, op._keep, op.kind, op.nnz, op._h = ctx, np.dtype(A.dtype), (n, n), [], "dense", n * n, h
	return op, n + pad


@pytest.mark.parametrize("variant", [{}, {"SLQ_DENSE_MFMA": "0"}], ids=_vid)
@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
def test_leading_dimension_above_n(eng, variant_env, dtype, symmetric, variant):
	variant_env(variant)
	kernels = set()
	for n in (5, 33, 300):
		A, X, _ = exact_case(dtype, n)
		if symmetric:
			A = A + A.T  # (entries to 2 lim: the partial sums stay exact floats)
			assert 2 * n * (1000 if dtype == F64 else 64) ** 2 < (2**53 if dtype == F64 else 2**24)
		ref = A.astype(np.int64) @ X.astype(np.int64)
		op, lda = strided_operator(eng, A.astype(dtype))
		for P in (16, 33, 65, 129):
			## (the device copy is compact, leading dimension n: the host's lda plays no part in the choice of the kernel)
			kernels.add(assert_path(eng, op, dtype, variant, P, what="lda"))
			Y = op.matmat(np.asfortranarray(X[:, :P].astype(dtype)))
			assert not np.any(np.isnan(Y)), f"n={n} lda={lda} P={P} {variant}: NaN in the product - the padding rows were read"
			assert np.array_equal(Y, ref[:, :P]), f"n={n} lda={lda} P={P} {variant}: {np.count_nonzero(Y != ref[:, :P])} entries differ"
		op.close()
	print(f"[dense-parity] check=d dtype={np.dtype(dtype).name} variant={_vid(variant)} symmetric={symmetric} kernels={sorted(kernels)} exact")


## ---- (e) ------------------------------------------------------------------------------------------------------------------
def test_variants_agree_and_repeat_bitwise(eng, variant_env):
	"""One real-valued operator, one panel (n = 300, P = 64): k_dense_mfma_lds, k_dense_mfma_tile and k_dense_mfma_3term and the K splits 1
	and 16 of the first two agree within twice the bound of (b) - each is within one bound of the exact product -, and the same variant
	run twice agrees bitwise (the slab and wave sums are in fixed order)."""
	n, P = 300, 64
	A, X, ref, mag = rounded_case(F64, n)
	Xp = np.asfortranarray(X[:, :P])
	variants = [{}, {"SLQ_DENSE_LDS": "0"}, {"SLQ_DENSE_TILE16": "1"}] + [dict(v, SLQ_DENSE_KSPLIT=k) for k in ("1", "16") for v in ({}, {"SLQ_DENSE_LDS": "0"})]
	got, seen = [], set()
	for v in variants:
		variant_env(v)
		op = eng.DeviceOperator(A)
		seen.add(assert_path(eng, op, F64, v, P, what="agree"))
		Y1, Y2 = op.matmat(Xp), op.matmat(Xp)
		op.close()
		assert np.array_equal(Y1, Y2), f"{v}: two runs differ in {np.count_nonzero(Y1 != Y2)} entries"
		got.append(Y1)
	assert seen == {2, 3, 4}
	worst = 0.0
	for i in range(len(variants)):
		for j in range(i):
			r = float(np.max(np.abs(got[i] - got[j]) / (2 * (n + 18) * unit(F64) * mag[:, :P])))
			worst = max(worst, r)
			assert r <= 1.0, f"{variants[i]} against {variants[j]}: {r:.3g} x twice the bound"
	print(f"[dense-parity] check=e dtype=float64 worst={worst:.4f} of twice the bound over {len(variants)} variants")
