"""The two host paths every product of the side objects shares - the host-staged panel product with its two pitched
copies, and the operand check and addresses of the DeviceMatrix entries - pinned directly: for the cross product forward and adjoint,
the feature product, its adjoint and the preconditioner's apply, in fp64, the host-staged C entry - called with leading dimensions
beyond the row counts, which the Python wrappers never pass - and the DeviceMatrix entry return the same bits, and the rows of the
caller's output between `rout` and `ldy` are left alone. And the one life cycle of the eight side handles: create, use, close, close
again, with the device bytes the library holds back where they were.

n = 40 points in d = 3, m = 7 new points, F2 = 5 frequencies, b = 1 and 17 columns, a preconditioner of rank 8. The slab driver's two
branches both occur: a summed side of at most 16 points is one tile and so one slab (the cross adjoint over the 7 new points, the
feature product over 5 frequencies, the adjoint feature product over 7 new points), and a longer one falls short of the chip and is
split (the cross product and the adjoint feature product over the 40 points). The feature product sums over the frequencies alone, so
a second map of 40 frequencies brings its slab sum in. `test_both_slab_branches_occur` reads this off the library's schedules at the
device's CU count."""

import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, M, F2, F2_SLABS, RANK = 40, 3, 7, 5, 40, 8
SENTINEL = -7.25


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


@pytest.fixture(scope="module")
def world(eng):
	import torch

	from primate_amd.operators import KernelOperator

	rng = np.random.default_rng(31)
	X = rng.standard_normal((N, D))
	K = KernelOperator(X, "rbf", lengthscale=0.8, outputscale=1.3, noise=0.1)
	op = eng.DeviceOperator(K)
	w = dict(op=op, ctx=op.ctx, cross=eng.KernelCross(op, rng.standard_normal((M, D))), pre=eng.DeviceOperator(K.preconditioned(RANK), ctx=op.ctx),
	         fmap={f2: eng.KernelFeatureMap(op, rng.standard_normal((f2, D))) for f2 in (F2, F2_SLABS)},
	         cus=torch.cuda.get_device_properties(op.ctx.device).multi_processor_count)  # fmt: skip
	w["plan"] = eng.LanczosPlan(op, 4, 10, 3, keep_basis=True)
	w["plan"].generate_probes("rademacher", seed=3)
	w["plan"].run()
	yield w
	for x in (w["plan"], *w["fmap"].values(), w["pre"], w["cross"], op):
		x.close()


def _product(eng, w, kind, f2, rows):
	"""(rin, rout, the host-staged C entry, the DeviceMatrix entry, the slab count of b columns or None) of one product."""
	from primate_amd import _capi

	L, cross, pre, cus = _capi.lib(), w["cross"], w["pre"], w["cus"]
	fmap = w["fmap"].get(f2)
	rh, nr = (cross._h, M) if rows else (None, N)
	if kind in ("cross", "cross_adjoint"):
		t = int(kind == "cross_adjoint")
		rin, rout = (M, N) if t else (N, M)
		return (rin, rout, lambda X, ldx, Y, ldy, b: L.slq_kernel_cross_matmat(cross._h, t, X, ldx, Y, ldy, b),
		        lambda IN, OUT, b: cross.matmat_dmat(IN, 0, OUT, 0, b, trans=bool(t)), lambda b: eng.kernel_cross_schedule(rout, rin, b, cus)["slabs"])  # fmt: skip
	if kind == "feature":
		return (2 * f2, nr, lambda X, ldx, Y, ldy, b: L.slq_kernel_feature_matmat(fmap._h, rh, X, ldx, Y, ldy, b),
		        lambda IN, OUT, b: fmap.matmat_dmat(IN, 0, OUT, 0, b, rows=cross if rows else None), lambda b: eng.kernel_feature_schedule(nr, f2, b, cus)["slabs"])  # fmt: skip
	if kind == "feature_adjoint":
		return (nr, 2 * f2, lambda X, ldx, Y, ldy, b: L.slq_kernel_feature_rmatmat(fmap._h, rh, X, ldx, Y, ldy, b),
		        lambda IN, OUT, b: fmap.rmatmat_dmat(IN, 0, OUT, 0, b, rows=cross if rows else None), lambda b: eng.kernel_feature_adjoint_schedule(f2, nr, b, cus)["slabs"])  # fmt: skip
	assert kind == "precond"
	return (N, N, lambda X, ldx, Y, ldy, b: L.slq_kernel_precond_apply(pre._h, X, ldx, Y, ldy, b), lambda IN, OUT, b: pre.inv_sqrt_dmat(IN, 0, OUT, 0, b), lambda b: None)


# (product, frequencies of the map, rows at the cross object's new points)
PRODUCTS = [("cross", 0, False), ("cross_adjoint", 0, False), ("feature", F2, False), ("feature", F2, True), ("feature", F2_SLABS, False),
            ("feature_adjoint", F2, False), ("feature_adjoint", F2, True), ("precond", 0, False)]  # fmt: skip
CASES = [(*p, b) for p in PRODUCTS for b in (1, 17)]
IDS = [f"{k}{'-F2=' + str(f) if f else ''}{'-rows' if r else ''}-b={b}" for k, f, r, b in CASES]


@pytest.mark.parametrize("kind,f2,rows,b", CASES, ids=IDS)
def test_staged_and_device_matrix_entries_agree_bitwise_and_padding_rows_are_kept(eng, world, kind, f2, rows, b):
	from primate_amd import _capi

	rin, rout, staged, dmat, _ = _product(eng, world, kind, f2, rows)
	rng = np.random.default_rng(100 * rin + b)
	X = rng.standard_normal((rin, b))
	Xp = np.full((rin + 3, b), np.nan, order="F")  # (the rows between rin and ldx are not the product's: NaN would show if one were read)
	Xp[:rin] = X
	Yp = np.full((rout + 5, b), SENTINEL, order="F")
	_capi.check(staged(_capi.ptr(Xp), rin + 3, _capi.ptr(Yp), rout + 5, b))
	assert np.all(Yp[rout:] == SENTINEL), "the pitched copy out wrote beyond the product's rows"
	assert np.all(np.isfinite(Yp[:rout])) and np.any(Yp[:rout] != SENTINEL)
	IN, OUT = eng.DeviceMatrix(rin, b, ctx=world["ctx"]), eng.DeviceMatrix(rout, b, ctx=world["ctx"])
	try:
		IN.set(0, X)
		dmat(IN, OUT, b)
		assert np.array_equal(OUT.get(0, b), Yp[:rout]), "host-staged and DeviceMatrix entries differ"
	finally:
		IN.close()
		OUT.close()


def test_both_slab_branches_occur(eng, world):
	"""Per slab-driven product the case list holds a case of one slab (written straight into the result) and one of several (partials
	in the scratch, then the slab sum), by the library's own schedules at this device's CU count."""
	slabs = {}
	for kind, f2, rows, b in CASES:
		s = _product(eng, world, kind, f2, rows)[4](b)
		if s is not None:
			slabs.setdefault(kind.split("_adjoint")[0] if kind.startswith("cross") else kind, []).append(s)
	assert set(slabs) == {"cross", "feature", "feature_adjoint"}
	for product, counts in slabs.items():
		assert min(counts) == 1 and max(counts) > 1, (product, counts)


def device_bytes():
	from primate_amd import _capi

	v = C.c_int64()
	_capi.check(_capi.lib().slq_debug_operator_device_bytes(C.byref(v)))
	return v.value


def _use_diag(eng, w):
	acc = eng.DiagAccumulator(N, ctx=w["ctx"])
	acc.update(w["plan"], "log")
	assert acc.get()[3] == 4
	return [acc]


def _use_density(eng, w):
	acc = eng.DensityAccumulator("gaussian", np.linspace(0.0, 20.0, 9), bw=1.0, ctx=w["ctx"])
	acc.update(w["plan"])
	assert acc.get()[3] == 4
	return [acc]


def _pair(eng, w, rows=N, cols=6):
	A = eng.DeviceMatrix(rows, cols, ctx=w["ctx"])
	A.generate(0, cols, "rademacher", seed=rows)
	return A


def _use_dmat(eng, w):
	A = _pair(eng, w)
	assert A.tn(0, 3, A, 3, 3).shape == (3, 3)
	return [A]


def _use_sddmm(eng, w):
	import scipy.sparse as sp

	A = _pair(eng, w)
	acc = eng.SddmmAccumulator(sp.random(N, N, density=0.1, random_state=2, format="csr") + sp.identity(N, format="csr"), ctx=w["ctx"])
	acc.update(A, 0, A, 3, 3, beta=0.0)
	assert acc.get()[1] == 3
	return [acc, A]


def _use_grad(eng, w):
	A = _pair(eng, w)
	acc = eng.KernelGradAccumulator(w["op"])
	acc.update(A, 0, A, 3, 3, beta=0.0)
	assert acc.get()[1] == 3
	return [acc, A]


def _use_cross(eng, w):
	cross = eng.KernelCross(w["op"], np.linspace(-1.0, 1.0, M * D).reshape(M, D))
	assert cross.matmat(np.ones((N, 17))).shape == (M, 17)  # (several slabs: staging buffers and the slab scratch grow)
	return [cross]


def _use_feature(eng, w):
	fmap = eng.KernelFeatureMap(w["op"], np.linspace(-1.0, 1.0, F2_SLABS * D).reshape(F2_SLABS, D))
	assert fmap.matmat(np.ones((2 * F2_SLABS, 17))).shape == (N, 17)
	return [fmap]


def _use_pointgrad(eng, w):
	A, U = _pair(eng, w), _pair(eng, w, rows=M)
	acc, cacc = eng.KernelPointGradAccumulator(w["op"]), eng.KernelPointGradAccumulator(w["cross"])
	acc.update(A, 0, A, 3, 3, beta=0.0)
	cacc.update(U, 0, A, 0, 3, beta=0.0)
	assert acc.get()[1] == 3 and cacc.get()[1] == 3
	return [acc, cacc, A, U]


@pytest.mark.parametrize("handle", ["diag", "density", "dmat", "sddmm", "grad", "cross", "feature", "pointgrad"])
def test_create_use_close_close_again_returns_the_device_bytes(eng, world, handle):
	gc.collect()
	start = device_bytes()
	objects = globals()[f"_use_{handle}"](eng, world)
	assert device_bytes() > start
	for x in objects:
		x.close()
		x.close()
	assert device_bytes() == start
