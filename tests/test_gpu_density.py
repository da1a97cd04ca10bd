"""Spectral density on the device (primate_amd.integrate.spectral_density, engine.DensityAccumulator, slq_density_*):
exact cases, parity with the oracle's Gauss rules through the NumPy checker, identities, unbiasedness, determinism,
the input paths, ABI misuse and the two-rank sharded form."""

import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from _density_check import density_np
from conftest import laplacian_2d

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KINDS = ("gaussian", "lorentzian", "histogram", "cdf")


def _host_probes(n: int, P: int, seed: int, pdf: str = "rademacher") -> np.ndarray:
	from primate_amd.random import isotropic

	return isotropic(size=(n, P), pdf=pdf, seed=np.random.default_rng(seed))


@pytest.mark.parametrize("kernel", ["histogram", "cdf"])
def test_exact_case_every_probe_is_the_eigenvalue_histogram(kernel):
	from primate_amd.integrate import spectral_density

	n = 64
	A = sp.diags(np.arange(n) + 0.5).tocsr()
	bins = n if kernel == "histogram" else n + 1
	vals, grid, info = spectral_density(A, bins=bins, interval=(0.0, float(n)), kernel=kernel, deg=n, orth=n, nprobes=48, batch=32, seed=5, full=True)
	want = np.ones(n) if kernel == "histogram" else np.arange(n + 1.0)
	np.testing.assert_allclose(grid, np.arange(n + 1.0))
	np.testing.assert_allclose(vals, want, rtol=0, atol=1e-10)
	assert np.all(info["stderr"] < 1e-10) and info["nprobes"] == 48
	np.testing.assert_allclose(info["outside"], [0.0, 0.0], atol=1e-10)


def _parity_cases():
	from primate_amd.random import symmetric

	D = symmetric(200, pd=True, seed=4) + 0.1 * np.eye(200)
	E = symmetric(12, seed=6)  # n < deg: the rule has n nodes
	few = sp.diags(np.repeat([1.0, 2.0, 3.5, 4.0, 6.0], 8)).tocsr()  # 5 distinct eigenvalues: the run stops after 5 steps
	return {"lap24": laplacian_2d(24), "dense200": D, "dense12": E, "stop5": few}


@pytest.mark.parametrize("name", ["lap24", "dense200", "dense12", "stop5"])
def test_oracle_parity_all_kinds(oracle, name):
	"""Host probes replayed through the oracle; its nodes and weights through the NumPy checker; the device mean must
	match to 1e-10 of max|mean| for every kind and orth 0, 3, deg."""
	from primate_amd.integrate import spectral_density

	A = _parity_cases()[name]
	n, P, deg, seed = A.shape[0], 40, 30, 17
	X = _host_probes(n, P, seed)
	Ad = A.toarray() if sp.issparse(A) else A
	lo, hi = np.linalg.eigvalsh(Ad)[[0, -1]]
	deg = min(deg, n)
	a, b = lo - 0.3137 * (hi - lo), hi + 0.0531 * (hi - lo)  # (part of the spectrum above the grid: the outside mass is exercised)
	for orth in (0, 3, deg):
		_, nodes, weights, _ = oracle.quad_batch(A, X, deg, orth, return_rule=True)
		live = nodes[weights > 0]
		for pts in (np.linspace(a, b, 37), np.linspace(a, b, 38)):  # no grid point or edge on a node: a test of the fold, not of rounding
			assert np.min(np.abs(live[:, None] - pts[None, :])) > 1e-9 * (hi - lo)
		for kernel in KINDS:
			bw = 0.07 * (hi - lo)
			vals, grid, info = spectral_density(A, bins=37, interval=(a, b), bw=bw, kernel=kernel, deg=deg, orth=orth, nprobes=P, batch=P, seed=seed, full=True)
			phi, out = density_np(kernel, grid, bw, nodes, weights, np.sum(X * X, axis=0))
			scale = max(np.abs(phi.mean(axis=0)).max(), 1.0)
			np.testing.assert_allclose(vals, phi.mean(axis=0), rtol=0, atol=1e-10 * scale, err_msg=f"{name} orth={orth} {kernel}")
			np.testing.assert_allclose(info["outside"], out.mean(axis=0), rtol=0, atol=1e-10 * n, err_msg=f"{name} orth={orth} {kernel} outside")


def test_fp32_operator_density_matches_its_own_rule_and_the_oracle(oracle):
	"""fp32 Lanczos: the accumulator checked against the rule of the same run to 1e-10, the density against the oracle's
	fp32 rule to the fp32 parity of the suite (3e-4)."""
	from primate_amd.engine import DensityAccumulator, DeviceOperator, LanczosPlan

	A = laplacian_2d(24, dtype=np.float32)
	n, P, deg = A.shape[0], 32, 30
	X = _host_probes(n, P, 8).astype(np.float32)
	op = DeviceOperator(A)
	plan = LanczosPlan(op, P, deg, 3)
	grid, bw = np.linspace(-0.5, 8.5, 41), 0.3
	for kernel in KINDS:
		g = np.linspace(-0.5, 8.5, 42) if kernel == "histogram" else grid
		acc = DensityAccumulator(kernel, g, bw)
		plan.set_probes(X)
		plan.run()
		_, nodes, weights = plan.quadrature("identity", return_rule=True)
		acc.update(plan)
		mean, _, _, cnt = acc.get()
		vn2 = np.sum(X.astype(np.float64) ** 2, axis=0)
		phi, _ = density_np(kernel, g, bw, nodes, weights, vn2)
		assert cnt == P
		np.testing.assert_allclose(mean, phi.mean(axis=0), rtol=0, atol=1e-10 * max(np.abs(mean).max(), 1.0), err_msg=kernel)
		if kernel in ("gaussian", "lorentzian"):
			_, on, ow, _ = oracle.quad_batch(A, X, deg, 3, return_rule=True)
			ref, _ = density_np(kernel, g, bw, on, ow, vn2)
			np.testing.assert_allclose(mean, ref.mean(axis=0), rtol=0, atol=3e-4 * np.abs(mean).max(), err_msg=f"{kernel} vs oracle")
		acc.close()
	plan.close()
	op.close()


def test_identities_cdf_plus_step_histogram_mass_gaussian_integral():
	from primate_amd.integrate import spectral_density
	from primate_amd.operators import MatrixFunction
	from primate_amd.trace import hutch

	A = laplacian_2d(20)
	n, P, seed = A.shape[0], 64, 21
	## cdf(c) + hutch(step at c, same probes) = mean ||v||^2 = n. The step 1[x >= c] is the device's "numrank" with threshold c
	## (|x| >= c: the same thing on this positive definite operator, whose Ritz values are all positive)
	cdf, cs = spectral_density(A, bins=9, interval=(0.0513, 7.9487), kernel="cdf", deg=30, orth=3, nprobes=P, batch=P, seed=seed)
	for c, v in zip(cs, cdf):
		Ms = MatrixFunction(A, fun="numrank", deg=30, orth=3, threshold=float(c))
		step = hutch(Ms, batch=P, pdf="rademacher", seed=seed, converge="count", count=P)
		assert abs(v + step - n) <= 1e-12 * n, (c, v, step)
	## histogram bins + outside = n (the interval leaves part of the spectrum out on both sides)
	h, _, info = spectral_density(A, bins=50, interval=(1.0, 6.0), kernel="histogram", deg=30, orth=3, nprobes=P, batch=P, seed=seed, full=True)
	assert info["outside"][0] > 1 and info["outside"][1] > 1
	assert abs(h.sum() + info["outside"].sum() - n) <= 1e-12 * n
	## gaussian: the trapezoid integral over a wide grid is n
	g, x = spectral_density(A, bins=4001, interval=(-2.0, 10.0), bw=0.2, kernel="gaussian", deg=30, orth=3, nprobes=P, batch=P, seed=seed)
	assert abs(np.trapezoid(g, x) / n - 1) < 1e-6


def test_unbiased_against_the_exact_smoothed_density():
	from primate_amd.integrate import spectral_density
	from primate_amd.random import symmetric

	n = 300
	ew = np.concatenate([np.linspace(0.5, 2.0, 200), np.linspace(4.0, 5.0, 100)])
	A = symmetric(n, ew=ew, seed=9)
	bw = 0.15
	vals, x, info = spectral_density(A, bins=80, interval=(0.0, 5.5), bw=bw, kernel="gaussian", deg=n, orth=n, nprobes=2048, batch=512, seed=1, full=True)
	exact = np.sum(np.exp(-((x[:, None] - ew[None, :]) ** 2) / (2 * bw * bw)), axis=1) / (bw * np.sqrt(2 * np.pi))
	assert info["nprobes"] == 2048
	assert np.all(np.abs(vals - exact) <= 5 * info["stderr"] + 1e-12), np.max(np.abs(vals - exact) / info["stderr"])


def test_deterministic_and_batch_independent():
	from primate_amd.integrate import spectral_density

	A = laplacian_2d(24)
	kw = dict(bins=300, kernel="lorentzian", deg=30, orth=3, nprobes=512, seed=3, full=True)
	v1, g1, i1 = spectral_density(A, batch=256, **kw)
	v2, g2, i2 = spectral_density(A, batch=256, **kw)
	assert np.array_equal(v1, v2) and np.array_equal(i1["m2"], i2["m2"]) and np.array_equal(g1, g2)
	assert i1["interval"] == i2["interval"] and i1["bw"] == i2["bw"]
	v3, _, _ = spectral_density(A, batch=64, interval=i1["interval"], bw=i1["bw"], **{k: v for k, v in kw.items()})
	np.testing.assert_allclose(v3, v1, rtol=0, atol=1e-9 * np.abs(v1).max())


def test_device_probes_torch_operator_and_matrix_function_inputs():
	import torch

	from primate_amd.integrate import spectral_density
	from primate_amd.operators import MatrixFunction, TorchOperator

	A = laplacian_2d(24)
	kw = dict(bins=60, interval=(-0.5, 8.5), bw=0.25, kernel="gaussian", deg=30, orth=3, full=True)
	vh, _, ih = spectral_density(A, nprobes=1024, batch=256, seed=4, **kw)
	vd, _, idv = spectral_density(A, nprobes=1024, batch=256, seed=4, pdf="device:rademacher", **kw)
	assert np.all(np.abs(vh - vd) <= 5 * np.hypot(ih["stderr"], idv["stderr"]) + 1e-12)
	assert not np.array_equal(vh, vd)
	## a MatrixFunction: its deg / orth are used
	vm, _, im = spectral_density(MatrixFunction(A, deg=30, orth=3), nprobes=64, batch=64, seed=4, **{**kw, "deg": 5, "orth": 0})
	vs, _, _ = spectral_density(A, nprobes=64, batch=64, seed=4, **kw)
	np.testing.assert_allclose(vm, vs, rtol=0, atol=1e-12 * np.abs(vs).max())
	## a TorchOperator (products on the GPU inside the run) against the same matrix as a dense array
	Ad = A.toarray()
	T = torch.tensor(Ad, device="cuda")
	vt, _, _ = spectral_density(TorchOperator(lambda X: T @ X, Ad.shape[0]), nprobes=64, batch=64, seed=4, **kw)
	vn, _, _ = spectral_density(Ad, nprobes=64, batch=64, seed=4, **kw)
	np.testing.assert_allclose(vt, vn, rtol=0, atol=1e-10 * np.abs(vn).max())


def test_one_ql_per_run_and_quadrature_unchanged():
	from primate_amd.engine import DensityAccumulator, DeviceOperator, LanczosPlan

	A = laplacian_2d(24)
	n, P = A.shape[0], 48
	X = _host_probes(n, P, 12)
	op = DeviceOperator(A)
	plan = LanczosPlan(op, P, 30, 3)
	grid = np.linspace(0.0, 8.0, 101)
	## reference: quadrature alone
	plan.set_probes(X)
	plan.run()
	q0, n0, w0 = plan.quadrature("log", return_rule=True)
	## density first, then quadrature: one QL, same quadrature values and rule
	acc1 = DensityAccumulator("histogram", grid)
	plan.profile_enable(True)
	plan.set_probes(X)
	plan.run()
	plan.profile_read(reset=True)
	acc1.update(plan)
	q1, n1, w1 = plan.quadrature("log", return_rule=True)
	assert plan.profile_read(reset=True)["quadrature"]["launches"] == 1
	np.testing.assert_allclose(q1, q0, rtol=1e-14, atol=0)
	assert np.array_equal(n1, n0) and np.array_equal(w1, w0)
	## quadrature first, then density: one QL, the same density
	acc2 = DensityAccumulator("histogram", grid)
	plan.set_probes(X)
	plan.run()
	plan.profile_read(reset=True)
	q2 = plan.quadrature("log")
	acc2.update(plan)
	assert plan.profile_read(reset=True)["quadrature"]["launches"] == 1
	assert np.array_equal(q2, q0)
	m1, s1, o1, c1 = acc1.get()
	m2, s2, o2, c2 = acc2.get()
	assert c1 == c2 == P and np.array_equal(m1, m2) and np.array_equal(s1, s2) and np.array_equal(o1, o2)
	plan.profile_enable(False)
	for h in (acc1, acc2, plan, op):
		h.close()


def test_abi_misuse_is_einval_without_a_device_fault():
	from primate_amd import _capi
	from primate_amd.engine import Context, DensityAccumulator, DeviceOperator, LanczosPlan, default_context

	L = _capi.lib()
	A = laplacian_2d(10)
	op = DeviceOperator(A)
	plan = LanczosPlan(op, 8, 10, 2)
	grid = np.linspace(0.0, 8.0, 11)
	acc = DensityAccumulator("gaussian", grid, 0.5)
	h = C.c_void_p()
	ctx = default_context()._h
	assert L.slq_density_update(acc._h, plan._h) == _capi.SLQ_EINVAL  # no run yet
	assert L.slq_density_update(acc._h, None) == _capi.SLQ_EINVAL
	assert L.slq_density_update(None, plan._h) == _capi.SLQ_EINVAL
	bad = np.array([0.0, 2.0, 1.0, 3.0])
	assert L.slq_density_create(ctx, 0, 4, _capi.ptr(bad), 0.5, C.byref(h)) == _capi.SLQ_EINVAL
	assert L.slq_density_create(ctx, 2, 3, _capi.ptr(np.array([0.0, 1.0, 1.0, 2.0])), 0.0, C.byref(h)) == _capi.SLQ_EINVAL  # repeated edge
	for bw in (0.0, -1.0, float("nan")):
		assert L.slq_density_create(ctx, 1, 11, _capi.ptr(grid), bw, C.byref(h)) == _capi.SLQ_EINVAL
	assert L.slq_density_create(ctx, 0, 0, _capi.ptr(grid), 0.5, C.byref(h)) == _capi.SLQ_EINVAL
	assert L.slq_density_create(ctx, 7, 11, _capi.ptr(grid), 0.5, C.byref(h)) == _capi.SLQ_EINVAL
	assert L.slq_density_create(ctx, 3, 11, _capi.ptr(grid), 0.0, C.byref(h)) == 0  # (bw is not read by the cdf)
	L.slq_density_destroy(h)
	with pytest.raises(ValueError):
		DensityAccumulator("histogram", bad)
	## a plan of another context
	ctx2 = Context(device=default_context().device)
	op2 = DeviceOperator(A, ctx=ctx2)
	plan2 = LanczosPlan(op2, 8, 10, 2)
	plan2.generate_probes("rademacher", seed=1)
	plan2.run()
	assert L.slq_density_update(acc._h, plan2._h) == _capi.SLQ_EINVAL
	## the accumulator still works
	plan.generate_probes("rademacher", seed=1)
	plan.run()
	acc.update(plan)
	mean, m2, out, cnt = acc.get()
	assert cnt == 8 and np.all(np.isfinite(mean)) and np.all(np.isfinite(m2))
	for hh in (acc, plan, op, plan2, op2):
		hh.close()
	ctx2.close()


def test_two_ranks_equal_one_process(tmp_path):
	"""World 2 over gloo on one shared GPU: sharded_spectral_density equals spectral_density over the same probe ids."""
	from primate_amd.integrate import spectral_density

	env = dict(os.environ, MASTER_ADDR="127.0.0.1", DIST_TEST_SHARE_GPU0="1")
	out = tmp_path / "dens"
	cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
	       "--master-port", "29547", str(ROOT / "tests" / "_dist_density_worker.py"), str(out)]  # fmt: skip
	r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
	assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
	res = [json.load(open(f"{out}.rank{k}.json")) for k in range(2)]
	A = laplacian_2d(24)
	for key, pdf in (("device", "device:rademacher"), ("host", "rademacher")):
		v, g, info = spectral_density(A, bins=64, interval=(-0.5, 8.5), bw=0.2, kernel="gaussian", deg=30, orth=3, nprobes=96, batch=24, pdf=pdf, seed=5, full=True)
		for rr in res:
			got = np.array(rr[key]["values"])
			assert rr[key]["nprobes"] == 96
			np.testing.assert_allclose(got, v, rtol=0, atol=1e-12 * np.abs(v).max(), err_msg=key)
			np.testing.assert_allclose(np.array(rr[key]["stderr"]), info["stderr"], rtol=1e-8, err_msg=key)
			np.testing.assert_allclose(rr[key]["grid"], g)
