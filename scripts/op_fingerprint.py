"""Fingerprint of what an operator's creation decides (order, tiles, streams) through what it produces: sha256 of alpha, beta and the
quadrature values of one seeded 256 x 30 run per operator. Two libraries that print the same lines build the same operators
(r04: used to show that the device-side build, the stamp-based regrouping and the cached first-level Cuthill-McKee leave every result
bitwise unchanged; later: that slq_layout.hpp does - the cases then cover the host builder, barrier tiles, a forced reorder without tiles, a
random graph, creation from device arrays, an affine and a Gram operator; later still: that one tile walk for the kernel-operator
family does - the "kernel ..." lines are sha256 of products, cross products and a gradient update themselves; and that one product
driver and one handle life cycle for the side objects do - side_objects(), profiles/side_objects_fingerprint.txt; --posterior: only the two
"posterior ..." lines of tests/_gp_mll_ref.posterior_fingerprint_lines, sha256 of gp.posterior's mean and variance without and with the
preconditioner - factoring its solve helper out for gp.mll leaves them as they were: profiles/gp_mll_posterior_fingerprint.txt).
PRIMATE_AMD_LIBSLQ=<other library> python scripts/op_fingerprint.py [--posterior]"""
import hashlib, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
from conftest import laplacian_2d, laplacian_3d
from primate_amd import engine as eng

if "--posterior" in sys.argv:
	from _gp_mll_ref import posterior_fingerprint_lines
	for line in posterior_fingerprint_lines():
		print(line, flush=True)
	sys.exit(0)

def random_graph(n=500000, deg=16, seed=1234):  # (the pattern of scripts/time_create.py's random graph plus a dominant diagonal: no tiles, automatic reorder declined)
	import scipy.sparse as sp
	rng = np.random.default_rng(seed)
	m = int(n * deg / 2)
	i, j = rng.integers(0, n, m), rng.integers(0, n, m)
	keep = i != j
	W = sp.coo_matrix((np.ones(keep.sum()), (i[keep], j[keep])), shape=(n, n)).tocsr()
	W = ((W + W.T) > 0).astype(np.float64).tocsr()
	W = (W + sp.identity(n) * (deg * 4.0)).tocsr()  # (diagonally dominant: log is defined)
	W.sort_indices()
	return W

def on_device(A):  # slq_csr_create_device: the operator from arrays that already live on the GPU
	import torch
	return torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int64)), torch.from_numpy(A.indices.astype(np.int64)), torch.from_numpy(A.data), size=A.shape).to("cuda")

def affine():
	from primate_amd.operators import AffineOperator
	import scipy.sparse as sp
	A = laplacian_2d(300)
	return AffineOperator(A, sp.diags(np.linspace(0.5, 1.5, A.shape[0])).tocsr(), t=0.75)

def gram():
	from primate_amd.operators import GramOperator
	import scipy.sparse as sp
	rng = np.random.default_rng(9)
	m = 650000
	B = sp.coo_matrix((rng.uniform(0.5, 1.5, m), (rng.integers(0, 120000, m), rng.integers(0, 90000, m))), shape=(120000, 90000)) + sp.eye(120000, 90000) * 3.0
	return GramOperator(B.tocsr())

# (label, matrix or builder, switches the operator is created under, probes, orth)
cases = [("lap2d_1000", lambda: laplacian_2d(1000), {}, 256, 3), ("lap2d_1000", None, {}, 64, 3), ("lap3d_100", lambda: laplacian_3d(100), {}, 256, 3), ("lap3d_100", None, {}, 64, 6),
         ("lap3d_100", None, {}, 32, 0), ("lap3d_80_f32", lambda: laplacian_3d(80, np.float32), {}, 256, 3),
         ## the creation paths beyond the default one
         ("lap2d_1000 host build", lambda: laplacian_2d(1000), {"SLQ_DEVICE_BUILD": "0"}, 256, 3), ("lap2d_1000 host build", None, {}, 64, 3),
         ("lap2d_1000 tiles 1", lambda: laplacian_2d(1000), {"SLQ_TILES": "1"}, 256, 3),
         ("lap3d_100 reorder 2, no tiles", lambda: laplacian_3d(100), {"SLQ_REORDER": "2", "SLQ_TILES": "0"}, 256, 3),
         ("random graph n=5e5", random_graph, {}, 64, 3),
         ("lap3d_100 from device arrays", lambda: on_device(laplacian_3d(100)), {}, 256, 3), ("lap3d_100 from device arrays", None, {}, 64, 6),
         ("affine lap2d_300 + 0.75 D", affine, {}, 64, 3), ("gram 120000 x 90000", gram, {}, 64, 3)]
import os
ops = {}
for name, make, env, P, orth in cases:
	env = ops[name][1] if name in ops else env  # (an operator and its plans are created under the same switches)
	saved = {k: os.environ.get(k) for k in env}
	os.environ.update(env)
	if name not in ops:
		t = time.perf_counter()
		ops[name] = (eng.DeviceOperator(make()), env)
		print(f"{name}: created in {time.perf_counter() - t:.3f} s", flush=True)
	plan = eng.LanczosPlan(ops[name][0], P, 30, orth)
	for k, v in saved.items():
		os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
	plan.generate_probes("rademacher", seed=77)
	plan.run()
	q = plan.quadrature("log")
	a, b, st = plan.tridiag()
	h = hashlib.sha256()
	for x in (a, b, q):
		h.update(np.ascontiguousarray(x).tobytes())
	info = plan.describe()
	print(f"{name} P={P} orth={orth} tiles={info['tiles']} seq={info['sequence']} sum={float(np.sum(q)):.12e} sha={h.hexdigest()[:16]}", flush=True)
	plan.close()
for op, _ in ops.values():
	op.close()

## the kernel-operator family (slq_kerneltile.hpp: one tile walk under the product, the cross products and the gradient update): sha256 of
## the operator's product (16 and 256 columns), of forward and adjoint cross products (m = 37 and 300 new points; 5 and 260 columns: the
## second column chunk and the slab sum) and, in fp64, of one gradient update of 65 columns (two chunks), at the pairs (n, d) = (300, 3),
## (5000, 20) - both coordinate depths; on a 256-unit chip every one of these is cut into several slabs - and (32768, 3), where 256 row
## blocks fill the chip: the product, the adjoint cross products and the gradient update run as ONE slab that writes the result directly
from primate_amd.operators import KernelOperator

def sha(*arrays):
	h = hashlib.sha256()
	for x in arrays:
		h.update(np.ascontiguousarray(x).tobytes())
	return h.hexdigest()[:16]

def side_objects(op, X, kernel, tag, dtype):
	"""The side objects of the C ABI at the small pair (n, d) = (300, 3) (their shared host paths): feature and adjoint
	feature products host-staged and - like everything below, in fp64 - through DeviceMatrix, point-gradient updates of both forms, the
	preconditioner's inv_sqrt both ways and its two exact trace parts, and one update each of an SddmmAccumulator, a DiagAccumulator and
	a DensityAccumulator."""
	import scipy.sparse as sp
	n, d, m, f2, b = X.shape[0], X.shape[1], 37, 45, 21
	r = np.random.default_rng(77)
	head = f"kernel {kernel} {tag} n={n} d={d}"
	cross = eng.KernelCross(op, r.standard_normal((m, d)).astype(dtype))
	fmap = eng.KernelFeatureMap(op, r.standard_normal((f2, d)).astype(dtype))
	Wf, Un, Um = r.standard_normal((2 * f2, b)).astype(dtype), r.standard_normal((n, b)).astype(dtype), r.standard_normal((m, b)).astype(dtype)
	print(f"{head} feature F2={f2} b={b} staged sha={sha(fmap.matmat(Wf))} rows sha={sha(fmap.matmat(Wf, rows=cross))} adjoint sha={sha(fmap.rmatmat(Un))} rows sha={sha(fmap.rmatmat(Um, rows=cross))}", flush=True)
	if dtype != np.float64:
		for x in (fmap, cross):
			x.close()
		return
	ctx = op.ctx
	F, N, M = eng.DeviceMatrix(2 * f2, 2 * b, ctx=ctx), eng.DeviceMatrix(n, 2 * b, ctx=ctx), eng.DeviceMatrix(m, 2 * b, ctx=ctx)
	F.set(0, Wf), N.set(0, Un), M.set(0, Um)
	fmap.matmat_dmat(F, 0, N, b, b)
	fmap.matmat_dmat(F, 0, M, b, b, rows=cross)
	got = [N.get(b, b), M.get(b, b)]
	fmap.rmatmat_dmat(N, 0, F, b, b)
	got.append(F.get(b, b))
	fmap.rmatmat_dmat(M, 0, F, b, b, rows=cross)
	got.append(F.get(b, b))
	print(f"{head} feature F2={f2} b={b} dmat sha={sha(got[0])} rows sha={sha(got[1])} adjoint sha={sha(got[2])} rows sha={sha(got[3])}", flush=True)
	pg, pgc = eng.KernelPointGradAccumulator(op), eng.KernelPointGradAccumulator(cross)
	N.set(b, r.standard_normal((n, b)))
	pg.update(N, 0, N, b, b, alpha=1.0, beta=0.0)
	pgc.update(M, 0, N, 0, b, alpha=1.0, beta=0.0)
	print(f"{head} point gradient m={b} training sha={sha(pg.get()[0])} cross sha={sha(pgc.get()[0])}", flush=True)
	pre = eng.DeviceOperator(KernelOperator(X, kernel, lengthscale=0.7 * np.sqrt(d), outputscale=1.3, noise=0.05).preconditioned(70), ctx=ctx)
	staged = pre.inv_sqrt(Un)
	pre.inv_sqrt_dmat(N, 0, N, b, b)
	acc, pacc = eng.KernelGradAccumulator(pre.base), eng.KernelPointGradAccumulator(pre.base)
	pre.precond_trace_grad(acc, 1.0, 0.0)
	pre.precond_trace_point_grad(pacc, 1.0, 0.0)
	print(f"{head} precond rank 70 inv_sqrt sha={sha(staged)} dmat sha={sha(N.get(b, b))} trace_grad sha={sha(acc.get()[0])} trace_point_grad sha={sha(pacc.get()[0])}", flush=True)
	pattern = sp.random(n, n, density=0.03, random_state=5, format="csr") + sp.identity(n, format="csr")
	sd = eng.SddmmAccumulator(pattern, ctx=ctx)
	sd.update(N, 0, N, b, b, alpha=0.5, beta=0.0, symmetric=True)
	plan = eng.LanczosPlan(op, 16, 20, 3, keep_basis=True)
	plan.generate_probes("rademacher", seed=5)
	plan.run()
	dg, dens = eng.DiagAccumulator(n, ctx=ctx), eng.DensityAccumulator("gaussian", np.linspace(0.0, 40.0, 33), bw=0.5, ctx=ctx)
	dg.update(plan, "log")
	dens.update(plan)
	print(f"{head} sddmm sha={sha(sd.get()[0])} diag sha={sha(*dg.get()[:3])} density sha={sha(*dens.get()[:3])}", flush=True)
	for x in (dens, dg, plan, sd, pacc, acc, pre, pgc, pg, F, N, M, fmap, cross):
		x.close()

rng = np.random.default_rng(2024)
for dtype, kernels in ((np.float64, ("rbf", "matern12", "matern32", "matern52")), (np.float32, ("rbf", "matern52"))):
	tag = "f64" if dtype == np.float64 else "f32"
	for kernel in kernels:
		for n, d in ((300, 3), (5000, 20), (32768, 3)):
			X = rng.standard_normal((n, d)).astype(dtype)
			op = eng.DeviceOperator(KernelOperator(X, kernel, lengthscale=0.7 * np.sqrt(d), outputscale=1.3, noise=0.05, dtype=dtype))
			for P in (16, 256):
				W = rng.standard_normal((n, P)).astype(dtype)
				Y = op.matmat(W)
				print(f"kernel {kernel} {tag} n={n} d={d} product P={P} sum={float(np.sum(Y, dtype=np.float64)):.12e} sha={sha(Y)}", flush=True)
			for m in (37, 300):
				cross = eng.KernelCross(op, rng.standard_normal((m, d)).astype(dtype))
				for b in (5, 260):
					F, A = cross.matmat(rng.standard_normal((n, b)).astype(dtype)), cross.matmat(rng.standard_normal((m, b)).astype(dtype), trans=True)
					print(f"kernel {kernel} {tag} n={n} d={d} cross m={m} b={b} forward sha={sha(F)} adjoint sha={sha(A)}", flush=True)
				cross.close()
			if dtype == np.float64:
				Z, V = eng.DeviceMatrix(n, 65, ctx=op.ctx), eng.DeviceMatrix(n, 65, ctx=op.ctx)
				Z.set(0, rng.standard_normal((n, 65)))
				V.set(0, rng.standard_normal((n, 65)))
				acc = eng.KernelGradAccumulator(op)
				acc.update(Z, 0, V, 0, 65, alpha=1.0, beta=0.0)
				vals, _ = acc.get()
				print(f"kernel {kernel} {tag} n={n} d={d} gradient m=65 sum={float(np.sum(vals)):.12e} sha={sha(vals)}", flush=True)
				for x in (acc, Z, V):
					x.close()
			if (n, d) == (300, 3):
				side_objects(op, X, kernel, tag, dtype)
			op.close()
