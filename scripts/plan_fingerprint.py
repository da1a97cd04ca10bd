"""Fingerprint of what a plan's creation decides (geometry, grids, tile stream, ring, workspace) through what it reports and produces:
per plan one line with describe(), the basis mode, the workspace bytes, the dense path and a sha256 of the outputs of one seeded run.
The companion of scripts/op_fingerprint.py for plans: two libraries that print the same lines create the same plans (first use: that
slq_plan_shape.hpp leaves every plan and every result bitwise unchanged).   PRIMATE_AMD_LIBSLQ=<other library> python scripts/plan_fingerprint.py"""
import hashlib, sys
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
from conftest import laplacian_2d, laplacian_3d
from primate_amd import engine as eng

def sha(*arrays):
	h = hashlib.sha256()
	for x in arrays:
		h.update(np.ascontiguousarray(x).tobytes())
	return h.hexdigest()[:16]

def line(name, plan, outs, basis_used="-"):
	d = plan.describe() if plan is not None else {}
	info = " ".join(f"{k}={d[k]}" for k in ("panel_width", "panels", "ring_slots", "sequence", "pipelined", "tiles", "omega", "dense_kernel", "dense_ksplit") if k in d)
	mode, ws = (plan.basis_mode, plan.workspace_bytes) if plan is not None else ("-", "-")
	print(f"{name}: {info} basis_mode={mode} workspace_bytes={ws} basis_used={basis_used} sha={sha(*outs)}", flush=True)

def probes(n, P, dtype=np.float64):
	rng = np.random.default_rng(2024)
	return np.asfortranarray(np.floor(rng.random((n, P)) * 2) * 2 - 1, dtype=dtype)

def dense(n, dtype):
	M = np.random.default_rng(5).standard_normal((n, n))
	return ((M + M.T) / np.sqrt(2 * n) + 3.0 * np.eye(n)).astype(dtype)  # (positive definite: log is defined)

def gram():
	from primate_amd.operators import GramOperator
	import scipy.sparse as sp
	rng = np.random.default_rng(9)
	m = 65000
	B = sp.coo_matrix((rng.uniform(0.5, 1.5, m), (rng.integers(0, 12000, m), rng.integers(0, 9000, m))), shape=(12000, 9000)) + sp.eye(12000, 9000) * 3.0
	return GramOperator(B.tocsr())

lap = eng.DeviceOperator(laplacian_2d(300))
n = lap.shape[0]
# action plans on one CSR operator: recompute, kept basis
for basis, P in (("recompute", 64), ("recompute", 16), ("keep", 64)):
	plan = eng.LanczosPlan(lap, P, 30, 3, basis=basis)
	plan.set_probes(probes(n, P))
	plan.run()
	a, b, st = plan.tridiag()
	line(f"lap2d_300 {basis} action P={P}", plan, (a, b, plan.fun_action("exp", t=-0.1)))
	plan.close()
# Chebyshev moments and the Chebyshev action
coef = np.linspace(1.0, 0.05, 41)
plan = eng.ChebyshevPlan(lap, 64, 40)
plan.set_probes(probes(n, 64))
plan.run((0.0, 8.1))
line("lap2d_300 chebyshev moments P=64", plan, (plan.moments(),))
plan.close()
plan = eng.ChebyshevPlan(lap, 64, 40, action=True)
plan.set_probes(probes(n, 64))
line("lap2d_300 chebyshev action P=64", plan, (plan.action((0.0, 8.1), coef), plan.moments()))
plan.close()
# the one-shot entries, which chunk their probes by the byte estimates; automatic basis mode
q = eng.quad_batch(lap, probes(n, 96), 30, 3, fun="log")
line("lap2d_300 quad_batch P=96", None, (q,))
Y, used = eng.fun_action_batch(lap, probes(n, 48), 30, 3, fun="exp", t=-0.1, basis="auto", return_basis=True)
line("lap2d_300 fun_action_batch auto P=48", None, (Y,), used)
lap.close()
# dense fp64 and fp32, a Gram operator
for name, A, dtype, P in (("dense_1000 f64", dense(1000, np.float64), np.float64, 64), ("dense_1000 f64", None, np.float64, 16), ("dense_1000 f32", dense(1000, np.float32), np.float32, 64),
                          ("gram 12000 x 9000", gram(), np.float64, 64)):
	if A is not None:
		op = eng.DeviceOperator(A, dtype=dtype)
	plan = eng.LanczosPlan(op, P, 30, 3)
	plan.set_probes(probes(op.shape[0], P, dtype))
	plan.run()
	a, b, st = plan.tridiag()
	line(f"{name} P={P}", plan, (a, b, plan.quadrature("log")))
	plan.close()
	if name.startswith("dense") and A is not None:  # (once per dense operator)
		line(f"{name} quad_batch P=40", None, (eng.quad_batch(op, probes(op.shape[0], 40, dtype), 30, 3, fun="log"),))
