"""Cost of one spectral density update (slq_density_update: k_density_eval + k_density_fold) on BASELINE.json configs[1]
(2D Laplacian n = 1e6, k = 30, 256 probes, orth 3, fp64) with G = 1024 grid points, per kernel kind, next to the batch it
rides on (slq_plan_run + the QL). Wall times on the context stream; run it under `rocprofv3 --kernel-trace --stats -- python
scripts/time_density.py --kind <kind>` for the per-kernel device times DESIGN.md §4.9 quotes.

  python scripts/time_density.py [--kind gaussian|lorentzian|histogram|cdf|all] [--m 1000] [--grid 1024] [--reps 20]"""

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--kind", default="all")
	ap.add_argument("--m", type=int, default=1000)
	ap.add_argument("--grid", type=int, default=1024)
	ap.add_argument("--probes", type=int, default=256)
	ap.add_argument("--deg", type=int, default=30)
	ap.add_argument("--reps", type=int, default=20)
	a = ap.parse_args()
	from primate_amd.engine import DensityAccumulator, DeviceOperator, LanczosPlan, default_context

	T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(a.m, a.m))
	A = (sp.kron(sp.identity(a.m), T) + sp.kron(T, sp.identity(a.m))).tocsr()
	ctx = default_context()
	op = DeviceOperator(A, ctx=ctx)
	plan = LanczosPlan(op, a.probes, a.deg, 3)
	res = {"n": A.shape[0], "probes": a.probes, "deg": a.deg, "grid": a.grid}
	## the batch: probes + run + QL (what the bench's step does), warm, then timed
	for it in range(3):
		plan.generate_probes("rademacher", seed=it)
		ctx.synchronize()
		t0 = time.perf_counter()
		plan.run()
		plan.quadrature("log")
		t1 = time.perf_counter()
	res["batch_ms"] = 1e3 * (t1 - t0)
	kinds = ["gaussian", "lorentzian", "histogram", "cdf"] if a.kind == "all" else [a.kind]
	for kind in kinds:
		grid = np.linspace(-0.1, 8.1, a.grid + (1 if kind == "histogram" else 0))
		acc = DensityAccumulator(kind, grid, 8.2 / a.deg)
		acc.update(plan)  # (the rule of this run is current: the update is the two density kernels only)
		ctx.synchronize()
		t0 = time.perf_counter()
		for _ in range(a.reps):
			acc.update(plan)
		ctx.synchronize()
		t1 = time.perf_counter()
		mean, m2, out, cnt = acc.get()
		assert cnt == (a.reps + 1) * a.probes and np.all(np.isfinite(mean))
		res[kind] = {"update_ms": 1e3 * (t1 - t0) / a.reps, "share_of_batch": (t1 - t0) / a.reps / (res["batch_ms"] * 1e-3),
					 "integral_over_n": float(np.sum(mean) / A.shape[0]) if kind == "histogram" else None}
		acc.close()
	plan.close()
	op.close()
	print(json.dumps(res))


if __name__ == "__main__":
	main()
