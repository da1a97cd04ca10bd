"""What a Chebyshev step costs next to a Lanczos step: the HIP-event time per step of a Chebyshev run and,
in the same process on the same operator and panel geometry, of the orth-0 and orth-3 Lanczos runs. Operators: BASELINE.json
configs[1] (2-D Laplacian, n = 1e6) and the 100^3 grid, at 256 and 64 probes, fp64, `--steps` steps each.

The time of a step is the sum of the per-kernel event times of a run (slq_plan_profile_*: every launch bracketed by two
events, probe generation left out) divided by the steps; five repeats, the median and the spread (max - min) reported.

The one condition checked: a Chebyshev step launches a strict subset of the orth-0 Lanczos step - its update pass and one
finalize kernel - so its time must not exceed the orth-0 step's by more than the run-to-run spread. If it does, a launch too
many has crept in (exit status 1). Both ratios and the moments per second go into the JSON line.

  python scripts/time_chebyshev.py [--op lap2d|lap3d] [--probes 256] [--steps 30] [--reps 5] [--out profiles/chebyshev_step.json]"""

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def laplacian(kind: str) -> sp.csr_matrix:
	m = 1000 if kind == "lap2d" else 100
	T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
	I = sp.identity(m)
	A = (sp.kron(I, T) + sp.kron(T, I)) if kind == "lap2d" else (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T))
	A = A.tocsr()
	A.sort_indices()
	return A


def step_times(plan, run, steps: int, reps: int) -> dict:
	"""Per-step device time (ms) of `reps` runs after one warm run: median, min, max, launches per step, ms per kernel class."""
	times, last = [], None
	plan.profile_enable(True)
	for it in range(reps + 1):
		plan.generate_probes("rademacher", seed=it)
		plan.profile_read(reset=True)  # (drops the probe kernels' events)
		run()
		last = plan.profile_read(reset=True)
		if it > 0:
			times.append(sum(v["ms"] for k, v in last.items() if k != "probes") / steps)
	plan.profile_enable(False)
	launches = sum(v["launches"] for k, v in last.items() if k != "probes")
	return {"ms": float(np.median(times)), "min": min(times), "max": max(times), "spread": max(times) - min(times),
	        "launches_per_step": launches / steps, "classes_ms_per_step": {k: v["ms"] / steps for k, v in last.items() if v["launches"]}}  # fmt: skip


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--op", default="lap2d", choices=("lap2d", "lap3d"))
	ap.add_argument("--probes", type=int, default=256)
	ap.add_argument("--steps", type=int, default=30)
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--out", default=None, help="append the result line to this JSON-lines file")
	a = ap.parse_args()
	from primate_amd.chebyshev import spectral_bounds
	from primate_amd.engine import ChebyshevPlan, DeviceOperator, LanczosPlan, default_context

	A = laplacian(a.op)
	ctx = default_context()
	op = DeviceOperator(A, ctx=ctx)
	bounds = spectral_bounds(A)
	res = {"op": a.op, "n": A.shape[0], "nnz": int(A.nnz), "probes": a.probes, "steps": a.steps, "reps": a.reps, "dtype": "f64"}
	cheb = ChebyshevPlan(op, a.probes, a.steps)
	res["describe"] = {k: v for k, v in cheb.describe().items() if k in ("panel_width", "panels", "sequence", "tiles", "pipelined")}
	res["chebyshev"] = step_times(cheb, lambda: cheb.run(bounds), a.steps, a.reps)
	mu, flags = cheb.moments(return_outside=True)
	assert not flags.any() and np.all(np.isfinite(mu))
	res["max_excess"] = float(np.max(np.abs(mu) / mu[:, :1] - 1.0))
	cheb.close()
	for orth in (0, 3):
		lan = LanczosPlan(op, a.probes, a.steps, orth)
		res[f"lanczos_orth{orth}"] = step_times(lan, lambda: lan.run(), a.steps, a.reps)
		lan.close()
	op.close()
	c, l0, l3 = res["chebyshev"], res["lanczos_orth0"], res["lanczos_orth3"]
	res["ratio_vs_orth0"] = c["ms"] / l0["ms"]
	res["ratio_vs_orth3"] = c["ms"] / l3["ms"]
	res["moments_per_second"] = 2.0 * a.probes / (c["ms"] * 1e-3)
	spread = max(c["spread"], l0["spread"])
	res["subset_ok"] = bool(c["ms"] <= l0["ms"] + spread and c["launches_per_step"] < l0["launches_per_step"])
	line = json.dumps(res)
	print(line)
	if a.out:
		with open(a.out, "a") as f:
			f.write(line + "\n")
	return 0 if res["subset_ok"] else 1


if __name__ == "__main__":
	sys.exit(main())
