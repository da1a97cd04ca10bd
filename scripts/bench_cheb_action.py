"""bench_cheb_action.py - what the Chebyshev action p(A) X costs (engine.ChebyshevPlan(action=True)).

    python scripts/bench_cheb_action.py [--m 1000] [--probes 256] [--deg 60] [--reps 5] [--warmup 2] [--profiled 3] [--out FILE]

configs[1]'s operator (2-D Laplacian m^2, fp64), exp(-0.1 x) at degree `deg` on the Gershgorin bounds: probes drawn on the
device, the result left on the device (slq_plan_chebyshev_action_dmat: no n x P host copy in the timed region). Wall time per
action with the spread, then `profiled` profiled repetitions of (a) the action and (b) a plain moments run of the same plan
(slq_plan_run_chebyshev: the same steps without the accumulation launches), whose per-class kernel times give update passes,
k_fin_cheb and accumulation, the update pass's time per step in both, and the accumulation kernel's rate over the panel passes
it moves (per launch nc reads, one write and - but for the first - one read of the output). The columns per launch are a
compile-time constant of the library: PRIMATE_AMD_LIBSLQ points at a build with another -DSLQ_CHEB_ACC_COLS.
Prints one JSON line; --out appends it to a file."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if not any(Path(p).resolve() == ROOT for p in sys.path if p):
	sys.path.append(str(ROOT))


def laplacian2d(m: int):
	import scipy.sparse as sp

	T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
	A = (sp.kron(sp.identity(m), T) + sp.kron(T, sp.identity(m))).tocsr().astype(np.float64)
	A.sort_indices()
	return A


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--m", type=int, default=1000)
	ap.add_argument("--probes", type=int, default=256)
	ap.add_argument("--deg", type=int, default=60)
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--warmup", type=int, default=2)
	ap.add_argument("--profiled", type=int, default=3)
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	from primate_amd import _capi, engine
	from primate_amd.chebyshev import chebyshev_coefficients, spectral_bounds

	A = laplacian2d(args.m)
	n, P, deg = A.shape[0], args.probes, args.deg
	bounds = spectral_bounds(A, "gershgorin")
	coef = chebyshev_coefficients("exp", deg + 1, bounds, t=-0.1)
	op = engine.DeviceOperator(A)
	ctx = op.ctx
	plan = engine.ChebyshevPlan(op, P, deg, action=True)
	plain = engine.ChebyshevPlan(op, P, deg)
	out = engine.DeviceMatrix(n, P, ctx=ctx)
	d = plan.describe()
	K, S = d["acc_cols"], d["ring_slots"]

	def action():
		plan.generate_probes("rademacher", seed=1234)
		plan.action_into(bounds, coef, out, 0)  # (synchronises)

	def moments(pl):
		pl.generate_probes("rademacher", seed=1234)
		pl.run(bounds)
		ctx.synchronize()

	for _ in range(args.warmup):
		action()
	times = []
	for _ in range(args.reps):
		t0 = time.perf_counter()
		action()
		times.append((time.perf_counter() - t0) * 1e3)

	def profiled(pl, fn):
		pl.profile_enable(True)
		pl.profile_read(reset=True)
		rows = []
		for _ in range(args.profiled):
			fn()
			rows.append({k: v for k, v in pl.profile_read(reset=True).items() if v["launches"]})
		pl.profile_enable(False)
		return rows

	plan.action_columns(reset=True)
	prof_action = profiled(plan, action)
	read, offered = plan.action_columns(reset=True)
	moments(plan)
	moments(plain)
	prof_same = profiled(plan, lambda: moments(plan))
	prof_plain = profiled(plain, lambda: moments(plain))

	vec = n * P * 8
	launches = prof_action[0]["fun_combine"]["launches"]
	## panel passes of the accumulation per action: every column read once, the output written per launch and read per launch but the first
	passes = read / args.profiled + 2 * launches - 1

	def per_step(rows):
		return [r["axpy_norm"]["ms"] / r["axpy_norm"]["launches"] for r in rows]  # (launches: the steps and the probes' norm sweep)

	acc_ms = [r["fun_combine"]["ms"] for r in prof_action]
	rec = {
		"bench": "cheb_action", "lib": str(_capi.LIB_PATH), "n": n, "probes": P, "deg": deg, "acc_cols": K, "ring_slots": S, "describe": d,
		"panels": S + 1, "panel_GB": vec / 1e9, "workspace_GB": plan.workspace_bytes / 1e9, "plain_workspace_GB": plain.workspace_bytes / 1e9,
		"action_ms": {"min": min(times), "median": float(np.median(times)), "max": max(times), "all": times},
		"profiled_action_ms_by_class": prof_action,
		"profiled_moments_same_plan_ms_by_class": prof_same,
		"profiled_moments_plain_plan_ms_by_class": prof_plain,
		"update_ms_per_launch": {"action": per_step(prof_action), "moments_same_plan": per_step(prof_same), "moments_plain_plan": per_step(prof_plain)},
		"accumulate": {"launches": launches, "columns_read": read / args.profiled, "columns_offered": offered / args.profiled, "panel_passes": passes,
					   "ms": acc_ms, "TBps": [passes * vec / (ms * 1e-3) / 1e12 for ms in acc_ms]},
	}  # fmt: skip
	line = json.dumps(rec)
	print(line)
	if args.out:
		Path(args.out).parent.mkdir(parents=True, exist_ok=True)
		with open(args.out, "a") as f:
			f.write(line + "\n")
	for x in (plan, plain, out, op):
		x.close()


if __name__ == "__main__":
	main()
