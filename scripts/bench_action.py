"""bench_action.py - what f(A)X costs on a kept-basis plan and on a recompute plan (two-pass Lanczos).

    python scripts/bench_action.py --case c1 --basis keep|recompute [--reps 5] [--warmup 2] [--chunk P] [--out FILE]

One process measures one (case, basis): probes drawn on the device, `run + fun_action` left on the device
(slq_plan_fun_action_dmat: no n x P host copy in the timed region), wall time per repetition with the spread, then one
profiled repetition whose per-class kernel times give the breakdown (pass 1, coefficients, replay passes, accumulation
launches). With --basis keep it uses only entries that exist before this feature, so the same script times the parent
commit's library (run it with that tree first on sys.path). Cases:
    c1        configs[1]: 2-D Laplacian 1000^2, fp64, 256 probes, k = 30, orth 3
    l126f32   3-D Laplacian 126^3, fp32, 128 probes, k = 50, orth 3
    wide      3-D Laplacian 126^3, fp64, k = 50, orth 3, 256 columns of f(A)X: one 256-probe recompute plan, or kept-basis
              plans of --chunk probes each (the widest panel whose basis fits the memory allowed)
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
	sys.path.append(str(ROOT))  # (appended: a tree put on PYTHONPATH - the parent commit's - wins)

CASES = {
	"c1": dict(kind="lap2d", m=1000, dtype=np.float64, P=256, deg=30, orth=3),
	"l126f32": dict(kind="lap3d", m=126, dtype=np.float32, P=128, deg=50, orth=3),
	"wide": dict(kind="lap3d", m=126, dtype=np.float64, P=256, deg=50, orth=3),
}


def laplacian(kind: str, m: int, dtype):
	import scipy.sparse as sp

	T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
	I = sp.identity(m)
	if kind == "lap2d":
		A = sp.kron(I, T) + sp.kron(T, I)
	else:
		A = sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)
	A = A.tocsr().astype(dtype)
	A.sort_indices()
	return A


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--case", default="c1", choices=sorted(CASES))
	ap.add_argument("--basis", default="recompute", choices=["keep", "recompute"])
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--warmup", type=int, default=2)
	ap.add_argument("--chunk", type=int, default=0, help="probes per plan (default: all of the case's columns on one plan)")
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	from primate_amd import engine

	c = CASES[args.case]
	A = laplacian(c["kind"], c["m"], c["dtype"])
	n = A.shape[0]
	op = engine.DeviceOperator(A)
	ctx = op.ctx
	P, deg, orth = c["P"], c["deg"], c["orth"]
	chunk = args.chunk or P
	free0, total = ctx.meminfo()
	plan = engine.LanczosPlan(op, chunk, deg, orth, keep_basis=True) if args.basis == "keep" else engine.LanczosPlan(op, chunk, deg, orth, basis="recompute")
	fp64 = c["dtype"] == np.float64
	out = engine.DeviceMatrix(n, chunk, ctx=ctx) if fp64 else None  # (slq_plan_fun_action_dmat is an fp64 entry; fp32: the host copy is left out by timing the device)
	fun, kw = "exp", {"t": -0.1}

	def add(acc, pr):
		for k, v in pr.items():
			acc.setdefault(k, {"ms": 0.0, "launches": 0})
			acc[k]["ms"] += v["ms"]
			acc[k]["launches"] += v["launches"]

	def once(phases=None, split=None):
		"""f(A) X for all P columns, chunk by chunk; phases (a list) receives (run, action) device-synchronised wall times,
		split (two dicts) the profiled kernel classes of the run and of the action."""
		for c0 in range(0, P, chunk):
			t0 = time.perf_counter()
			plan.generate_probes("rademacher", seed=1234, probe_offset=c0)
			plan.run()
			if phases is not None:
				ctx.synchronize()
			if split is not None:
				add(split[0], plan.profile_read(reset=True))
			t1 = time.perf_counter()
			if out is not None:
				plan.fun_action_into(out, 0, fun, **kw)
			else:
				plan.fun_action(fun, **kw)
			ctx.synchronize()
			if phases is not None:
				phases.append((t1 - t0, time.perf_counter() - t1))
			if split is not None:
				add(split[1], plan.profile_read(reset=True))

	for _ in range(args.warmup):
		once()
	ctx.synchronize()
	times = []
	for _ in range(args.reps):
		t0 = time.perf_counter()
		once()
		ctx.synchronize()
		times.append(time.perf_counter() - t0)
	phases = []
	once(phases)
	plan.profile_enable(True)
	plan.profile_read(reset=True)
	split = ({}, {})
	once(split=split)
	plan.profile_enable(False)
	prof = split[1]
	esz = 8 if fp64 else 4
	vec = n * chunk * esz
	comb = prof["fun_combine"]
	nch = -(-P // chunk)
	## algorithmic panel passes of the combination per chunk: kept basis reads deg columns, reads and writes the output (deg + 2);
	## recompute reads deg columns and per launch reads (but the first) and writes the output
	launches = comb["launches"] / nch
	passes = (deg + 2) if args.basis == "keep" else (deg + 2 * launches - 1)
	rec = {
		"case": args.case, "basis": args.basis, "n": n, "dtype": "f64" if fp64 else "f32", "probes": P, "chunk": chunk, "deg": deg, "orth": orth,
		"workspace_GB": plan.workspace_bytes / 1e9, "free_GB_before": free0 / 1e9, "total_GB": total / 1e9,
		"describe": plan.describe(),
		"wall_s": {"min": min(times), "median": float(np.median(times)), "max": max(times), "all": times},
		"phases_s": {"run": sum(p[0] for p in phases), "action": sum(p[1] for p in phases)},
		"profiled_run_ms_by_class": {k: v for k, v in split[0].items() if v["launches"]},
		"profiled_action_ms_by_class": {k: v for k, v in split[1].items() if v["launches"]},
		"combine": {"launches_per_chunk": launches, "ms_per_chunk": comb["ms"] / nch, "panel_passes": passes,
					"algorithmic_TBps": passes * vec / (comb["ms"] / nch * 1e-3) / 1e12 if comb["ms"] > 0 else None},
	}  # fmt: skip
	line = json.dumps(rec)
	print(line)
	if args.out:
		Path(args.out).parent.mkdir(parents=True, exist_ok=True)
		with open(args.out, "a") as f:
			f.write(line + "\n")
	plan.close()
	op.close()


if __name__ == "__main__":
	main()
