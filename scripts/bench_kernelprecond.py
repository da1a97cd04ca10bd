"""bench_kernelprecond.py - what the pivoted-Cholesky preconditioner of the kernel operator costs (slq_kernel_precond_*).

rbf, d = 3, fp64, rank 128, noise 1e-4. The method is bench_kernelop.py's: every figure is 5 runs after a warm-up run, reported as
median [min, max].

  (a) factor   n = 16384 and 262144: slq_kernel_precond_refresh, the whole refactorisation in place. `device_ms` is the wall time of
               the launches up to the one synchronisation (the rank_max column steps and the Gram matrix L^T L), `host_ms` the host
               part behind it (Jacobi on the 128 x 128 Gram matrix, G, its upload), `refresh_ms` the call as the caller sees it.
  (b) step     n = 16384, P = 128 probes: the plan's profile (class spmm_3term: the operator's share of a step - for the
               preconditioned operator the two applies of M and the base's product -, over the 10 steps of a run) of the
               preconditioned operator against the plain kernel operator of the same build in the same process, and the ratio of
               the medians; `apply_ms` is one apply of M on the same 128 columns through slq_kernel_precond_apply_dmat (10 calls
               per window), `wall_ms_per_step` the whole run's wall time over its steps for both operators.

    python scripts/bench_kernelprecond.py [--out profiles/kernelprecond_bench.json] [--quick 1]
Prints one JSON line; --out writes it to a file. ((c), nothing existing moved, is bench.py itself on two trees.)"""

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

RUNS, STEPS = 5, 10
RANK, NOISE, D = 128, 1e-4, 3


def spread(v):
	v = sorted(v)
	return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def points(n, d, seed=0):
	return np.random.default_rng(n + d + seed).random((n, d))


def factor_times(eng, ctx, n):
	from primate_amd.operators import KernelOperator

	K = KernelOperator(points(n, D), "rbf", lengthscale=0.3, noise=NOISE)
	op = eng.DeviceOperator(K.preconditioned(RANK), ctx=ctx)
	try:
		dev, host, wall = [], [], []
		for r in range(RUNS + 1):
			ctx.synchronize()
			t0 = time.perf_counter()
			op.refresh()
			t = 1e3 * (time.perf_counter() - t0)
			ft = op.factor_timing()
			if r:
				dev.append(ft["device_ms"]), host.append(ft["host_ms"]), wall.append(t)
		info = op.info()
		return dict(n=n, d=D, rank_max=RANK, rank=info["rank"], residual_trace=info["residual_trace"], device_ms=spread(dev), host_ms=spread(host), refresh_ms=spread(wall))
	finally:
		op.close()


def step_times(eng, ctx, op, P):
	"""(profile ms per step of class spmm_3term, wall ms per step) over RUNS runs of STEPS steps after a warm-up run."""
	plan = eng.LanczosPlan(op, P, STEPS, 0)
	try:
		prof, wall = [], []
		plan.profile_enable(True)
		for r in range(RUNS + 1):
			plan.generate_probes("rademacher", seed=r)
			plan.run()
			pr = plan.profile_read()["spmm_3term"]
			if r:
				prof.append(pr["ms"] / STEPS)
		plan.profile_enable(False)
		for r in range(RUNS + 1):
			plan.generate_probes("rademacher", seed=r)
			ctx.synchronize()
			t0 = time.perf_counter()
			plan.run()
			ctx.synchronize()
			if r:
				wall.append(1e3 * (time.perf_counter() - t0) / STEPS)
		return spread(prof), spread(wall)
	finally:
		plan.close()


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--out", default=None)
	ap.add_argument("--quick", type=int, default=0, help="1: n = 2048 everywhere (a check that the script runs)")
	a = ap.parse_args()
	from primate_amd import engine as eng
	from primate_amd.operators import KernelOperator

	ctx = eng.default_context()
	res = dict(runs=RUNS, steps_per_run=STEPS, warmup_runs=1, profile="rbf", d=D, rank=RANK, noise=NOISE, factor=[], step=None)
	for n in (2048,) if a.quick else (16384, 262144):
		row = factor_times(eng, ctx, n)
		res["factor"].append(row)
		print(json.dumps(row), file=sys.stderr, flush=True)
	n, P = (2048 if a.quick else 16384), 128
	K = KernelOperator(points(n, D), "rbf", lengthscale=0.3, noise=NOISE)
	plain = eng.DeviceOperator(K, ctx=ctx)
	pre = eng.DeviceOperator(K.preconditioned(RANK), ctx=ctx)
	try:
		p_plain, w_plain = step_times(eng, ctx, plain, P)
		p_pre, w_pre = step_times(eng, ctx, pre, P)
		IN, OUT = eng.DeviceMatrix(n, P, ctx=ctx), eng.DeviceMatrix(n, P, ctx=ctx)
		IN.set(0, np.asfortranarray(np.random.default_rng(1).standard_normal((n, P))))
		ap_ms = []
		for r in range(RUNS + 1):
			ctx.synchronize()
			t0 = time.perf_counter()
			for _ in range(STEPS):
				pre.inv_sqrt_dmat(IN, 0, OUT, 0, P)
			ctx.synchronize()
			if r:
				ap_ms.append(1e3 * (time.perf_counter() - t0) / STEPS)
		IN.close(), OUT.close()
		res["step"] = dict(n=n, P=P, plain_ms=p_plain, precond_ms=p_pre, ratio=p_pre["median"] / p_plain["median"], apply_ms=spread(ap_ms),
						   wall_ms_per_step=dict(plain=w_plain, precond=w_pre, ratio=w_pre["median"] / w_plain["median"]))  # fmt: skip
	finally:
		pre.close()
		plain.close()
	line = json.dumps(res)
	print(line)
	if a.out:
		Path(a.out).parent.mkdir(parents=True, exist_ok=True)
		Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
	main()
