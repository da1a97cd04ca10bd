"""bench_kernelgrad.py - what a hyperparameter-gradient update of the kernel operator costs (slq_kernel_grad_update):

 (a) one update against one operator product of the same n and column count: n = 16384, d = 3 and 16, m = 64 and 128, rbf and
     matern52, fp64. The update: a host clock around `inner` updates ended by the accumulator's synchronising read, over `inner`;
     median [min, max] of `reps` such windows after a warm-up window. The product: the plan's own profile (class spmm_3term) as
     scripts/bench_kernelop.py takes it, from the same process. Both have the 2 n^2 (d_pad + m) matrix-core flops; the update
     evaluates a second profile value per pair and 3 d_pad VALU operations per pair for the differences.
 (b) what a gradient costs its user: n = 16384, d = 3, rbf, deg = 30, 64 device-drawn probes, a kept-basis plan - seconds for the
     Lanczos run with its quadrature, for the action f'(A) V, and for the update, each ended by a synchronise.

    python scripts/bench_kernelgrad.py [--reps 5] [--inner 10] [--parts ab] [--out profiles/kernelgrad_bench.json]
Prints one JSON line; --out writes it to a file."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "scripts"):
	if not any(Path(q).resolve() == p for q in sys.path if q):
		sys.path.append(str(p))

from bench_kernelop import PEAK, points, product_ms, spread  # noqa: E402


def update_ms(eng, op, n, m, reps, inner):
	"""ms per update: `reps` windows of `inner` updates, each ended by the synchronising get, after one warm-up window."""
	Z, W = eng.DeviceMatrix(n, m, ctx=op.ctx), eng.DeviceMatrix(n, m, ctx=op.ctx)
	Z.generate(0, m, "normal", seed=1)
	W.generate(0, m, "rademacher", seed=2)
	acc = eng.KernelGradAccumulator(op)
	try:
		out = []
		for r in range(reps + 1):
			acc.get()
			t0 = time.perf_counter()
			for _ in range(inner):
				acc.update(Z, 0, W, 0, m, alpha=1.0 / inner, beta=1.0)
			vals, _ = acc.get()
			dt = time.perf_counter() - t0
			if r:
				out.append(1e3 * dt / inner)
		assert np.all(np.isfinite(vals))
		return spread(out)
	finally:
		for x in (acc, Z, W):
			x.close()


def part_a(eng, reps, inner):
	from primate_amd.operators import KernelOperator

	n, rows = 16384, []
	for name in ("rbf", "matern52"):
		for d in (3, 16):
			K = KernelOperator(points(n, d, np.float64), name, lengthscale=0.3 * np.sqrt(d / 3.0), noise=0.1)
			op = eng.DeviceOperator(K)
			for m in (64, 128):
				prod = product_ms(eng, op, m, reps)
				upd = update_ms(eng, op, n, m, reps, inner)
				dpad = (d + 3) // 4 * 4
				flops = 2.0 * n * n * (dpad + m)
				rows.append(dict(kernel=name, n=n, d=d, m=m, launches=-(-m // 64), update_ms=upd, product_ms=prod, update_over_product=upd["median"] / prod["median"],
								 mfma_flops=flops, update_tflops=flops / (upd["median"] * 1e-3) / 1e12, update_frac_of_matrix_peak=flops / (upd["median"] * 1e-3) / PEAK["float64"]))  # fmt: skip
			op.close()
	return rows


def part_b(eng, reps):
	from primate_amd.operators import KernelOperator, MatrixFunction

	n, d, P, deg = 16384, 3, 64, 30
	K = KernelOperator(points(n, d, np.float64), "rbf", lengthscale=0.3, noise=0.1)
	M = MatrixFunction(K, "log", deg=deg, orth=3)
	ctx = M._op.ctx
	plan = M._plan(P, True)
	W, Z = eng.DeviceMatrix(n, P, ctx=ctx), eng.DeviceMatrix(n, P, ctx=ctx)
	acc = eng.KernelGradAccumulator(M._op)
	run_s, act_s, upd_s = [], [], []
	try:
		for r in range(reps + 1):
			plan.generate_probes("rademacher", seed=r)
			plan.get_probes_into(W, 0)
			ctx.synchronize()
			t0 = time.perf_counter()
			plan.run(M._rtol)
			plan.quadrature("log")
			t1 = time.perf_counter()
			plan.fun_action_into(Z, 0, "inv")
			ctx.synchronize()
			t2 = time.perf_counter()
			acc.update(Z, 0, W, 0, P, alpha=1.0 / P, beta=0.0)
			vals, _ = acc.get()
			t3 = time.perf_counter()
			if r:
				run_s.append(t1 - t0), act_s.append(t2 - t1), upd_s.append(t3 - t2)
		run, act, upd = spread(run_s), spread(act_s), spread(upd_s)
		return dict(n=n, d=d, P=P, deg=deg, orth=3, basis=plan.basis_kind, run_and_quadrature_s=run, action_s=act, update_s=upd,
					update_over_run=upd["median"] / run["median"], gradient_over_run=(act["median"] + upd["median"]) / run["median"],
					grads=[float(v) for v in vals])  # fmt: skip
	finally:
		for x in (acc, W, Z):
			x.close()


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--inner", type=int, default=10)
	ap.add_argument("--parts", default="ab")
	ap.add_argument("--out", default=None)
	a = ap.parse_args()
	from primate_amd import engine as eng

	res = dict(reps=a.reps, warmup_windows=1, updates_per_window=a.inner)
	if "a" in a.parts:
		res["a_update_vs_product"] = part_a(eng, a.reps, a.inner)
	if "b" in a.parts:
		res["b_gradient_vs_lanczos_batch"] = part_b(eng, a.reps)
	line = json.dumps(res)
	print(line)
	if a.out:
		Path(a.out).parent.mkdir(parents=True, exist_ok=True)
		Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
	main()
