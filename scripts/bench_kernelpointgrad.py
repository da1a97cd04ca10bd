"""bench_kernelpointgrad.py - what a point-gradient update of the kernel operator costs (slq_kernel_pointgrad_update):

 (a) one point-gradient update against one hyperparameter-gradient update (KernelGradAccumulator.update) of the same shape, in the
     same process and build: n = 16384, d = 3 and 16, m = 64 and 128, rbf and matern52, fp64. Three timings per shape: the
     hyperparameter update; the training form with Z and W two matrices (TWO one-sided passes per 64-column chunk); the training form
     with Z and W one matrix (ONE pass, twice its weight). A host clock around `inner` updates ended by the accumulator's synchronising
     read, over `inner`; median [min, max] of `reps` such windows after a warm-up window. per_pass_over_hyper is the ratio a pass
     costs: the two-pass median over twice the hyperparameter median, and the one-pass median over it.
 (b) what points=True adds to one gp.mll call: the setting of scripts/bench_gp_mll.py at n = 16384 (rbf, d = 3, rank 128,
     sigma2 = 1e-4, deg 20, 64 probes in batches of 16, the hyperparameters moved by 1 % before every call), the phase "points" of
     profile=True - the data-fit update, the batches' updates, the exact part where the control variate is on, the one read-back -
     against the call's total; and the total of the same calls without points.

    python scripts/bench_kernelpointgrad.py [--reps 5] [--inner 10] [--parts ab] [--out profiles/kernelpointgrad_bench.json]
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

from bench_kernelop import points, spread  # noqa: E402


def windows_ms(acc, update, reps, inner):
	"""ms per update: `reps` windows of `inner` updates, each ended by the synchronising get, after one warm-up window."""
	out = []
	for r in range(reps + 1):
		acc.get()
		t0 = time.perf_counter()
		for _ in range(inner):
			update()
		vals, _ = acc.get()
		dt = time.perf_counter() - t0
		if r:
			out.append(1e3 * dt / inner)
	assert np.all(np.isfinite(vals))
	return spread(out)


def part_a(eng, reps, inner):
	from primate_amd.operators import KernelOperator

	n, rows = 16384, []
	for name in ("rbf", "matern52"):
		for d in (3, 16):
			K = KernelOperator(points(n, d, np.float64), name, lengthscale=0.3 * np.sqrt(d / 3.0), noise=0.1)
			op = eng.DeviceOperator(K)
			for m in (64, 128):
				Z, W = eng.DeviceMatrix(n, m, ctx=op.ctx), eng.DeviceMatrix(n, m, ctx=op.ctx)
				Z.generate(0, m, "normal", seed=1)
				W.generate(0, m, "rademacher", seed=2)
				hacc, pacc = eng.KernelGradAccumulator(op), eng.KernelPointGradAccumulator(op)
				hyper = windows_ms(hacc, lambda: hacc.update(Z, 0, W, 0, m, alpha=1.0 / inner, beta=1.0), reps, inner)
				two = windows_ms(pacc, lambda: pacc.update(Z, 0, W, 0, m, alpha=1.0 / inner, beta=1.0), reps, inner)
				one = windows_ms(pacc, lambda: pacc.update(Z, 0, Z, 0, m, alpha=1.0 / inner, beta=1.0), reps, inner)
				S = eng.kernel_pointgrad_schedule(n, n, 256)
				rows.append(dict(kernel=name, n=n, d=d, m=m, launches_per_pass=-(-m // 64), slabs=S["slabs"], hyper_update_ms=hyper, point_update_two_pass_ms=two,
								 point_update_one_pass_ms=one, two_pass_over_hyper=two["median"] / hyper["median"], one_pass_over_hyper=one["median"] / hyper["median"],
								 per_pass_over_hyper=dict(two_pass=two["median"] / (2.0 * hyper["median"]), one_pass=one["median"] / hyper["median"])))  # fmt: skip
				for x in (hacc, pacc, Z, W):
					x.close()
			op.close()
	return rows


def part_b(reps):
	from primate_amd import gp
	from primate_amd.lanczos import _as_device_operator
	from primate_amd.operators import KernelOperator

	n = 16384
	rng = np.random.default_rng(n)
	X = rng.random((n, 3))
	y = np.sin(4.0 * X[:, 0]) * np.cos(3.0 * X[:, 1]) + 0.01 * rng.standard_normal(n)
	K = KernelOperator(X, "rbf", lengthscale=0.3, outputscale=1.0, noise=1e-4)
	B = K.preconditioned(128)
	res = {}
	for with_points in (False, True):
		totals, phases = [], []
		for rep in range(reps + 1):
			K.set_parameters(lengthscale=0.3 * (1.0 + 0.01 * rep))  # (the factor is stale: the call refreshes it)
			t = time.perf_counter()
			value, grads, info = gp.mll(B, y, deg=20, count=64, batch=16, seed=1, profile=True, points=with_points)
			total = 1e3 * (time.perf_counter() - t)
			if rep:  # (the first call is the warm-up)
				totals.append(total)
				phases.append(info["timing_ms"])
		res["points" if with_points else "plain"] = dict(total_ms=spread(totals), phases_ms={k: spread([p[k] for p in phases]) for k in phases[0]},
														 control_variate=info["logdet_info"]["control_variate"])  # fmt: skip
	res["points_phase_share_of_total"] = res["points"]["phases_ms"]["points"]["median"] / res["points"]["total_ms"]["median"]
	res["total_points_over_plain"] = res["points"]["total_ms"]["median"] / res["plain"]["total_ms"]["median"]
	res["config"] = dict(n=n, kernel="rbf", d=3, lengthscale=0.3, rank=128, noise=1e-4, deg=20, count=64, batch=16)
	res["max_abs_points"] = float(np.max(np.abs(grads["points"])))
	for obj in (B, K):
		_as_device_operator(obj, dtype=np.float64).close()
	return res


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
		res["a_point_update_vs_hyper_update"] = part_a(eng, a.reps, a.inner)
	if "b" in a.parts:
		res["b_points_share_of_gp_mll"] = part_b(a.reps)
	line = json.dumps(res)
	print(line)
	if a.out:
		Path(a.out).parent.mkdir(parents=True, exist_ok=True)
		Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
	main()
