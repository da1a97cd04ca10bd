"""bench_gp_features.py - what the adjoint feature product and `gp.feature_posterior` cost (slq_kernel_feature_rdmat),
with the method of bench_gp_paths.py: 5 runs after a warm-up, median [min, max].

 (a) one adjoint product Z = Phi^T U between device matrices at the operator's points: n = 16384, d = 3, rbf, fp64, F2 = 1024 and
     4096, b = 64 (slq_kernel_feature_rdmat: 10 launches closed by one synchronisation, the wall time over 10). The yardstick is the
     FORWARD product at the same shape - its time from profiles/gp_paths_bench.json, and measured again in this process - and the flop
     model 2 n F2 (d_pad + 2 b), which is the same for both directions. Reported: the ratio, the Tflop/s, the slab count and the
     workgroups launched.
 (b) `gp.feature_posterior` end to end at n = 16384 and 65536 with F2 = 1024: the wall time of the call and of the Gram build inside it
     (timed on its own, same map), the share of the Gram build, and `gp.posterior`'s solve at the same n (m = 64 new points,
     variance=False, deg = 60) beside it.
 (c) with --parent DIR (a checkout of the parent commit with its own library built): `python bench.py --gpus 1 --steps 5 --warmup 2` in
     that tree and in this one, alternating three times, each run a child process of its own under its own time limit; the first failure
     ends the part. The six lines (probe-matvecs/s, ms per step, the estimate) go to --ab-out. bench.py itself is not touched.

    python scripts/bench_gp_features.py [--reps 5] [--parts ab] [--out profiles/gp_features_bench.json]
    python scripts/bench_gp_features.py --parts c --parent DIR --ab-out profiles/gp_features_bench_ab.txt
Prints one JSON line; --out writes it to a file. No rocprofv3 trace and no counters are taken: the times are host clocks around
stream-ordered windows."""

from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if not any(Path(p).resolve() == ROOT for p in sys.path if p):
	sys.path.append(str(ROOT))

PEAK_F64 = 78.6e12


def spread(v):
	v = sorted(v)
	return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def points(n, d, dtype):
	return np.random.default_rng(n + d).random((n, d)).astype(dtype)


def forward_ms_on_record(n, f2, b):
	"""The forward product's median ms at the same shape from profiles/gp_paths_bench.json; None where it has no such row."""
	try:
		rows = json.loads((ROOT / "profiles" / "gp_paths_bench.json").read_text())["a_feature_product"]
	except (OSError, KeyError, ValueError):
		return None
	for r in rows:
		if r["dtype"] == "float64" and r["n"] == n and r["F2"] == f2 and r["b"] == b:
			return r["ms"]["median"]
	return None


def timed(ctx, reps, launch):
	ms = []
	for r in range(reps + 1):
		ctx.synchronize()
		t0 = time.perf_counter()
		for _ in range(10):
			launch()
		ctx.synchronize()
		if r:
			ms.append(1e3 * (time.perf_counter() - t0) / 10)
	return ms


def part_a(eng, reps):
	from primate_amd.operators import KernelOperator

	n, d, dpad, b = 16384, 3, 4, 64
	out = []
	K = KernelOperator(points(n, d, np.float64), "rbf", lengthscale=0.3, outputscale=1.5, noise=0.1)
	op = eng.DeviceOperator(K)
	for f2 in (1024, 4096):
		fmap = K.features(f2, seed=1).device(op)
		Wd, Ud, Yd, Zd = (eng.DeviceMatrix(r, b, ctx=op.ctx) for r in (2 * f2, n, n, 2 * f2))
		Wd.set(0, np.random.default_rng(f2).standard_normal((2 * f2, b)))
		Ud.set(0, np.random.default_rng(f2 + 1).standard_normal((n, b)))
		adj = timed(op.ctx, reps, lambda: fmap.rmatmat_dmat(Ud, 0, Zd, 0, b))
		fwd = timed(op.ctx, reps, lambda: fmap.matmat_dmat(Wd, 0, Yd, 0, b))
		flops = 2.0 * n * f2 * (dpad + 2 * b)
		S, Sf = eng.kernel_feature_adjoint_schedule(f2, n, b, 256, np.float64), eng.kernel_feature_schedule(n, f2, b, 256, np.float64)
		rec = forward_ms_on_record(n, f2, b)
		row = dict(dtype="float64", n=n, d=d, F2=f2, b=b, entry="rdmat (device to device)", ms=spread(adj), forward_ms_now=spread(fwd), forward_ms_on_record=rec,
				   mfma_flops=flops, tflops=flops / (np.median(adj) * 1e-3) / 1e12, frac_of_matrix_peak=flops / (np.median(adj) * 1e-3) / PEAK_F64,
				   forward_tflops_now=flops / (np.median(fwd) * 1e-3) / 1e12, adjoint_over_forward_now=float(np.median(adj) / np.median(fwd)),
				   adjoint_over_forward_on_record=None if rec is None else float(np.median(adj)) / rec, slabs=S["slabs"], row_blocks=S["nrb"], col_blocks=S["col_blocks"],
				   chunks=S["chunks"], workgroups=S["nrb"] * S["chunks"] * S["slabs"], partial_panel_bytes=S["slabs"] * 2 * f2 * b * 8 if S["slabs"] > 1 else 0,
				   forward_workgroups=Sf["nrb"] * Sf["chunks"] * Sf["slabs"])  # fmt: skip
		out.append(row)
		for o in (Wd, Ud, Yd, Zd, fmap):
			o.close()
	op.close()
	return out


def part_b(eng, reps):
	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	out = []
	for n in (16384, 65536):
		X = points(n, 3, np.float64)
		y = np.sin(6 * X[:, 0]) * np.cos(4 * X[:, 1]) + 0.3 * np.random.default_rng(1).standard_normal(n)
		K = KernelOperator(X, "rbf", lengthscale=0.3, outputscale=1.5, noise=0.1)
		op = eng.DeviceOperator(K)
		Xnew = points(64, 3, np.float64)[::-1].copy()
		Ft = K.features(1024, seed=3)
		total, gram, pred = [], [], []
		for r in range(reps + 1):
			op.ctx.synchronize()
			t0 = time.perf_counter()
			post = gp.feature_posterior(K, y, features=Ft)
			t1 = time.perf_counter()
			mean, var = post.predict(Xnew)
			t2 = time.perf_counter()
			post._fmap.gram()
			t3 = time.perf_counter()
			mll, finite = post.mll, bool(np.all(np.isfinite(mean)) and np.all(np.isfinite(var)))
			post.close()
			if r:
				total.append(1e3 * (t1 - t0)), pred.append(1e3 * (t2 - t1)), gram.append(1e3 * (t3 - t2))
		solve = []
		for r in range(3):  # (a warm-up call, then two timed ones: the exact solve is the slow side)
			op.ctx.synchronize()
			t0 = time.perf_counter()
			gp.posterior(K, y, Xnew, deg=60, variance=False)
			if r:
				solve.append(1e3 * (time.perf_counter() - t0))
		out.append(dict(n=n, d=3, F2=1024, feature_posterior_ms=spread(total), gram_ms=spread(gram), gram_share=float(np.median(gram) / np.median(total)),
						predict_64_points_ms=spread(pred), posterior_mean_solve_ms=spread(solve), mll=mll, finite=finite))  # fmt: skip
		op.close()
	return out


def part_c(parent: Path, ab_out):
	head = ["bench.py --gpus 1 --steps 5 --warmup 2 on the parent commit (its own tree and library) and on this tree, alternating three times in one job",
			"(MI355X; DESIGN.md 4.22). probe-matvecs/s, ms per step, the estimate."]  # fmt: skip
	lines, rows = [], []
	for i in (1, 2, 3):
		for tag, tree in (("parent", parent), ("this", ROOT)):
			r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"], cwd=tree, capture_output=True, text=True, timeout=150)
			if r.returncode != 0:
				raise RuntimeError(f"bench.py in {tree} ended with status {r.returncode}: {r.stderr[-400:]}")
			res = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and '"estimate"' in l][-1]
			rows.append(dict(tree=tag, run=i, value=res["value"], ms_per_step=res["ms_per_step"], estimate=res["estimate"]))
			lines.append(f"{tag + ' ' + str(i):<10} {res['value']:.1f}  {res['ms_per_step']:.3f} ms/step  estimate {res['estimate']!r}")
	if ab_out:
		Path(ab_out).write_text("\n".join(head + lines) + "\n")
	return dict(runs=rows, estimates_identical=len({r["estimate"] for r in rows}) == 1)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--parts", default="ab")
	ap.add_argument("--out", default=None)
	ap.add_argument("--parent", default=None, help="(part c) a checkout of the parent commit with its library built")
	ap.add_argument("--ab-out", default=None, help="(part c) where the six lines go")
	args = ap.parse_args()
	if "c" in args.parts:  # (before this process opens the device: the children own it in turn)
		if not args.parent:
			ap.error("--parts c needs --parent DIR")
		res = dict(c_bench_ab=part_c(Path(args.parent).resolve(), args.ab_out))
		print(json.dumps(res))
		return
	from primate_amd import engine as eng

	res = dict(reps=args.reps, warmup_runs=1, launches_per_run=10)
	if "a" in args.parts:
		res["a_adjoint_product"] = part_a(eng, args.reps)
	if "b" in args.parts:
		res["b_feature_posterior"] = part_b(eng, args.reps)
	line = json.dumps(res)
	print(line)
	if args.out:
		Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
	main()
