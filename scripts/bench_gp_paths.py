"""bench_gp_paths.py - what the random-feature product and `gp.sample_paths` cost (slq_kernel_feature_*):

 (a) one feature product Y = Phi W at the operator's points: n = 16384, d = 3, F2 = 1024 and 4096; fp64 with b = 64 between device
     matrices (slq_kernel_feature_dmat: 10 launches closed by one synchronisation, the wall time over 10), and fp32 with b = 256
     through the host entry (slq_kernel_feature_matmat: the only fp32 entry; its time INCLUDES the upload of W and the download of Y,
     which is said in the row). 5 runs after a warm-up, median [min, max], as bench_kernelop.py reports. Each time stands beside the
     flop model 2 n F2 (d_pad + 2 b) and beside one kernel-operator product at the same n, d and dtype from profiles/kernelop_bench.json
     (P = 128 in fp64, 256 in fp32, scaled to b columns by the operator's own flop model 2 n^2 (d_pad + P)).
 (b) `gp.sample_paths` end to end, count = 64, F2 = 2048, deg = 60, rbf, at n = 16384 and n = 65536: the wall time of the call, of the
     feature product inside it (timed on its own, same shapes), and of `evaluate` at m = 1024 new points; the rest of the call is the
     residual, the draws and the solve.

    python scripts/bench_gp_paths.py [--reps 5] [--out profiles/gp_paths_bench.json]
Prints one JSON line; --out writes it to a file."""

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

PEAK = {"float64": 78.6e12, "float32": 157.3e12}


def spread(v):
	v = sorted(v)
	return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def points(n, d, dtype):
	return np.random.default_rng(n + d).random((n, d)).astype(dtype)


def operator_product_ms(n, d, dtype):
	"""(ms, P) of one kernel-operator product from profiles/kernelop_bench.json at the same n, d and dtype; None where it has no such row."""
	try:
		rows = json.loads((ROOT / "profiles" / "kernelop_bench.json").read_text())["a_product_vs_dense"]
	except (OSError, KeyError, ValueError):
		return None
	for r in rows:
		if r["dtype"] == dtype and r["n"] == n and r["d"] == d:
			return r["kernel_ms"]["median"], r["P"]
	return None


def part_a(eng, reps):
	from primate_amd.operators import KernelOperator

	n, d, dpad = 16384, 3, 4
	out = []
	for dtype, b in ((np.float64, 64), (np.float32, 256)):
		name = np.dtype(dtype).name
		K = KernelOperator(points(n, d, dtype), "rbf", lengthscale=0.3, outputscale=1.5, noise=0.1, dtype=dtype)
		op = eng.DeviceOperator(K)
		for f2 in (1024, 4096):
			fmap = K.features(f2, seed=1).device(op)
			W = np.asfortranarray(np.random.default_rng(f2).standard_normal((2 * f2, b)).astype(dtype))
			ms = []
			if dtype == np.float64:
				Wd, Yd = eng.DeviceMatrix(2 * f2, b, ctx=op.ctx), eng.DeviceMatrix(n, b, ctx=op.ctx)
				Wd.set(0, W)
				for r in range(reps + 1):
					op.ctx.synchronize()
					t0 = time.perf_counter()
					for _ in range(10):
						fmap.matmat_dmat(Wd, 0, Yd, 0, b)
					op.ctx.synchronize()
					if r:
						ms.append(1e3 * (time.perf_counter() - t0) / 10)
				Wd.close(), Yd.close()
				entry = "dmat (device to device)"
			else:
				for r in range(reps + 1):
					t0 = time.perf_counter()
					fmap.matmat(W)
					if r:
						ms.append(1e3 * (time.perf_counter() - t0))
				entry = "matmat (host panels: upload of W and download of Y included)"
			flops = 2.0 * n * f2 * (dpad + 2 * b)
			S = eng.kernel_feature_schedule(n, f2, b, 256, dtype)
			row = dict(dtype=name, n=n, d=d, F2=f2, b=b, entry=entry, ms=spread(ms), mfma_flops=flops, tflops=flops / (np.median(ms) * 1e-3) / 1e12,
					   frac_of_matrix_peak=flops / (np.median(ms) * 1e-3) / PEAK[name], slabs=S["slabs"], col_blocks=S["col_blocks"], chunks=S["chunks"])  # fmt: skip
			ref = operator_product_ms(n, d, name)
			if ref is not None:
				ms_op, P = ref
				scaled = ms_op * (dpad + b) / (dpad + P)
				row.update(operator_product_ms=ms_op, operator_product_P=P, operator_product_ms_at_b=scaled, feature_over_operator=float(np.median(ms)) / scaled,
						   flop_model_ratio=flops / (2.0 * n * n * (dpad + b)))  # fmt: skip
			out.append(row)
			fmap.close()
		op.close()
	return out


def part_b(eng):
	from primate_amd import gp
	from primate_amd.operators import KernelOperator

	out = []
	for n in (16384, 65536):
		X = points(n, 3, np.float64)
		y = np.sin(6 * X[:, 0]) * np.cos(4 * X[:, 1]) + 0.3 * np.random.default_rng(1).standard_normal(n)
		K = KernelOperator(X, "rbf", lengthscale=0.3, outputscale=1.5, noise=0.1)
		op = eng.DeviceOperator(K)
		Xnew = points(1024, 3, np.float64)[::-1].copy()
		row = dict(n=n, d=3, count=64, F2=2048, deg=60, m=1024)
		for r in range(2):  # (a warm-up call, then the timed one)
			op.ctx.synchronize()
			t0 = time.perf_counter()
			paths = gp.sample_paths(K, y, count=64, num_features=2048, deg=60, seed=3)
			op.ctx.synchronize()
			total = 1e3 * (time.perf_counter() - t0)
			t0 = time.perf_counter()
			F = paths.evaluate(Xnew)
			ev = 1e3 * (time.perf_counter() - t0)
			t0 = time.perf_counter()
			F, dF = paths.evaluate(Xnew[:64], grad=True)
			evg = 1e3 * (time.perf_counter() - t0)
			steps = paths.info["steps"]
			fmap = paths.features.device(op)
			Wd, Yd = eng.DeviceMatrix(4096, 64, ctx=op.ctx), eng.DeviceMatrix(n, 64, ctx=op.ctx)
			fmap.matmat_dmat(Wd, 0, Yd, 0, 64)
			op.ctx.synchronize()
			t0 = time.perf_counter()
			fmap.matmat_dmat(Wd, 0, Yd, 0, 64)
			op.ctx.synchronize()
			feat = 1e3 * (time.perf_counter() - t0)
			for o in (Wd, Yd, fmap, paths):
				o.close()
		row.update(sample_paths_ms=total, features_ms=feat, rest_ms=total - feat, evaluate_ms=ev, evaluate_grad_64_points_ms=evg, steps=[int(np.max(s)) for s in steps],
				   finite=bool(np.all(np.isfinite(F)) and np.all(np.isfinite(dF))))  # fmt: skip
		out.append(row)
		op.close()
	return out


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--parts", default="ab")
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	from primate_amd import engine as eng

	res = dict(reps=args.reps, warmup_runs=1, launches_per_run=10)
	if "a" in args.parts:
		res["a_feature_product"] = part_a(eng, args.reps)
	if "b" in args.parts:
		res["b_sample_paths"] = part_b(eng)
	line = json.dumps(res)
	print(line)
	if args.out:
		Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
	main()
