"""bench_kernelop.py - what the matrix-free kernel operator costs (slq_kernel_*), three measurements:

 (a) one product against the dense operator: n = 16384, d = 3 and 16, P = 128 (fp64) and 256 (fp32), rbf. The time of one product
     is the plan's own profile (class spmm_3term: the product kernel and, where j is split, the slab sum) over `reps` Lanczos runs
     of 10 steps after a warm-up run, next to the library's dense operator on a materialised matrix of the same size under the
     same plan. Flops: 2 n^2 (d_pad + P) on the matrix cores; quoted against 78.6 (fp64) / 157.3 (fp32) TFLOP/s.
     --phi1 LIB: the same kernel-operator rows again from a build with -DSLQ_KERNEL_PHI_ONE (phi == 1: scripts/ab_build.py), in a
     process of its own: what share of the time the profile costs.
 (b) the size no dense operator reaches: n = 262144, d = 3, fp64, 64 device-drawn probes, deg = 30, orth 3: seconds per batch of
     MatrixFunction.quad_generated (wall time, ended by its synchronising read), and the operator's bytes on the device.
 (c) columns per K-tile evaluation: n = 16384, d = 3, fp64, P = 16 .. 256 (1 .. 16 accumulator tiles per wave): ms per product and
     per column.

    python scripts/bench_kernelop.py [--reps 5] [--parts abc] [--phi1 build/kernelop_phi1/_libslq.so] [--out profiles/kernelop_bench.json]
Prints one JSON line; --out writes it to a file."""

from __future__ import annotations

import argparse
import json
import os
import subprocess
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


def product_ms(eng, op, P, reps, steps=10):
	"""ms per product from the plan's profile: `reps` runs of `steps` steps after one warm-up run."""
	plan = eng.LanczosPlan(op, P, steps, 0)
	try:
		plan.profile_enable(True)
		out = []
		for r in range(reps + 1):
			plan.generate_probes("rademacher", seed=r)
			plan.run()
			pr = plan.profile_read()["spmm_3term"]
			if r:
				out.append(pr["ms"] / max(pr["launches"], 1))
		d = plan.describe()
		return dict(spread(out), launches_per_run=int(pr["launches"]), panels=d["panels"], panel_width=d["panel_width"], slabs=d["dense_ksplit"])
	finally:
		plan.close()


def points(n, d, dtype):
	return np.random.default_rng(n + d).random((n, d)).astype(dtype)


def part_a(eng, reps, kernel_only):
	from primate_amd.operators import KernelOperator

	n, rows = 16384, []
	for dtype, P in ((np.float64, 128), (np.float32, 256)):
		name = np.dtype(dtype).name
		dense_ms = None
		if not kernel_only:
			K3 = KernelOperator(points(n, 3, dtype), "rbf", lengthscale=0.3, noise=0.1, dtype=dtype)
			A = np.empty((n, n), dtype=dtype, order="F")
			for i0 in range(0, n, 2048):
				A[i0 : i0 + 2048] = K3.rows(np.arange(i0, min(n, i0 + 2048)))
			A = np.asfortranarray(np.minimum(A, A.T))  # (exactly symmetric, whatever the blocked evaluation rounded)
			op = eng.DeviceOperator(A)
			dense_ms = product_ms(eng, op, P, reps)
			op.close()
			del A
		for d in (3, 16):
			K = KernelOperator(points(n, d, dtype), "rbf", lengthscale=0.3 * np.sqrt(d / 3.0), noise=0.1, dtype=dtype)
			op = eng.DeviceOperator(K)
			ms = product_ms(eng, op, P, reps)
			op.close()
			dpad = (d + 3) // 4 * 4
			flops = 2.0 * n * n * (dpad + P)
			row = dict(dtype=name, n=n, d=d, P=P, kernel_ms=ms, mfma_flops=flops, tflops=flops / (ms["median"] * 1e-3) / 1e12,
					   frac_of_matrix_peak=flops / (ms["median"] * 1e-3) / PEAK[name])  # fmt: skip
			if dense_ms is not None:
				row["dense_ms"] = dense_ms
				row["dense_over_kernel"] = dense_ms["median"] / ms["median"]
			rows.append(row)
	return rows


def part_b(eng):
	from primate_amd.operators import KernelOperator, MatrixFunction

	n, d, P, deg = 262144, 3, 64, 30
	K = KernelOperator(points(n, d, np.float64), "rbf", lengthscale=0.05, noise=0.1)
	ctx = eng.default_context()
	ctx.synchronize()
	free0, _ = ctx.meminfo()
	M = MatrixFunction(K, fun="log", deg=deg, orth=3)
	free1, _ = ctx.meminfo()
	secs = []
	for r in range(3):
		t0 = time.perf_counter()
		q = M.quad_generated(P, "rademacher", seed=r)
		secs.append(time.perf_counter() - t0)
	return dict(n=n, d=d, P=P, deg=deg, orth=3, operator_bytes=int(free0 - free1), dense_bytes=8 * n * n, first_batch_s=secs[0], batch_s=spread(secs[1:]),
				logdet_estimate=float(np.mean(q)), products_per_batch=deg, mfma_flops_per_batch=2.0 * n * n * (4 + P) * deg)  # fmt: skip


def part_c(eng, reps):
	from primate_amd.operators import KernelOperator

	n, d = 16384, 3
	K = KernelOperator(points(n, d, np.float64), "rbf", lengthscale=0.3, noise=0.1)
	op = eng.DeviceOperator(K)
	rows = []
	for P in (16, 32, 64, 128, 256):
		ms = product_ms(eng, op, P, reps)
		rows.append(dict(P=P, column_tiles_per_wave=min(16, P // 16), ms=ms, us_per_column=1e3 * ms["median"] / P))
	op.close()
	return rows


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--parts", default="abc")
	ap.add_argument("--phi1", default=None, help="a libslq built with -DSLQ_KERNEL_PHI_ONE: part (a)'s kernel rows again, in a child process")
	ap.add_argument("--kernel-only", type=int, default=0, help="part (a) without the dense operator (what the --phi1 child runs)")
	ap.add_argument("--out", default=None)
	a = ap.parse_args()
	from primate_amd import engine as eng

	res = dict(reps=a.reps, warmup_runs=1, steps_per_run=10, library=os.environ.get("PRIMATE_AMD_LIBSLQ", "primate_amd/_libslq.so"))
	if "a" in a.parts:
		res["a_product_vs_dense"] = part_a(eng, a.reps, bool(a.kernel_only))
	if "c" in a.parts:
		res["c_columns_per_tile_evaluation"] = part_c(eng, a.reps)
	if "b" in a.parts:
		res["b_large"] = part_b(eng)
	if a.phi1 and "a" in a.parts:
		env = dict(os.environ, PRIMATE_AMD_LIBSLQ=str(Path(a.phi1).resolve()))
		child = subprocess.run([sys.executable, __file__, "--parts", "a", "--kernel-only", "1", "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=600)
		if child.returncode != 0:
			raise RuntimeError(f"the phi == 1 run failed:\n{child.stderr}")
		phi1 = json.loads(child.stdout.strip().splitlines()[-1])["a_product_vs_dense"]
		for row, one in zip(res["a_product_vs_dense"], phi1):
			row["phi1_ms"] = one["kernel_ms"]
			row["profile_share_of_time"] = 1.0 - one["kernel_ms"]["median"] / row["kernel_ms"]["median"]
	line = json.dumps(res)
	print(line)
	if a.out:
		Path(a.out).parent.mkdir(parents=True, exist_ok=True)
		Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
	main()
