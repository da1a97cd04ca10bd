"""bench_kernelcross.py - what the cross-covariance products of the kernel operator cost (slq_kernel_cross_*).

rbf, d = 3 and 16, n = 16384 training points, m = 128, 1024 and 16384 new points, b = 1, 64 and 128 columns, forward (Y = C W) and
adjoint (Y = C^T U), in fp64 and fp32. Each figure is 5 windows of 10 calls after a warm-up window, wall time of a window ended by a
stream synchronisation, reported as median [min, max] ms per call:

  fp64  through slq_kernel_cross_dmat: operands and results stay on the device - the kernel, and the slab sum where there is one;
  fp32  has no device-matrix entry: slq_kernel_cross_matmat, whose time INCLUDES the two panels' transfers; the fp64 rows carry the
        same entry's time too (`host_ms`), so that the share of the transfers can be read off.

Beside each shape stands the operator's own square product of the same flop count - n' = sqrt(m n) points (1448, 4096, 16384), b
probes, the unchanged k_kernel_panel under a plan, from the plan's profile (class spmm_3term over the products of a 10-step run) -
and the ratio of the two flop rates (2 rows points (d_pad + b) each; a plan pads b = 1 to a panel of 16 columns, the cross product
to one 16-column tile: both spend the same matrix-core work on it).

For m = 128 the forward rows also record the schedule's slab count and `one_slab_round_ms`: the forward product of 32768 = 256 x 128
new points against the same n and b, which the schedule leaves at one slab - every workgroup walks all n / 16 tiles, one workgroup
per compute unit - i.e. what the m = 128 product would cost without the cut.

    python scripts/bench_kernelcross.py [--out profiles/kernelcross_bench.json]
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

WINDOWS, CALLS = 5, 10
N = 16384


def spread(v):
	v = sorted(v)
	return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def windows(ctx, call):
	"""ms per call: WINDOWS windows of CALLS calls after a warm-up window."""
	out = []
	for w in range(WINDOWS + 1):
		ctx.synchronize()
		t0 = time.perf_counter()
		for _ in range(CALLS):
			call()
		ctx.synchronize()
		if w:
			out.append(1e3 * (time.perf_counter() - t0) / CALLS)
	return spread(out)


def points(n, d, dtype, seed=0):
	return np.random.default_rng(n + d + seed).random((n, d)).astype(dtype)


def square_ms(eng, op, P):
	"""ms per product of the operator's own k_kernel_panel under a plan of P probes: the plan's profile over 10-step runs."""
	plan = eng.LanczosPlan(op, P, CALLS, 0)
	try:
		plan.profile_enable(True)
		out = []
		for r in range(WINDOWS + 1):
			plan.generate_probes("rademacher", seed=r)
			plan.run()
			pr = plan.profile_read()["spmm_3term"]
			if r:
				out.append(pr["ms"] / CALLS)
		return spread(out)
	finally:
		plan.close()


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--out", default=None)
	ap.add_argument("--quick", type=int, default=0, help="1: d = 3, m = 128 only (a check that the script runs)")
	a = ap.parse_args()
	from primate_amd import engine as eng
	from primate_amd.operators import KernelOperator

	ctx = eng.default_context()
	rows = []
	for dtype in (np.float64, np.float32):
		name = np.dtype(dtype).name
		for d in (3,) if a.quick else (3, 16):
			dpad = (d + 3) // 4 * 4
			ls = 0.3 * np.sqrt(d / 3.0)
			K = KernelOperator(points(N, d, dtype), "rbf", lengthscale=ls, noise=0.1, dtype=dtype)
			op = eng.DeviceOperator(K, ctx=ctx)
			for m in (128,) if a.quick else (128, 1024, 16384):
				nsq = int(round(np.sqrt(m * N)))
				Ksq = KernelOperator(points(nsq, d, dtype, seed=1), "rbf", lengthscale=ls, noise=0.1, dtype=dtype)
				opsq = eng.DeviceOperator(Ksq, ctx=ctx)
				cross = eng.KernelCross(op, points(m, d, dtype, seed=2))
				big = eng.KernelCross(op, points(256 * 128, d, dtype, seed=3)) if m == 128 else None
				for b in (1, 64, 128):
					flops = 2.0 * m * N * (dpad + b)
					sq = square_ms(eng, opsq, b)
					sq_flops = 2.0 * nsq * nsq * (dpad + b)
					Wn = np.asfortranarray(np.random.default_rng(b).standard_normal((N, b)).astype(dtype))
					Um = np.asfortranarray(np.random.default_rng(b + 1).standard_normal((m, b)).astype(dtype))
					for trans in (False, True):
						X = Um if trans else Wn
						host = windows(ctx, lambda: cross.matmat(X, trans=trans))
						row = dict(dtype=name, d=d, m=m, n=N, b=b, direction="adjoint" if trans else "forward", mfma_flops=flops, host_ms=host)
						if dtype == np.float64:
							Nm, Mm = eng.DeviceMatrix(N, b, ctx=ctx), eng.DeviceMatrix(m, b, ctx=ctx)
							(Mm if trans else Nm).set(0, X)
							IN, OUT = (Mm, Nm) if trans else (Nm, Mm)
							row["ms"] = windows(ctx, lambda: cross.matmat_dmat(IN, 0, OUT, 0, b, trans=trans))
							row["entry"] = "dmat"
							Nm.close(), Mm.close()
						else:
							row["ms"], row["entry"] = host, "matmat (includes the transfers)"
						S = eng.kernel_cross_schedule(N if trans else m, m if trans else N, b, 256)
						row["slabs"], row["row_blocks"], row["col_blocks"] = S["slabs"], S["nrb"], S["col_blocks"]
						row["tflops"] = flops / (row["ms"]["median"] * 1e-3) / 1e12
						row["square"] = dict(n=nsq, P=b, ms=sq, mfma_flops=sq_flops, tflops=sq_flops / (sq["median"] * 1e-3) / 1e12)
						row["rate_over_square"] = row["tflops"] / row["square"]["tflops"]
						if big is not None and not trans and dtype == np.float64:
							Nm, Bm = eng.DeviceMatrix(N, b, ctx=ctx), eng.DeviceMatrix(256 * 128, b, ctx=ctx)
							Nm.set(0, Wn)
							Sb = eng.kernel_cross_schedule(256 * 128, N, b, 256)
							row["one_slab_round_ms"] = windows(ctx, lambda: big.matmat_dmat(Nm, 0, Bm, 0, b))
							row["one_slab_round_slabs"] = Sb["slabs"]
							Nm.close(), Bm.close()
						rows.append(row)
						print(json.dumps(row), file=sys.stderr, flush=True)
				for o in (cross, big, opsq):
					if o is not None:
						o.close()
			op.close()
	res = dict(windows=WINDOWS, calls_per_window=CALLS, warmup_windows=1, n=N, profile="rbf", rows=rows)
	line = json.dumps(res)
	print(line)
	if a.out:
		Path(a.out).parent.mkdir(parents=True, exist_ok=True)
		Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
	main()
