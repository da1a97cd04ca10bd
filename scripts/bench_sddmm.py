"""bench_sddmm.py - what the sampled dense-dense product (slq_sddmm_update) moves, and what the gradient adds to a trace
estimate (primate_amd.grad.trace_grad against trace.hutch).

    python scripts/bench_sddmm.py [--ops lap2d,lap3d,graph] [--m 64,256] [--window 0.5] [--reps 5] [--grad 1] [--profile-only 0] [--out FILE]

Kernel rate: on the 2-D Laplacian n = 10^6, the 3-D 100^3 Laplacian and an Erdos-Renyi graph Laplacian (n = 5e5, average degree
16: configs[2]'s kind), m columns of two random device matrices, symmetric off and on. After a warm-up, `reps` windows of at
least `window` seconds of back-to-back updates, each ended by a device synchronise; ms per update = window / updates. Bytes per
update are the model of DESIGN §4.14 - 2 n m 8 (4 n m 8 when symmetric) + nnz (4 + 8 (1 + [beta != 0])) + 4 (n + 1) - and the
rate is quoted against slq_measure_stream(mode 0) taken in this process and against 8 TB/s.
What the gradient adds: MatrixFunction(log, deg = 30) on the 2-D Laplacian, 256 device-drawn Rademacher probes in one batch:
hutch(M) and trace_grad(M), alternating, `reps` times each, wall time ended by the calls' own synchronising reads.
--profile-only 1: a few updates per shape and nothing else - the run to put under `rocprofv3 --kernel-trace --stats`.
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


def lap1d(m):
	import scipy.sparse as sp

	return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))


def make_pattern(kind: str):
	import scipy.sparse as sp

	if kind == "lap2d":
		T, I = lap1d(1000), sp.identity(1000)
		A = sp.kron(I, T) + sp.kron(T, I)
	elif kind == "lap3d":
		T, I = lap1d(100), sp.identity(100)
		A = sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)
	elif kind == "graph":
		n, deg = 500_000, 16.0
		rng = np.random.default_rng(4)
		k = int(n * deg / 2)
		i, j = rng.integers(0, n, k), rng.integers(0, n, k)
		keep = i != j
		W = sp.coo_matrix((np.ones(int(keep.sum())), (i[keep], j[keep])), shape=(n, n))
		W = (W + W.T).tocsr()
		W.sum_duplicates()
		A = sp.diags(np.asarray(W.sum(axis=1)).ravel() + 1.0) - W
	else:
		raise ValueError(f"unknown operator '{kind}'")
	A = A.tocsr().astype(np.float64)
	A.sort_indices()
	return A


def model_bytes(n: int, nnz: int, m: int, symmetric: bool, beta: float) -> int:
	return (4 if symmetric else 2) * n * m * 8 + nnz * (4 + 8 * (1 + (1 if beta != 0.0 else 0))) + 4 * (n + 1)


def time_updates(ctx, acc, W, Z, m, symmetric, window, reps):
	def burst(k):
		t0 = time.perf_counter()
		for _ in range(k):
			acc.update(W, 0, Z, 0, m, alpha=1e-3, beta=1.0, symmetric=symmetric)
		ctx.synchronize()
		return time.perf_counter() - t0

	burst(3)  # warm-up: code object, caches
	one = burst(4) / 4
	k = max(4, int(np.ceil(1.2 * window / max(one, 1e-6))))
	ms = []
	for _ in range(reps):
		acc.reset()
		ctx.synchronize()
		dt = burst(k)
		ms.append(dt / k * 1e3)
	return k, ms


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--ops", default="lap2d,lap3d,graph")
	ap.add_argument("--m", default="64,256")
	ap.add_argument("--window", type=float, default=0.5)
	ap.add_argument("--reps", type=int, default=5)
	ap.add_argument("--grad", type=int, default=1)
	ap.add_argument("--profile-only", type=int, default=0)
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	from primate_amd import _capi, engine

	ctx = engine.default_context()
	ms_list = [int(v) for v in args.m.split(",")]
	rec = {"bench": "sddmm", "lib": Path(_capi.LIB_PATH).name, "window_s": args.window, "reps": args.reps, "kernel": [], "gradient": "not measured"}
	if not args.profile_only:
		rec["stream_read_GBps"] = [ctx.measure_stream("read") for _ in range(3)]
	stream = float(np.median(rec.get("stream_read_GBps", [np.nan])))
	for kind in [k for k in args.ops.split(",") if k]:
		A = make_pattern(kind)
		n, nnz = A.shape[0], A.nnz
		sched = engine.sddmm_schedule(A.indptr)
		acc = engine.SddmmAccumulator(A, ctx=ctx)
		cols = max(ms_list)
		W, Z = engine.DeviceMatrix(n, cols, ctx=ctx), engine.DeviceMatrix(n, cols, ctx=ctx)
		W.generate(0, cols, "normal", seed=1)
		Z.generate(0, cols, "rademacher", seed=2)
		for m in ms_list:
			for symmetric in (False, True):
				if args.profile_only:
					for _ in range(5):
						acc.update(W, 0, Z, 0, m, alpha=1e-3, beta=1.0, symmetric=symmetric)
					ctx.synchronize()
					continue
				k, ms = time_updates(ctx, acc, W, Z, m, symmetric, args.window, args.reps)
				nbytes = model_bytes(n, nnz, m, symmetric, 1.0)
				med = float(np.median(ms))
				rec["kernel"].append({
					"op": kind, "n": n, "nnz": nnz, "m": m, "symmetric": symmetric, "items": int(sched["row0"].size), "long_rows": sched["nlong"],
					"updates_per_window": k, "ms_per_update": {"min": min(ms), "median": med, "max": max(ms), "all": ms}, "model_bytes": nbytes,
					"model_TBps": nbytes / (med * 1e-3) / 1e12, "share_of_stream_read": nbytes / (med * 1e-3) / 1e9 / stream,
					"share_of_8TBps": nbytes / (med * 1e-3) / 8e12,
				})  # fmt: skip
		for d in (acc, W, Z):
			d.close()
	if args.grad and not args.profile_only:
		from primate_amd.grad import trace_grad
		from primate_amd.operators import MatrixFunction
		from primate_amd.trace import hutch

		A = make_pattern("lap2d")
		M = MatrixFunction(A, "log", deg=30)
		kw = dict(pdf="device:rademacher", seed=7)

		def run_hutch():
			t0 = time.perf_counter()
			est = hutch(M, batch=256, converge="count", count=256, **kw)
			return (time.perf_counter() - t0) * 1e3, float(est)

		def run_grad():
			t0 = time.perf_counter()
			est, grad, info = trace_grad(M, count=256, batch=256, **kw)
			return (time.perf_counter() - t0) * 1e3, float(est)

		run_hutch(), run_grad()  # warm-up: both plans exist afterwards
		th, tg, eh, eg = [], [], None, None
		for _ in range(args.reps):
			a, eh = run_hutch()
			b, eg = run_grad()
			th.append(a)
			tg.append(b)
		rec["gradient"] = {
			"op": "lap2d", "n": A.shape[0], "fun": "log", "deg": 30, "probes": 256, "batch": 256, "basis_used": M.basis_used,
			"hutch_ms": {"min": min(th), "median": float(np.median(th)), "max": max(th), "all": th}, "hutch_estimate": eh,
			"trace_grad_ms": {"min": min(tg), "median": float(np.median(tg)), "max": max(tg), "all": tg}, "trace_grad_estimate": eg,
			"ratio_median": float(np.median(tg) / np.median(th)),
			"note": "trace_grad's time includes the f'(A) V combination over the kept basis, the probe copy, the SDDMM update and the nnz-sized copy of the gradient to the host",
		}  # fmt: skip
	line = json.dumps(rec)
	print(line)
	if args.out:
		Path(args.out).parent.mkdir(parents=True, exist_ok=True)
		Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
	main()
