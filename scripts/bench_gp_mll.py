"""One gp.mll call split into its phases -> profiles/gp_mll_bench.json: n = 16384 and 262144 points in [0, 1]^3, rbf,
lengthscale 0.3, rank 128, sigma2 = 1e-4, deg 20, 64 device-drawn probes in batches of 16, one column of y. A training step is what is
timed: the preconditioned operator is kept, the hyperparameters move by 1 % before every call, so `refresh` is a whole factorisation.
Wall time per phase in ms, each phase closed by a stream synchronisation (gp.mll(profile=True)): median [min, max] of 5 calls after
one warm-up. `lanczos` is the 4 batches' runs, quadratures and inverse actions, `updates` the 4 sampled gradient updates with their
read-back, `exact` the deterministic part tr(P^-1 dA/dtheta) - ceil(rank / 64) pairs of column launches and gradient updates. `auto`
leaves the exact part out where the factor is poor (the largest Ritz value of B above 2), so it is ALSO timed on its own after the
calls (`exact_alone_ms`: DeviceOperator.precond_trace_grad and the read-back of d + 2 doubles, median [min, max] of 5 after a warm-up).
  python scripts/bench_gp_mll.py [--sizes 16384,262144] [--out profiles/gp_mll_bench.json]"""
import argparse, json, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from primate_amd import gp
from primate_amd.operators import KernelOperator

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="16384,262144")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=str(ROOT / "profiles" / "gp_mll_bench.json"))
args = ap.parse_args()
out = dict(config=dict(kernel="rbf", d=3, lengthscale=0.3, rank=128, noise=1e-4, deg=20, count=64, batch=16, reps=args.reps), sizes={})
for n in (int(v) for v in args.sizes.split(",")):
	rng = np.random.default_rng(n)
	X = rng.random((n, 3))
	y = np.sin(4.0 * X[:, 0]) * np.cos(3.0 * X[:, 1]) + 0.01 * rng.standard_normal(n)
	K = KernelOperator(X, "rbf", lengthscale=0.3, outputscale=1.0, noise=1e-4)
	B = K.preconditioned(128)
	rows, totals, last = [], [], None
	for rep in range(args.reps + 1):
		K.set_parameters(lengthscale=0.3 * (1.0 + 0.01 * rep))  # (the factor is stale: the call refreshes it)
		t = time.perf_counter()
		value, grads, info = gp.mll(B, y, deg=20, count=64, batch=16, seed=1, profile=True)
		total = 1e3 * (time.perf_counter() - t)
		if rep:  # (the first call is the warm-up: it also creates the device operators)
			rows.append(info["timing_ms"])
			totals.append(total)
		last = (value, grads, info)
		print(f"n {n} call {rep}: {total:.1f} ms  " + "  ".join(f"{k} {v:.1f}" for k, v in info["timing_ms"].items()), flush=True)
	stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))  # noqa: E731
	li = last[2]["logdet_info"]
	out["sizes"][str(n)] = dict(phases_ms={k: stat([r[k] for r in rows]) for k in rows[0]}, total_ms=stat(totals),
								control_variate=li["control_variate"], ritz_max=li["ritz_max"], rank=li["rank"], steps=last[2]["steps"], value=last[0],
								grads={k: np.ravel(v).tolist() for k, v in last[1].items()},
								grad_std_error={k: np.ravel(v).tolist() for k, v in last[2]["grad_std_error"].items()})  # fmt: skip
	from primate_amd import engine
	from primate_amd.lanczos import _as_device_operator
	pop = _as_device_operator(B, dtype=np.float64)
	acc = engine.KernelGradAccumulator(pop.base)
	alone = []
	for rep in range(args.reps + 1):
		pop.ctx.synchronize()
		t = time.perf_counter()
		pop.precond_trace_grad(acc, 1.0, 0.0)
		vals = acc.get()[0]
		alone.append(1e3 * (time.perf_counter() - t))
	acc.close()
	out["sizes"][str(n)]["exact_alone_ms"] = stat(alone[1:])
	out["sizes"][str(n)]["exact_values"] = vals.tolist()
	print(f"n {n} exact part alone: " + "  ".join(f"{v:.2f}" for v in alone) + " ms", flush=True)
	for obj in (B, K):
		_as_device_operator(obj, dtype=np.float64).close()
Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
print(f"wrote {args.out}")
