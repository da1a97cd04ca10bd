"""The launch sequence and the numbers of one library build, for an A/B of two builds (not a test).

Run once per build under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/sequence_trace.py --root TREE --out DIR/out.npz`
(TREE: the checkout whose primate_amd is imported; default: this one), then
    python scripts/sequence_trace.py --compare DIR_A DIR_B
prints, and returns non-zero unless, the sequence of (kernel name, grid, workgroup size, LDS bytes) in the two traces is identical
line for line and every array of the two .npz files is np.array_equal.

Cases: every sequence enqueue_run can take (ring-fed tiles at four panel widths and four depths, generic passes and generic
Gram, stored u, dense, a host callback, a resumed run, kept-basis and recompute plans, stale ring columns) and every non-default
switch setting the test suite uses. Each creates its operator and plan under its own environment, draws seeded probes, runs, and
records tridiag() and the quadratures of log, exp and step."""

from __future__ import annotations

import argparse
import csv
import os
import sys
from pathlib import Path

import numpy as np

DEG = 14


def laplacian_2d(m, dtype=np.float64):
	import scipy.sparse as sp

	T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
	A = (sp.kron(sp.identity(m), T) + sp.kron(T, sp.identity(m))).tocsr().astype(dtype)
	A.sort_indices()
	return A


def random_spd_graph(n, avg_deg, seed=17, dtype=np.float64):
	"""Symmetric graph Laplacian + I of a G(n, p) graph (tests/test_gpu_parity.py): scattered neighbours, the stored-u sequence."""
	import scipy.sparse as sp

	rng = np.random.default_rng(seed)
	m = int(n * avg_deg / 2)
	i, j = rng.integers(0, n, m), rng.integers(0, n, m)
	keep = i != j
	W = sp.coo_matrix((rng.uniform(0.5, 2.0, keep.sum()), (i[keep], j[keep])), shape=(n, n))
	W = (W + W.T).tocsr()
	W.sum_duplicates()
	A = (sp.diags(np.asarray(W.sum(axis=1)).ravel() + 1.0) - W).tocsr().astype(dtype)
	A.sort_indices()
	return A


def dense_spd(n, dtype=np.float64):
	rng = np.random.default_rng(3)
	M = rng.standard_normal((n, n))
	return np.asfortranarray((M @ M.T / n + np.eye(n)).astype(dtype))


class HostMatvec:
	"""An operator the library only knows through matvec: the host-callback kind."""

	def __init__(self, A):
		self.A, self.shape, self.dtype = A, A.shape, A.dtype

	def matvec(self, x):
		return self.A @ x


class Env:
	def __init__(self, env):
		self.env, self.had = env, {}

	def __enter__(self):
		for k, v in self.env.items():
			self.had[k] = os.environ.get(k)
			os.environ[k] = v

	def __exit__(self, *exc):
		for k, v in self.had.items():
			if v is None:
				del os.environ[k]
			else:
				os.environ[k] = v


def record(out, name, plan, mid):
	a, b, steps = plan.tridiag()
	out[f"{name}/alpha"], out[f"{name}/beta"], out[f"{name}/steps"] = a, b, steps
	out[f"{name}/log"] = plan.quadrature("log")
	out[f"{name}/exp"] = plan.quadrature("exp", t=-0.1)
	out[f"{name}/step"] = plan.quadrature("step", c=mid)
	info = plan.describe()
	out[f"{name}/describe"] = np.array([str(info[k]) for k in ("panel_width", "panels", "ring_slots", "tiles", "sequence", "omega", "dense_kernel")])


def run_cases(eng, out):
	grid, grid32 = laplacian_2d(72), laplacian_2d(72, np.float32)

	def case(name, A, P, orth, env, mid=4.0, basis=None, stages=None, action=False):
		with Env(env):
			op = eng.DeviceOperator(A)
			plan = eng.LanczosPlan(op, P, min(DEG, A.shape[0]), orth, basis=basis) if basis else eng.LanczosPlan(op, P, min(DEG, A.shape[0]), orth)
			plan.generate_probes("rademacher", seed=5)
			if stages:
				for upto in stages:
					plan.run(upto=upto)
			else:
				plan.run()
			record(out, name, plan, mid)
			if action:
				out[f"{name}/action"] = plan.fun_action("exp", t=-0.1)
			plan.close()
			op.close()

	ring, generic = {"SLQ_TILES": "2"}, {"SLQ_TILES": "0"}
	for P in (130, 64, 32, 16):
		for orth in (0, 3, 6, 12):
			case(f"ring f64 P{P} orth{orth}", grid, P, orth, ring)
			if P >= 64:
				case(f"ring f32 P{P} orth{orth}", grid32, P, orth, ring)
	for orth in (0, 3, 14):
		case(f"generic P40 orth{orth}", grid, 40, orth, generic)
	case("stored-u P40 orth3", random_spd_graph(3000, 5.0), 40, 3, {}, mid=6.0)
	for dt, tag in ((np.float64, "f64"), (np.float32, "f32")):
		for P in (24, 64):
			case(f"dense {tag} P{P}", dense_spd(300, dt), P, 3, {}, mid=1.0)
	case("callback", HostMatvec(random_spd_graph(300, 5.0)), 8, 3, {}, mid=6.0)
	case("resumed 0-5-14", grid, 130, 3, ring, stages=(5, DEG))
	case("kept basis", grid, 130, 3, ring, basis="keep", action=True)
	case("recompute", grid, 130, 3, ring, basis="recompute", action=True)
	## the drop-in entry with two stale ring columns (orth 3: the caller's Q holds the previous run's vectors): exact MGS order
	from primate_amd.lanczos import lanczos

	rng = np.random.default_rng(9)
	Q = np.asfortranarray(rng.standard_normal((grid.shape[0], 3)))
	v0 = rng.uniform(-1.0, 1.0, grid.shape[0])
	with Env(ring):
		a, b = lanczos(grid, v0, deg=DEG, orth=3, Q=Q)
	out["stale/alpha"], out["stale/beta"] = a, b
	for setting in ({"SLQ_MERGED": "0", "SLQ_CROSS": "0"}, {"SLQ_FUSED": "0"}, {"SLQ_MGS": "1"}, {"SLQ_RING_GEN": "0"}, {"SLQ_RING_DEEP": "0"},
	                {"SLQ_GRAM": "0"}, {"SLQ_OMEGA": "0"}, {"SLQ_LAST_STORE": "1"}, {"SLQ_GRAPH": "0"}):  # fmt: skip
		tag = " ".join(f"{k}={v}" for k, v in setting.items())
		for orth in (0, 3, 6):
			case(f"{tag} ring P130 orth{orth}", grid, 130, orth, {**ring, **setting})
		case(f"{tag} ring P32 orth3", grid, 32, 3, {**ring, **setting})
		case(f"{tag} generic P40 orth3", grid, 40, 3, {**generic, **setting})


def kernel_lines(d: Path):
	files = sorted(d.rglob("*kernel_trace.csv"))
	assert len(files) == 1, f"{d}: expected one kernel trace, found {files}"
	with open(files[0], newline="") as fh:
		rows = list(csv.DictReader(fh))
	key = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
	rows.sort(key=lambda r: int(r[key]))
	cols = [c for c in rows[0] if c == "Kernel_Name" or c.startswith("Grid_Size") or c.startswith("Workgroup_Size") or c in ("LDS_Block_Size", "Group_Segment_Size")]
	assert "Kernel_Name" in cols and len(cols) >= 8, cols
	return [tuple(r[c] for c in cols) for r in rows]


def compare(da: Path, db: Path) -> int:
	bad = 0
	ka, kb = kernel_lines(da), kernel_lines(db)
	print(f"kernel trace: {len(ka)} launches in {da}, {len(kb)} in {db}")
	for i, (x, y) in enumerate(zip(ka, kb)):
		if x != y:
			print(f"  launch {i} differs:\n    {x}\n    {y}")
			bad += 1
			if bad >= 20:
				break
	bad += len(ka) != len(kb)
	print("kernel trace: " + ("IDENTICAL line for line (kernel name, grid, workgroup size, LDS bytes)" if not bad else f"{bad} DIFFERENCES"))
	za, zb = np.load(da / "out.npz"), np.load(db / "out.npz")
	names = sorted(set(za.files) | set(zb.files))
	unequal = [n for n in names if n not in za.files or n not in zb.files or not np.array_equal(za[n], zb[n], equal_nan=za[n].dtype.kind == "f")]
	print(f"arrays: {len(names)} in {len({n.split('/')[0] for n in names})} cases; " + ("every one np.array_equal" if not unequal else f"UNEQUAL: {unequal}"))
	return int(bool(bad or unequal))


def main() -> int:
	ap = argparse.ArgumentParser()
	ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
	ap.add_argument("--out")
	ap.add_argument("--compare", nargs=2)
	args = ap.parse_args()
	if args.compare:
		return compare(Path(args.compare[0]), Path(args.compare[1]))
	sys.path.insert(0, str(Path(args.root).resolve()))
	from primate_amd import engine as eng

	out = {}
	run_cases(eng, out)
	np.savez(args.out, **out)
	print(f"{len(out)} arrays written to {args.out} (library of {Path(eng.__file__).resolve().parent})")
	return 0


if __name__ == "__main__":
	sys.exit(main())
