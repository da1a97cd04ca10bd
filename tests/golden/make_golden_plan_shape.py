"""Records tests/golden/plan_shape_golden.npz (tests/test_plan_shape_cpu.py, tests/test_gpu_plan_shape.py). Three steps, each
writing a part file, then a merge:

  python tests/golden/make_golden_plan_shape.py live OUT.npz --lib PARENT_LIB   (GPU; the library of the commit BEFORE plan_shape existed)
  python tests/golden/make_golden_plan_shape.py facts OUT.npz                   (GPU; this tree's library)
  python tests/golden/make_golden_plan_shape.py grid OUT.npz                    (no GPU; this tree's library)
  python tests/golden/make_golden_plan_shape.py merge LIVE.npz FACTS.npz GRID.npz

`live`: the plans of _plan_cases.GPU_CASES created with the parent's library, which is that commit plus one uncommitted entry
`slq_debug_plan_shape_of` that reads the FIELDS of a live plan into the order of plan_shape_to_array (NaN where that commit kept no
field: the region sizes, t_slabs_bound, two offsets). Per case: those values, describe(), basis mode, workspace bytes, the dense
path, and the arrays of one 12-step run. This is what ties plan_shape() to what creation computed before it was a function.
`facts`: the same plans with this tree's library: their facts (the parent had no such record), matched by label.
`grid`: slq_debug_plan_shape over the CPU grid, from this tree: that part guards later changes, it does not prove the first one."""

import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
GOLDEN = ROOT / "tests" / "golden" / "plan_shape_golden.npz"


def live(out: str, lib, with_runs: bool):
	from primate_amd import _capi

	if lib:
		_capi.LIB_PATH = Path(lib).resolve()
		_capi._SIGNATURES.pop("slq_debug_plan_shape")  # (the parent's library has only the recorder)
	import _plan_cases as pc
	from primate_amd.engine import Context, DeviceOperator

	ctx = Context(device=0)
	rec, ops = {}, {}
	for label, (opname, tiles, dtype, kind, nprobes) in pc.GPU_CASES.items():
		with pc.tiles_env(tiles):
			key = (opname, tiles, dtype)
			if key not in ops:
				ops[key] = DeviceOperator(pc.gpu_matrix(opname), dtype=np.float64 if dtype == "f64" else np.float32, ctx=ctx)
			op = ops[key]
			plan = pc.gpu_plan(op, kind, nprobes)
		fa, sa = pc.shape_of_plan(plan)
		if with_runs:
			rec[f"{label}/shape"] = sa
			rec[f"{label}/describe"] = pc.describe_array(plan)
			rec[f"{label}/basis_mode"] = np.array(plan.basis_mode)
			rec[f"{label}/workspace_bytes"] = np.array(plan.workspace_bytes, dtype=np.int64)
			for k, v in pc.gpu_run(plan, kind, pc.gpu_probes(op.shape[0], nprobes)).items():
				rec[f"{label}/run_{k}"] = v
		else:
			rec[f"{label}/facts"] = fa
		plan.close()
		print(label, "ok", flush=True)
	np.savez_compressed(out, **rec)


def grid(out: str):
	import _plan_cases as pc

	call = pc.shape_call()
	labels, shapes = [], []
	for label, sw, f in pc.cpu_grid():
		with pc.switches(sw):
			s = call(pc.facts_array(f))
		assert np.all(s == np.round(s))
		labels.append(label), shapes.append(s.astype(np.int64))
	np.savez_compressed(out, grid_labels=np.array(labels), grid_shapes=np.array(shapes))
	print(len(labels), "grid cases")


def merge(parts):
	rec = {}
	for p in parts:
		with np.load(p) as z:
			rec.update({k: z[k] for k in z.files})
	np.savez_compressed(GOLDEN, **rec)
	print(GOLDEN, GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
	mode = sys.argv[1]
	if mode == "live":
		live(sys.argv[2], sys.argv[sys.argv.index("--lib") + 1], True)
	elif mode == "facts":
		live(sys.argv[2], None, False)
	elif mode == "grid":
		grid(sys.argv[2])
	else:
		merge(sys.argv[2:])
