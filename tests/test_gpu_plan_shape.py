"""A live plan is what plan_shape() says (csrc/slq_plan_shape.hpp), and computes what the plans of the commit before plan_shape()
computed. Small operators only (tests/_plan_cases.py: GPU_CASES): a 96 x 96 2-D Laplacian on ring-fed tiles at 128, 64, 32 and 16
probes (the tiles as clustered, then the merged streams R = 2 and 4: in fp64 those are 64 and 32 probes, so 32 is
there beside the 16 of a panel no tile stream serves), on barrier tiles and without tiles; a 20^3 3-D Laplacian
(pipelined row loop); a dense operator n = 300 in fp64 at 64 and 16 probes and in fp32; a Gram operator; a recompute plan, a
Chebyshev plan and a Chebyshev action plan.

Per case:
 * slq_debug_plan_shape(facts of the plan) == the shape of the plan (slq_debug_plan_shape_of): creation consumed the pure function;
 * describe(), basis mode, workspace bytes and the dense path equal the shape's fields - and what the parent's library reported for
   the same plan (tests/golden/plan_shape_golden.npz, recorded on the device from that library);
 * the arrays of one 12-step run (tridiagonals and log quadrature; the moments of a Chebyshev plan; the action of an action plan)
   are array_equal to the parent's: the grids decide the order of every partial sum, so this is the bitwise tie to them."""

from pathlib import Path

import numpy as np
import pytest

import _plan_cases as pc

pytestmark = pytest.mark.gpu

LANES = {"lap96_t2_p128": (64, 1, 1), "lap96_t2_p64": (32, 2, 2), "lap96_t2_p32": (16, 4, 3), "lap96_t2_p16": (8, 0, 0), "lap96_t1_p128": (64, 1, 0),
         "lap96_t0_p128": (64, 0, 0)}  # fmt: skip
GOLDEN = Path(__file__).resolve().parent / "golden" / "plan_shape_golden.npz"


@pytest.fixture(scope="module")
def golden():
	with np.load(GOLDEN) as z:
		return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def operator_of():
	from primate_amd.engine import Context, DeviceOperator

	ctx = Context(device=0)
	ops = {}

	def get(name, tiles, dtype):
		if (name, tiles, dtype) not in ops:
			with pc.tiles_env(tiles):
				ops[name, tiles, dtype] = DeviceOperator(pc.gpu_matrix(name), dtype=np.float64 if dtype == "f64" else np.float32, ctx=ctx)
		return ops[name, tiles, dtype]

	yield get
	for op in ops.values():
		op.close()


@pytest.mark.parametrize("label", list(pc.GPU_CASES))
def test_live_plan_is_its_shape_and_runs_as_before(label, operator_of, golden):
	opname, tiles, dtype, kind, nprobes = pc.GPU_CASES[label]
	op = operator_of(opname, tiles, dtype)
	call = pc.shape_call()
	with pc.tiles_env(tiles):
		plan = pc.gpu_plan(op, kind, nprobes)
		fa, sa = pc.shape_of_plan(plan)
		again = call(fa)  # (under the switches the plan was created with)
	try:
		assert np.array_equal(again, sa)
		assert np.array_equal(fa, golden[f"{label}/facts"])
		s = dict(zip(pc.SHAPE, (int(v) for v in sa)))
		f = dict(zip(pc.FACTS, fa))
		d = plan.describe()
		assert (d["panel_width"], d["panels"], d["ring_slots"], d["pipelined"]) == (s["PW"], s["NP"], s["S"], s["pipelined"])
		assert d["tiles"] == (0 if s["ringR"] == 0 else (2 if f["tiles_ringed"] else 1)) and d["upper_alpha"] == f["upper"] and d["far_per_row"] == f["far_per_row"]
		assert (d["dense_kernel"], d["dense_ksplit"]) == (s["dense_class"], s["dense_ks"]) and (d["omega"] != 0) == bool(s["omega_on"])
		info = plan.basis_info()
		assert info == {"mode": {pc.KEEP: 1, pc.RECOMPUTE: 2}.get(kind, 0), "ring_slots": s["S"], "acc_cols": s["acc_cols"]}
		assert plan.workspace_bytes == sum(s[f"ws_{r}_bytes"] for r in pc.COUNTED)
		## ... and the parent's library said the same of the same plan
		assert np.array_equal(pc.describe_array(plan), golden[f"{label}/describe"])
		assert info["mode"] == int(golden[f"{label}/basis_mode"]) and plan.workspace_bytes == int(golden[f"{label}/workspace_bytes"])
		want = golden[f"{label}/shape"]
		known = ~np.isnan(want)
		assert np.array_equal(sa[known], want[known])
		## what the cases are there for: the tiles as clustered, the merged streams of R = 2 and 4, and a panel too narrow for any
		if label in LANES:
			assert (s["LPR"], s["ringR"], s["stream"]) == LANES[label], label
		got = pc.gpu_run(plan, kind, pc.gpu_probes(op.shape[0], nprobes))
		for k, v in got.items():
			assert np.array_equal(v, golden[f"{label}/run_{k}"], equal_nan=True), k
	finally:
		plan.close()
