"""What creating a plan decides, without a device: `slq_debug_plan_shape` (csrc/slq_plan_shape.hpp: plan_shape) over a grid of
facts that turns every branch (tests/_plan_cases.py: five plan kinds, both dtypes, every lanes-per-row, CSR without tiles / with
barrier tiles / with ring-fed tiles and their streams, dense, Gram, callback, two CU counts, the switches that enter the shape).

Asserted on every case: the invariants the kernels rely on; the public byte queries against the shape's ring region; the
workspace sum against its formula; a transcription of the estimates of the one-shot entries as the commit before plan_shape()
computed them (`parent_*` below, written from that commit's slq.hip the way test_sequence_cpu.py transcribes its sequence);
equality with tests/golden/plan_shape_golden.npz.

What the golden proves. Its `live` part was recorded on the device from the library of the commit BEFORE plan_shape() existed:
the fields of live plans (tests/golden/make_golden_plan_shape.py). `test_live_plans_of_the_parent` feeds the facts of the same
plans to plan_shape() and compares every value that commit kept: that is the proof that the function computes what creation
computed. Its `grid` part was recorded from this tree: it guards later changes, it does not prove the first one."""

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import _plan_cases as pc
from _plan_cases import CHEB, CHEB_ACTION, F64, KEEP, OP_CSR, OP_DENSE, OP_GRAM, RECOMPUTE, RING
from primate_amd import _capi

GOLDEN = Path(__file__).resolve().parent / "golden" / "plan_shape_golden.npz"


@pytest.fixture(scope="module")
def grid():
	"""[(label, switches, facts dict, shape dict)] of the whole grid, computed once."""
	call = pc.shape_call()
	out = []
	for label, sw, f in pc.cpu_grid():
		with pc.switches(sw):
			s = call(pc.facts_array(f))
		out.append((label, sw, f, dict(zip(pc.SHAPE, (int(v) for v in s)))))
	return out


@pytest.fixture(scope="module")
def golden():
	with np.load(GOLDEN) as z:
		return {k: z[k] for k in z.files}


def esz(f):
	return 8 if f["dtype"] == F64 else 4


def test_grid_turns_every_branch(grid):
	seen = {k: set() for k in ("LPR", "ringR", "stream", "rs_upper", "pipelined", "dense_class", "omega_on", "gram", "gram_csr", "alpha_pad", "dense_ks")}
	for _, _, f, s in grid:
		for k in seen:
			seen[k].add(int(s[k]))
	assert seen["LPR"] == {8, 16, 32, 64} and seen["ringR"] == {0, 1, 2, 4} and seen["stream"] == {0, 1, 2, 3}
	assert seen["rs_upper"] == {0, 1} and seen["pipelined"] == {0, 1} and seen["dense_class"] == {0, 1, 2, 3, 4, 5}
	assert seen["omega_on"] == {0, 1} and seen["gram"] == {0, 1} and seen["gram_csr"] == {0, 1} and seen["alpha_pad"] == {0, 65536}
	assert {0, 1, 7, 16} <= seen["dense_ks"] and len(grid) > 5000


def test_invariants_the_kernels_rely_on(grid):
	for label, _, f, s in grid:
		for g in ("nblkA", "nblkU", "nblkF", "nblkT"):
			assert s[g] > 0 and s[g] % 8 == 0, (label, g)
		assert s["nblkS"] > 0, label
		if f["has_tiles"]:
			per_xcd = min(max(1, s[f"rs_xcd{x + 1}"] - s[f"rs_xcd{x}"]) for x in range(8))
			assert s["nblkT"] // 8 <= per_xcd, label
		assert s["part_maxblk"] == max(s[g] for g in ("nblkA", "nblkS", "nblkU", "nblkF", "nblkT")), label
		assert s["bpad"] == s["NP"] * s["PW"] >= f["nprobes"] > s["bpad"] - s["PW"], label
		assert s["PW"] == s["LPR"] * (2 if f["dtype"] == F64 else 4), label
		## the blocks carved out of `scal`: disjoint, ordered, and they end at the region's size
		offs = [s[f"scal_{k}"] for k in pc.SCAL]
		assert offs[0] == 0 and all(a < b or (i == 1 and f["orth"] == 0) for i, (a, b) in enumerate(zip(offs, offs[1:]))), label
		assert s["scal_nu"] - s["scal_nu_margin"] == f["orth"] * s["bpad"] and s["scal_end"] - s["scal_gamma"] == s["rmax"] * s["bpad"], label
		assert s["scal_end"] * 8 == s["ws_scal_bytes"], label
		assert (s["active_steps"], s["active_fail"], s["active_ring_fail"], s["active_fail2"]) == (s["bpad"], 2 * s["bpad"], 2 * s["bpad"] + 1, 2 * s["bpad"] + 2), label
		assert s["active_fail2"] < s["active_end"] and s["active_end"] * 4 == s["ws_active_bytes"], label
		## every ring slot, and the panels of an action, lie inside the ring region (a Ring or Chebyshev plan has no action: its
		## v_slot / y_slot are never read)
		slot = s["slot_stride"] * esz(f)
		assert s["S"] >= 2 and s["S"] * slot <= s["ws_ring_bytes"], label
		if f["plan"] in (KEEP, RECOMPUTE, CHEB_ACTION):
			assert 0 <= s["v_slot"] and 0 <= s["y_slot"] and (max(s["v_slot"], s["y_slot"]) + 1) * slot <= s["ws_ring_bytes"], label
		if f["plan"] == RECOMPUTE:
			assert s["S"] >= s["acc_cols"] + 1 and s["S"] <= s["v_slot"] < s["y_slot"], label
		assert [s[f"ws_{r}_id"] for r in pc.REGIONS] == list(range(len(pc.REGIONS))), label
		assert [r for r in pc.REGIONS if s[f"ws_{r}_counted"]] == [r for r in pc.REGIONS if r in pc.COUNTED], label
		assert (s["ws_T_bytes"] == 0) == (f["kind"] == OP_CSR) and (s["ws_T2_bytes"] != 0) == (f["kind"] == OP_GRAM), label
		assert (s["stream"] == 0) == (s["ringR"] == 0 or not f["tiles_ringed"]), label
		if s["ringR"] > 1:
			assert s["stream"] == (2 if s["ringR"] == 2 else 3) and f[f"merged{0 if s['ringR'] == 2 else 1}_available"], label


## ---- the commit before plan_shape(), transcribed --------------------------------------------------------------------
def parent_geometry(sw, dtype, nprobes):
	V = 2 if dtype == F64 else 4
	lpr = 8
	while lpr < 64 and lpr * V < nprobes:
		lpr *= 2
	if int(sw.get("SLQ_LPR", 0)) in (8, 16, 32, 64):
		lpr = int(sw["SLQ_LPR"])
	PW = lpr * V
	return lpr, PW, (nprobes + PW - 1) // PW


def parent_ring_slots(deg, orth, keep):
	return deg + 1 if keep else (2 if orth == 0 else max(orth + 1, 3))


def parent_query_bytes(sw, f, keep):
	_, PW, NP = parent_geometry(sw, f["dtype"], f["nprobes"])
	return parent_ring_slots(f["deg"], f["orth"], keep) * NP * f["n"] * PW * esz(f)


def parent_query_bytes_recompute(sw, f):
	_, PW, NP = parent_geometry(sw, f["dtype"], f["nprobes"])
	S = max(parent_ring_slots(f["deg"], f["orth"], 0), min(pc.K_ACC_COLS, f["deg"]) + 1) + 2
	return S * NP * f["n"] * PW * esz(f)


def parent_plan_bytes_on(sw, f, keep):
	b = parent_query_bytes(sw, f, keep)
	_, PW, NP = parent_geometry(sw, f["dtype"], f["nprobes"])
	panel = NP * PW * esz(f)
	if f["kind"] != OP_CSR:
		big_tiles = f["kind"] == OP_DENSE and (f["dtype"] != F64 or PW >= 32)
		b += (1 + (16 if big_tiles else 0)) * panel * f["n"]
	if f["kind"] == OP_GRAM:
		b += panel * f["mrows"]
	return b


def parent_plan_bytes_on_mode(sw, f, mode):
	b = parent_plan_bytes_on(sw, f, mode == 1)
	if mode == 2:
		b += parent_query_bytes_recompute(sw, f) - parent_query_bytes(sw, f, 0)
	return b


def parent_workspace_bytes(f, s):
	"""p->bytes of that commit's plan_create_mode, from the values it summed."""
	cheb, recompute = f["plan"] in (CHEB, CHEB_ACTION), f["plan"] == RECOMPUTE
	bp, deg, orth, e = s["bpad"], f["deg"], f["orth"], esz(f)
	hist = 0 if cheb else deg
	ring = (s["S"] + (2 if recompute else (1 if f["plan"] == CHEB_ACTION else 0))) * s["slot_stride"] * e
	ncoef = deg * bp if recompute else 0
	nscal = ((hist + 1) * 2 + orth + 1 + 2 + 1 + 1 + 2 * (pc.K_FUSED_MAX_R + 1) + s["rmax"]) * bp
	npart = pc.K_REORTH_CHUNK * s["part_maxblk"] * bp
	t_slabs = 0 if f["kind"] == OP_CSR else 1 + s["dense_ks"]
	t2 = s["NP"] * f["mrows"] * s["PW"] * e if f["kind"] == OP_GRAM else 0
	nmom = 2 * deg + 1 if cheb else 0
	return ring + ncoef * 8 + nscal * 8 + npart * 8 + (bp + 2 * bp * hist) * 8 + t_slabs * s["slot_stride"] * e + t2 + nmom * bp * 8


def head_estimate(f, s):
	"""plan_estimate_bytes of the header, from the shape's fields."""
	return s["ws_ring_bytes"] + s["t_slabs_bound"] * s["slot_stride"] * esz(f) + s["ws_T2_bytes"]


def test_estimates_and_workspace_against_the_parent_transcribed(grid):
	for label, sw, f, s in grid:
		assert sum(s[f"ws_{r}_bytes"] for r in pc.COUNTED) == parent_workspace_bytes(f, s), label
		## the bound of the one-shot entries' estimate covers the exact T, whatever dense_ks the search found
		assert s["t_slabs_bound"] * s["slot_stride"] * esz(f) >= s["ws_T_bytes"] and 0 <= s["dense_ks"] <= 16, label
		if f["kind"] != OP_CSR:
			assert s["ws_T_bytes"] == (1 + s["dense_ks"]) * s["slot_stride"] * esz(f), label
		mode = {RING: 0, KEEP: 1, RECOMPUTE: 2}.get(f["plan"])
		if mode is None:
			continue
		assert head_estimate(f, s) == parent_plan_bytes_on_mode(sw, f, mode), label
		if mode < 2:
			assert head_estimate(f, s) == parent_plan_bytes_on(sw, f, mode == 1), label


def test_public_byte_queries_are_the_ring_region(grid):
	"""slq_plan_query_bytes / _recompute take no operator: they answer with the ring region of the shape of (dtype, n, nprobes, deg,
	orth, kind) alone, so the region of every grid case - whatever its operator, CU count and streams - must equal the query's."""
	L = _capi.lib()
	b = C.c_size_t()
	for label, sw, f, s in grid:
		if f["plan"] in (CHEB, CHEB_ACTION):
			continue
		with pc.switches(sw):
			if f["plan"] == RECOMPUTE:
				assert L.slq_plan_query_bytes_recompute(f["dtype"], f["n"], f["nprobes"], f["deg"], f["orth"], C.byref(b)) == _capi.SLQ_OK
				assert b.value == parent_query_bytes_recompute(sw, f), label
			else:
				assert L.slq_plan_query_bytes(f["dtype"], f["n"], f["nprobes"], f["deg"], f["orth"], int(f["plan"] == KEEP), C.byref(b)) == _capi.SLQ_OK
				assert b.value == parent_query_bytes(sw, f, f["plan"] == KEEP), label
		assert b.value == s["ws_ring_bytes"], label


def test_recompute_query_is_independent_of_deg_above_the_accumulation_width():
	L = _capi.lib()
	got = set()
	for deg in (pc.K_ACC_COLS, pc.K_ACC_COLS + 1, 30, 512, 100000):  # (the query answers beyond kMaxDeg: a footprint, not a plan)
		b = C.c_size_t()
		assert L.slq_plan_query_bytes_recompute(F64, 10**6, 100, deg, 3, C.byref(b)) == _capi.SLQ_OK
		got.add(b.value)
	assert got == {(pc.K_ACC_COLS + 1 + 2) * 128 * 10**6 * 8}
	b = C.c_size_t()
	assert L.slq_plan_query_bytes(F64, (3 << 31), 100, 40, 5, 0, C.byref(b)) == _capi.SLQ_OK and b.value == 6 * 128 * (3 << 31) * 8  # (n beyond 2^31)
	assert L.slq_plan_query_bytes(F64, 1000, 100, pc.K_MAX_DEG + 1, 5, 0, C.byref(b)) == _capi.SLQ_EINVAL
	assert L.slq_plan_query_bytes(F64, 0, 100, 40, 5, 0, C.byref(b)) == _capi.SLQ_EINVAL and L.slq_plan_query_bytes(F64, 10, 10, 4, 2, 0, None) == _capi.SLQ_EINVAL


def test_debug_entry_checks_its_arguments():
	L = _capi.lib()
	dp = C.POINTER(C.c_double)
	f = pc.facts_array(pc.request(pc.operators()["csr5"], F64, 256, 8, 30, 3, RING))
	out = np.empty(pc.NS)
	ok = lambda fa, nf, ns: L.slq_debug_plan_shape(np.ascontiguousarray(fa).ctypes.data_as(dp), nf, out.ctypes.data_as(dp), ns)  # noqa: E731
	assert ok(f, pc.NF, pc.NS) == _capi.SLQ_OK
	assert ok(f, pc.NF - 1, pc.NS) == _capi.SLQ_EINVAL and ok(f, pc.NF, pc.NS + 1) == _capi.SLQ_EINVAL
	for name, bad in (("kind", 5), ("dtype", 2), ("plan", 5), ("n", 0), ("nprobes", 0), ("deg", 0), ("num_cus", 0)):
		g = f.copy()
		g[pc.FACTS.index(name)] = bad
		assert ok(g, pc.NF, pc.NS) == _capi.SLQ_EINVAL, name
	assert L.slq_debug_plan_shape_of(None, out.ctypes.data_as(dp), pc.NF, out.ctypes.data_as(dp), pc.NS) == _capi.SLQ_EINVAL


def test_live_plans_of_the_parent(golden):
	"""plan_shape() on the facts of live plans against the fields the parent's creation left in the same plans (NaN: no such field)."""
	call = pc.shape_call()
	for label, (_, tiles, _, _, _) in pc.GPU_CASES.items():
		with pc.switches({} if tiles is None else {"SLQ_TILES": tiles}):
			s = call(golden[f"{label}/facts"])
		want = golden[f"{label}/shape"]
		known = ~np.isnan(want)
		assert known.sum() >= 26 + 18 + 6 + 16 + 8 + 3, label  # (every named field of that commit's plan)
		bad = [(pc.SHAPE[i], s[i], want[i]) for i in np.flatnonzero(known) if s[i] != want[i]]
		assert not bad, (label, bad)
		d = dict(zip(pc.SHAPE, s))
		assert sum(d[f"ws_{r}_bytes"] for r in pc.COUNTED) == int(golden[f"{label}/workspace_bytes"]), label
		## the parent recorded a region's size as 0 where it had not allocated it
		assert [d[f"ws_{r}_bytes"] > 0 for r in pc.REGIONS] == [not (w == 0) for w in want[[pc.SHAPE.index(f"ws_{r}_bytes") for r in pc.REGIONS]]], label


def test_grid_equals_the_golden(grid, golden):
	labels = [g[0] for g in grid]
	assert labels == list(golden["grid_labels"])
	got = np.array([[g[3][k] for k in pc.SHAPE] for g in grid])
	want = golden["grid_shapes"]
	bad = np.argwhere(got != want)
	assert bad.size == 0, [(labels[i], pc.SHAPE[j], got[i, j], want[i, j]) for i, j in bad[:10]]
