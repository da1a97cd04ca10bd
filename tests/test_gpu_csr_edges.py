"""CSR operators on the inputs the C-ABI admits and no other GPU test feeds - rows unsorted, reversed, with duplicate columns, stored
zeros, cancelling pairs, empty rows, rows of hundreds of entries (tests/_csr_cases.py; its models are checked by tests/test_csr_cases_cpu.py) -
through every product, every update pass and every Lanczos pass, in every column. Every spelling reaches the library unchanged, by both
creation entries: slq_csr_create on the raw host arrays (through ctypes: engine.DeviceOperator sorts a SciPy matrix) and slq_csr_create_device
on a torch sparse-CSR tensor. Every item first asserts WHICH path its plan takes (describe(), _plan_cases.shape_of_plan), written down here from
the switch table of DESIGN.md §5.4: a switch that is silently ignored would turn the item into a repeat of the default path. Each prints
its worst ratio on a `[csr-edges]` line before it asserts (`-s` shows them).

 (a) the product, bitwise: integer operands, every partial sum an exact float, so matmat equals the int64 product in any summation order.
 (b) every update pass, bitwise: the Chebyshev action with bounds (-16, 16) is the update pass with constant power-of-two coefficients; with
     coef = e_k it returns w_k of the exact integer recurrence, for as many steps as the model proves every partial sum representable.
 (c) every Lanczos pass, every column: alpha_j, beta_j against oracle.lanczos on the canonical spelling, at the bars of test_gpu_dense.py (c).
 (d) the affine and Gram operators on irregular input, through ctypes (the engine sorts their inputs)."""

import ctypes as C

import numpy as np
import pytest

import _csr_cases as cc
from _plan_cases import FACTS, SHAPE, shape_of_plan

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
DTYPES = [F64, F32]
ENTRIES = ("host", "device")
SWITCHES = ("SLQ_TILES", "SLQ_REORDER", "SLQ_PIPE", "SLQ_FUSED", "SLQ_RING_GEN", "SLQ_DEVICE_BUILD", "SLQ_GRAM_CSR", "SLQ_MERGED", "SLQ_MGS",
            "SLQ_SYM_ALPHA", "SLQ_RING_ALPHA", "SLQ_RING_DEEP", "SLQ_STORED_U", "SLQ_GRAM", "SLQ_LPR", "SLQ_NT", "SLQ_RING_NARROW", "SLQ_OMEGA")  # fmt: skip
BOUNDS = (-cc.H, cc.H)


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


@pytest.fixture
def variant_env(monkeypatch):
	def set_variant(variant):
		for k in SWITCHES:
			monkeypatch.delenv(k, raising=False)
		for k, x in variant.items():
			monkeypatch.setenv(k, x)

	return set_variant


def _vid(v):
	return ",".join(f"{k[4:]}={x}" for k, x in v.items()) or "default"


def _dt(dtype):
	return np.dtype(dtype).name


# ---- the two creation entries ------------------------------------------------------------------------------------------------
def _shell(eng, ctx, h, dtype, n, nnz, kind):
	"""The C handle under the Python surface (DeviceOperator itself canonicalises what it is given)."""
	op = object.__new__(eng.DeviceOperator)
	op.ctx, op.dtype, op.shape, op._keep, op.kind, op.nnz, op._h = ctx, np.dtype(dtype), (n, n), [], kind, nnz, h
	return op


def make_operator(eng, R, dtype, entry):
	"""The spelling R as it is: entry "host" - slq_csr_create on its arrays; "device" - a torch sparse-CSR tensor on the GPU, whose arrays
	engine.DeviceOperator hands to slq_csr_create_device untouched. Returns (operator, what must outlive its creation)."""
	from primate_amd import _capi

	n, vals = R.M.n, R.vals(dtype)
	if entry == "host":
		ctx = eng.default_context()
		h = C.c_void_p()
		_capi.check(_capi.lib().slq_csr_create(ctx._h, _capi.dtype_id(dtype), n, R.nnz, _capi.ptr(R.rowptr), _capi.ptr(R.colind), _capi.ptr(vals), C.byref(h)))
		return _shell(eng, ctx, h, dtype, n, R.nnz, "csr"), (vals,)
	import torch

	crow, col, val = (torch.from_numpy(z.copy()).to("cuda") for z in (R.rowptr, R.colind, vals))
	t = torch.sparse_csr_tensor(crow, col, val, size=(n, n), check_invariants=False)
	assert np.array_equal(t.col_indices().cpu().numpy(), R.colind) and np.array_equal(t.values().cpu().numpy(), vals)  # (torch left the spelling alone)
	op = eng.DeviceOperator(t)
	assert op.nnz == R.nnz
	return op, (t,)


def plan_facts(plan):
	"""(describe(), the plan's facts by name, its shape by name)"""
	fa, sa = shape_of_plan(plan)
	return plan.describe(), dict(zip(FACTS, fa)), dict(zip(SHAPE, sa))


def geometry(dtype, P):
	"""(lanes per row, panel width, panels) of P probes."""
	V = 2 if np.dtype(dtype) == np.dtype(F64) else 4
	lpr = 8
	while lpr < 64 and lpr * V < P:
		lpr *= 2
	return lpr, lpr * V, -(-P // (lpr * V))


# ---- what a plan must report, from the switch table and the rules of §4.6 / §5.3 - not from slq.hip -------------------
def expected_upper(R, variant, permuted):
	"""Whether the operator keeps an upper-triangle copy: an exactly symmetric CSR whose stored rows are sorted and free of duplicates, unless
	SLQ_SYM_ALPHA=0. A builder that permutes the rows (SLQ_REORDER=2, tiles) sorts every stored row on the way - equal columns in the caller's
	order -, so a shuffled or reversed spelling is stored sorted; duplicates and the cancelling pairs of `zeros` stay."""
	if not (R.M.symmetric and R.nnz > 0) or variant.get("SLQ_SYM_ALPHA") == "0":
		return 0
	return int(cc.stored_exactly_symmetric(R, rows_sorted_by_builder=permuted))


def expected_sequence(variant, orth, upper, tiles, ringed_gram_ok, far_gt4):
	"""describe()["sequence"] of a plan on a CSR operator. orth = 0 also stands for a Chebyshev plan (its step is the orth-0 update pass)."""
	if variant.get("SLQ_FUSED") == "0" or variant.get("SLQ_MGS") == "1":
		return "sweeps"
	merged = variant.get("SLQ_MERGED") != "0"
	if far_gt4:  # the gathers are not served from cache: one gather pass per step that stores u, where there is something to project on
		return "fused_stored_u" if (orth >= 1 and merged and variant.get("SLQ_STORED_U") != "0" and not tiles) else "sweeps"
	if orth == 0 or not upper or not merged or variant.get("SLQ_GRAM") == "0":
		return "fused"
	if tiles == 2:
		return "fused_gram" if ringed_gram_ok else "fused"
	if tiles == 1:
		return "fused"
	return "fused_gram" if variant.get("SLQ_GRAM_CSR") != "0" else "fused"


def assert_path(what, R, dtype, variant, P, orth, d, f, s, want_tiles):
	"""The path assertions shared by (b) and (c). want_tiles: the value the plan must report, or None where the library may decline
	(a row longer than a tile's caps, scattered rows): then only consistency is required. Returns the tiles value."""
	lpr, pw, npan = geometry(dtype, P)
	assert (d["panel_width"], d["panels"]) == (pw, npan) and s["LPR"] == lpr, (what, d)
	if want_tiles is not None:
		assert d["tiles"] == want_tiles, f"{what}: tiles {d['tiles']}, asked for {want_tiles} ({d})"
	tiles = d["tiles"]
	asked = int(variant.get("SLQ_TILES", "0"))
	assert tiles in (0, asked), (what, d)
	assert tiles == 0 or f["has_tiles"] == 1, (what, f)
	if tiles:
		assert f["tiles_ringed"] == (1 if tiles == 2 else 0) and s["ringR"] == 64 // lpr and d["reordered"] == 1, (what, s)
		if tiles == 2:
			want_gen = 0 if (variant.get("SLQ_RING_GEN") == "0" and lpr == 64) else 1
			want_deep = 0 if variant.get("SLQ_RING_DEEP") == "0" else 1
			assert (s["ring_gen"], s["ring_deep"]) == (want_gen, want_deep), f"{what}: ring_gen {s['ring_gen']}, ring_deep {s['ring_deep']}"
	else:
		assert s["ringR"] == 0, (what, s)
		if not f["has_tiles"]:
			assert d["reordered"] == (1 if variant.get("SLQ_REORDER") == "2" and R.nnz > 0 else 0), (what, d)
	pipe = variant.get("SLQ_PIPE")
	want_pipe = lpr == 64 and ((pipe != "0") if pipe is not None else R.nnz / R.M.n > 5.5)
	assert d["pipelined"] == int(want_pipe) == s["pipelined"], f"{what}: pipelined {d['pipelined']}, expected {int(want_pipe)}"
	upper = expected_upper(R, variant, d["reordered"] == 1)
	assert d["upper_alpha"] == upper == f["upper"], f"{what}: upper {d['upper_alpha']}, expected {upper} for the {R.spelling} spelling"
	far_gt4 = d["far_per_row"] > 4.0
	if not d["reordered"]:
		far = np.count_nonzero(np.abs(R.rows - R.colind) > 4096) / R.M.n
		assert d["far_per_row"] == pytest.approx(far, rel=1e-12), (what, d["far_per_row"], far)
		assert far_gt4 == (R.M.name.startswith("far7")), (what, far)
	gram_ok = tiles == 2 and s["ring_gen"] == 1 and s["ring_deep"] == 1
	seq = expected_sequence(variant, orth, upper, tiles, gram_ok, far_gt4)
	assert d["sequence"] == seq, f"{what}: sequence {d['sequence']}, expected {seq} (upper {upper}, tiles {tiles}, far {d['far_per_row']:.2f})"
	if variant.get("SLQ_GRAM_CSR") == "0":
		assert s["gram_csr"] == 0, (what, s["gram_csr"])
	return tiles


def first_difference(Y, ref, R):
	bad = np.argwhere(Y != ref)
	i, c = (int(x) for x in bad[0])
	cols = R.colind[R.rowptr[i] : R.rowptr[i + 1]].tolist()
	return (f"{len(bad)} of {Y.size} entries differ; rows {bad[:, 0].min()}..{bad[:, 0].max()}, columns {bad[:, 1].min()}..{bad[:, 1].max()}; first at row {i}, "
	        f"column {c}: got {Y[i, c]!r}, exact {ref[i, c]!r}; row {i} stores columns {cols[:12]}{'...' if len(cols) > 12 else ''}")  # fmt: skip


# ---- (a) -----------------------------------------------------------------------------------------------------------------------
PS_A = (1, 17, 130)
_PRODUCT = {}


def product_case(name, spelling):
	"""Integer X (130 columns, |x| <= 7) and the exact product of the spelling as stored; shared, never written to."""
	key = (name, spelling)
	if key not in _PRODUCT:
		R = cc.raw(name, spelling)
		X = cc.int_panel(R.M.n, max(PS_A), 1)
		Y, bits = cc.exact_product(R, X)
		assert bits < 24  # every partial sum is an exact float in both dtypes
		for Z in (X, Y):
			Z.setflags(write=False)
		_PRODUCT[key] = (R, X, Y)
	return _PRODUCT[key]


@pytest.mark.parametrize("reorder", ["0", "2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_product_is_exact_for_every_spelling(eng, variant_env, dtype, reorder):
	variant = {"SLQ_REORDER": reorder}
	variant_env(variant)
	failures, count = [], 0
	for name in cc.ALL_NAMES:
		for spelling in cc.SPELLINGS:
			R, X, ref = product_case(name, spelling)
			for entry in ENTRIES:
				op, keep = make_operator(eng, R, dtype, entry)
				plan = eng.LanczosPlan(op, 17, 1, 0)
				d = plan.describe()
				plan.close()
				what = f"{name} {spelling} {entry} {_dt(dtype)} REORDER={reorder}"
				assert d["reordered"] == (1 if reorder == "2" and R.nnz > 0 else 0) and d["tiles"] == 0, (what, d)
				for P in PS_A:
					Y = op.matmat(np.asfortranarray(X[:, :P].astype(dtype)))
					count += 1
					if not np.array_equal(Y, ref[:, :P]):
						msg = f"{what} P={P}: " + first_difference(Y, ref[:, :P], R)
						if not R.M.symmetric:
							D = np.zeros(R.M.shape, dtype=np.int64)
							np.add.at(D, (R.rows, R.colind.astype(np.int64)), R.num)
							msg += "; the product is A^T X" if np.array_equal(Y, D.T @ X[:, :P]) else "; it is not A^T X either"
						failures.append(msg)
					if R.M.nnz == 0:
						assert not np.any(Y), what
				op.close()
				del keep
	print(f"[csr-edges] check=a dtype={_dt(dtype)} variant={_vid(variant)} products={count} mismatches={len(failures)} worst=" + ("exact" if not failures else "WRONG"))
	assert not failures, "\n".join(failures[:20])


# ---- (b) -----------------------------------------------------------------------------------------------------------------------
GRIDS = ("grid64", "grid70")
TILED = GRIDS + ("longrow4096_17_130", "far")
# (variant, names, P in fp64, P in fp32). SLQ_PIPE acts on panels of 64 lanes per row (P > 64 in fp64, > 128 in fp32); barrier tiles (SLQ_TILES=1) serve
# those panels only; SLQ_TILES=2 at 20 / 40 / 130 probes in fp64 and 40 / 130 in fp32: merged tiles of 4 and 2 base tiles, and the base tiles.
VARIANTS_B = [
	({}, cc.CHEB_NAMES, (17, 130), (17, 130)),
	({"SLQ_PIPE": "0"}, ("band1000", "grid64", "far"), (130,), (130,)),
	({"SLQ_PIPE": "1"}, ("band1000", "grid64", "far"), (130,), (130,)),
	({"SLQ_FUSED": "0"}, cc.CHEB_NAMES, (17,), (17,)),
	({"SLQ_REORDER": "2"}, ("band1000", "grid64", "longrow4096_17_130"), (17,), (17,)),
	({"SLQ_TILES": "1"}, TILED, (130,), (130,)),
	({"SLQ_TILES": "2"}, TILED, (20, 40, 130), (40, 130)),
	({"SLQ_TILES": "2", "SLQ_RING_GEN": "0"}, TILED, (130,), (130,)),
	({"SLQ_TILES": "2", "SLQ_DEVICE_BUILD": "2"}, TILED, (20, 130), (40, 130)),
]
CASES_B = [(dt, v) for v in VARIANTS_B for dt in DTYPES]
_CHEB = {}


def cheb_case(name, dtype):
	"""Rademacher probes (130 columns) and the exact w_0 .. w_nsteps, moments and bounds of the canonical spelling - every spelling is the same
	matrix, and tests/test_csr_cases_cpu.py proves the bound for each of them. One family at a time is kept (11 panels of 8 MB)."""
	nsteps = cc.cheb_steps(name, dtype)
	key = (name, nsteps)
	if key not in _CHEB:
		_CHEB.clear()
		R = cc.raw(name, "canonical")
		V = cc.rademacher(R.M.n, 130, 0)
		m = cc.exact_chebyshev(R, V, nsteps)
		assert m["K"] == nsteps
		m["sum"] = np.sum(m["w"], axis=0)
		for Z in [V, m["sum"], m["mu"]] + m["w"]:
			Z.setflags(write=False)
		_CHEB[key] = (V, m)
	V, m = _CHEB[key]
	mant = cc.MANT[np.dtype(dtype)]
	assert cc.proven_steps(m["bits"], mant) == nsteps and m["sum_bits"] < mant, (name, m["bits"])
	return nsteps, V, m, [k for k in range(2 * nsteps + 1) if m["mu_bits"][k] < mant]


def tiles_report(variant, chosen, failures):
	"""What the library chose where it may decline (a spelling with duplicates has more entries per tile: it may be declined where the canonical
	one is not): both creation entries must agree, and the bits are held to the same reference either way. Returns the line for the log."""
	if "SLQ_TILES" not in variant:
		return ""
	for (name, spelling, P), t in sorted(chosen.items()):
		if len(t) != 1:
			failures.append(f"{name} {spelling} P={P}: the two creation entries got different tiles {sorted(t)}")
	names = sorted({(name, P) for name, _, P in chosen})
	return " ".join(f"{name}@P{P}:tiles=" + "/".join(str(min(chosen[(name, sp, P)])) for sp in cc.SPELLINGS) for name, P in names)


def want_tiles_of(variant, name):
	asked = int(variant.get("SLQ_TILES", "0"))
	return (asked if name in GRIDS else None) if asked else 0


@pytest.mark.parametrize("dtype,spec", CASES_B, ids=[f"{_dt(dt)}-{_vid(v[0])}" for dt, v in CASES_B])
def test_every_update_pass_is_exact(eng, variant_env, dtype, spec):
	"""coef = e_k returns w_k bit for bit in every row and column, coef = 1 the exact sum; the moments mu_k bitwise for the k whose sums the model proves exact."""
	variant, names, P64, P32 = spec
	variant_env(variant)
	failures, chosen, runs, moments = [], {}, 0, 0
	for name in names:
		nsteps, V, m, mu_proven = cheb_case(name, dtype)
		for spelling in cc.SPELLINGS:
			R = cc.raw(name, spelling)
			for entry in ENTRIES:
				op, keep = make_operator(eng, R, dtype, entry)
				for P in P64 if dtype == F64 else P32:
					what = f"{name} {spelling} {entry} {_dt(dtype)} {_vid(variant)} P={P}"
					plan = eng.ChebyshevPlan(op, P, nsteps, action=True)
					tiles = assert_path(what, R, dtype, variant, P, 0, *plan_facts(plan), want_tiles_of(variant, name))
					chosen.setdefault((name, spelling, P), set()).add(tiles)
					Vp = np.asfortranarray(V[:, :P].astype(dtype))
					for k in list(range(nsteps + 1)) + [None]:
						coef = np.ones(nsteps + 1) if k is None else np.eye(nsteps + 1)[k]
						ref = (m["sum"] if k is None else m["w"][k])[:, :P]
						plan.set_probes(Vp)  # (an action takes the probes set since the last run)
						Y = plan.action(BOUNDS, coef)
						runs += 1
						if not np.array_equal(Y, ref):
							failures.append(f"{what} " + ("sum of all w_k" if k is None else f"w_{k}") + ": " + first_difference(Y, ref, R))
							break
					mu = plan.moments()
					for k in mu_proven:
						moments += 1
						if not np.array_equal(mu[:, k], m["mu"][:P, k]):
							c = int(np.flatnonzero(mu[:, k] != m["mu"][:P, k])[0])
							failures.append(f"{what} mu_{k}: column {c} got {mu[c, k]!r}, exact {m['mu'][c, k]!r}")
							break
					plan.close()
				op.close()
				del keep
	picked = tiles_report(variant, chosen, failures)
	print(f"[csr-edges] check=b dtype={_dt(dtype)} variant={_vid(variant)} actions={runs} moments={moments} mismatches={len(failures)} worst=" + ("exact" if not failures else "WRONG") + (" " + picked if picked else ""))
	assert not failures, "\n".join(failures[:20])


# ---- (c) -----------------------------------------------------------------------------------------------------------------------
ORTHS = (0, 3, 5, 12)
SMALL = ("band5", "band65", "band1000", "longrow1000_0_999", "grid64")
TILED_C = GRIDS + ("longrow4096_17_130", "longrow4096_4000_300", "far")
VARIANTS_C = [
	({}, cc.LANCZOS_NAMES, (17,), (17,)),
	({"SLQ_PIPE": "0"}, ("band1000", "grid64", "far"), (130,), (130,)),
	({"SLQ_PIPE": "1"}, ("band1000", "grid64", "far"), (130,), (130,)),
	({"SLQ_FUSED": "0"}, SMALL + ("far7",), (17,), (17,)),
	({"SLQ_REORDER": "2"}, ("band65", "band1000", "grid64", "longrow4096_17_130"), (17,), (17,)),
	({"SLQ_TILES": "1"}, TILED_C, (130,), (130,)),
	({"SLQ_TILES": "2"}, TILED_C, (20, 40, 130), (40, 130)),
	({"SLQ_TILES": "2", "SLQ_RING_GEN": "0"}, TILED_C, (130,), (130,)),
	({"SLQ_TILES": "2", "SLQ_DEVICE_BUILD": "2"}, TILED_C, (20, 130), (40, 130)),
	({"SLQ_GRAM_CSR": "0"}, SMALL, (17,), (17,)),
	({"SLQ_MERGED": "0"}, SMALL, (17,), (17,)),
	({"SLQ_MGS": "1"}, SMALL, (17,), (17,)),
	({"SLQ_SYM_ALPHA": "0"}, SMALL, (17,), (17,)),
	({"SLQ_TILES": "2", "SLQ_RING_ALPHA": "1"}, GRIDS, (20, 130), (40, 130)),
	({"SLQ_TILES": "2", "SLQ_RING_DEEP": "0"}, GRIDS, (20, 130), (40, 130)),
	({"SLQ_STORED_U": "0"}, ("far7",), (17,), (17,)),
]
CASES_C = [(dt, v) for v in VARIANTS_C for dt in DTYPES]
_LANCZOS = {}


def lanczos_case(oracle, name, dtype, orth):
	"""The spd values of a family, Rademacher probes, and the oracle's alpha, beta and steps of every column on the canonical spelling, v^T A v beside them."""
	key = (name, _dt(dtype), orth)
	if key not in _LANCZOS:
		M = cc.family(name, "spd")
		n = M.n
		ncols = 130 if n >= 1000 else 17
		A = M.scipy(dtype)
		V = np.asfortranarray(cc.rademacher(n, ncols, 2).astype(dtype))
		deg = min(12, n)
		al, be = np.zeros((ncols, deg + 1), dtype), np.zeros((ncols, deg + 1), dtype)
		steps = np.zeros(ncols, dtype=np.int32)
		for c in range(ncols):
			Q = np.zeros((n, max(orth, 2)), dtype, order="F")
			steps[c] = oracle.lanczos(A, V[:, c].copy(), deg, 1e-8, min(orth, deg), al[c], be[c], Q)
		vAv = np.einsum("ij,ij->j", V.astype(F64), A.astype(F64) @ V.astype(F64))
		for Z in (V, al, be, steps, vAv):
			Z.setflags(write=False)
		_LANCZOS[key] = (V, deg, al, be, steps, vAv)
	return _LANCZOS[key]


@pytest.mark.parametrize("dtype,spec", CASES_C, ids=[f"{_dt(dt)}-{_vid(v[0])}" for dt, v in CASES_C])
def test_every_lanczos_pass_in_every_column(oracle, eng, variant_env, dtype, spec):
	"""Bars (test_gpu_dense.py check (c)): alpha, beta within 1e-10 (fp64) / 3e-4 (fp32) of the tridiagonal's largest entry, for every column,
	equal step counts; f = identity within 1e-11 (fp64; fp32: its bar) of v^T A v. The inputs are insensitive to the summation order at 1 / 100 of
	these bars (tests/test_csr_cases_cpu.py), so every spelling is held to the canonical spelling's reference. fp32 leaves n < 12 out."""
	variant, names, P64, P32 = spec
	variant_env(variant)
	bar = 1e-10 if dtype == F64 else 3e-4
	bar_id = 1e-11 if dtype == F64 else 3e-4
	worst = {"tridiag": (0.0, None), "identity": (0.0, None)}
	failures, chosen, sequences = [], {}, set()
	for name in names:
		n = cc.family(name, "spd").n
		if dtype == F32 and n < 12:
			continue
		for spelling in cc.SPELLINGS:
			R = cc.raw(name, spelling, "spd")
			for entry in ENTRIES:
				op, keep = make_operator(eng, R, dtype, entry)
				for P in P64 if dtype == F64 else P32:
					P = min(P, 17) if n < 1000 else P
					for orth in ORTHS:
						V, deg, al, be, steps, vAv = lanczos_case(oracle, name, dtype, orth)
						what = f"{name} {spelling} {entry} {_dt(dtype)} {_vid(variant)} P={P} orth={orth}"
						plan = eng.LanczosPlan(op, P, deg, orth)
						d, f, s = plan_facts(plan)
						tiles = assert_path(what, R, dtype, variant, P, min(orth, deg), d, f, s, want_tiles_of(variant, name))
						chosen.setdefault((name, spelling, P), set()).add(tiles)
						sequences.add((spelling, min(orth, 1), d["sequence"]))
						plan.set_probes(np.asfortranarray(V[:, :P]))
						plan.run()
						a, b, st = plan.tridiag()
						q_id = plan.quadrature("identity")
						plan.close()
						if not np.array_equal(st, steps[:P]):
							failures.append(f"{what}: steps {st} against the oracle's {steps[:P]}")
							continue
						scale = np.max(np.abs(al[:P, :deg]), axis=1, keepdims=True).astype(F64)
						ea = np.abs(a[:, :deg].astype(F64) - al[:P, :deg]) / scale
						eb = np.abs(b[:, :deg].astype(F64) - be[:P, :deg]) / scale
						e_tri = float(max(np.max(ea), np.max(eb)))
						e_id = float(np.max(np.abs(q_id / vAv[:P] - 1.0)))
						for kind, e, lim in (("tridiag", e_tri, bar), ("identity", e_id, bar_id)):
							if not e <= lim:  # (NaN fails)
								c = int(np.argmax(np.max(np.maximum(ea, eb), axis=1))) if kind == "tridiag" else int(np.argmax(np.abs(q_id / vAv[:P] - 1.0)))
								failures.append(f"{what}: {kind} error {e:.3e} above {lim:g} (column {c})")
							if not e / lim <= worst[kind][0]:
								worst[kind] = (float(e / lim), f"{name}/{spelling}/{entry}/P{P}/o{orth}")
				op.close()
				del keep
	if not variant:
		## the switch of sequence is asserted, not merely tolerated: on default switches a canonical symmetric spelling takes the Gram sequence, every
		## shuffled, reversed or duplicated one the merged sequence (assert_path held each plan to it; here: both occurred)
		assert ("canonical", 1, "fused_gram") in sequences and all((sp, 1, "fused") in sequences for sp in ("shuffled", "reversed", "dups")), sequences
		assert ("canonical", 1, "fused_stored_u") in sequences  # far7
	picked = tiles_report(variant, chosen, failures)
	print(f"[csr-edges] check=c dtype={_dt(dtype)} variant={_vid(variant)} " + " ".join(f"{k}={r:.4g}@{w}" for k, (r, w) in worst.items() if w) + (" " + picked if picked else ""))
	assert not failures, "\n".join(failures[:20])


# ---- (d) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_affine_operator_on_irregular_input(eng, dtype):
	"""slq_csr_affine_create with A shuffled and B with duplicates: matmat at t = 0, 1, -0.5 is the exact product of A + t B."""
	from primate_amd import _capi

	RA, RB = cc.raw("band1000", "shuffled"), cc.raw("longrow1000_999_65", "dups")
	n = 1000
	X = cc.int_panel(n, 17, 4)
	YA, ba = cc.exact_product(RA, X)
	YB, bb = cc.exact_product(RB, X)
	assert max(ba + RB.M.shift + 1, bb + 1) + 1 < 24  # (A X + t B X in units of half B's quantum, for t = -0.5: ba counts units of 1, bb of 2**-shift)
	ctx = eng.default_context()
	va, vb = RA.vals(dtype), RB.vals(dtype)
	h = C.c_void_p()
	_capi.check(_capi.lib().slq_csr_affine_create(ctx._h, _capi.dtype_id(dtype), n, RA.nnz, _capi.ptr(RA.rowptr), _capi.ptr(RA.colind), _capi.ptr(va),
	                                              RB.nnz, _capi.ptr(RB.rowptr), _capi.ptr(RB.colind), _capi.ptr(vb), C.byref(h)))  # fmt: skip
	op = _shell(eng, ctx, h, dtype, n, RA.nnz + RB.nnz, "affine")
	try:
		for t in (0.0, 1.0, -0.5):
			op.set_parameter(t)
			Y = op.matmat(np.asfortranarray(X.astype(dtype)))
			ref = YA + t * YB
			assert np.array_equal(Y, ref), f"t={t} {_dt(dtype)}: " + first_difference(Y, ref, RA)
	finally:
		op.close()
	print(f"[csr-edges] check=d dtype={_dt(dtype)} operator=affine worst=exact")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_gram_operator_on_irregular_input(eng, dtype):
	"""slq_csr_gram_create on a rectangular B with duplicate entries, in unsorted rows: the product is the exact B^T B X."""
	from primate_amd import _capi

	B = cc.rect(350, 200)
	R = cc.spell(B, "dups")
	X = cc.int_panel(200, 17, 5)
	T, b1 = cc.exact_product(R, X)
	D = np.zeros(B.shape, dtype=np.int64)
	np.add.at(D, (R.rows, R.colind.astype(np.int64)), np.abs(R.num))
	ref = R.dense_num().T @ T.astype(np.int64)
	assert b1 < 24 and float((D.T @ np.abs(T)).max()) < 2.0**24  # both products' partial sums are exact floats
	ctx = eng.default_context()
	vals = R.vals(dtype)
	h = C.c_void_p()
	_capi.check(_capi.lib().slq_csr_gram_create(ctx._h, _capi.dtype_id(dtype), 350, 200, R.nnz, _capi.ptr(R.rowptr), _capi.ptr(R.colind), _capi.ptr(vals), C.byref(h)))
	op = _shell(eng, ctx, h, dtype, 200, R.nnz, "gram")
	try:
		Y = op.matmat(np.asfortranarray(X.astype(dtype)))
		if not np.array_equal(Y, ref):
			bad = np.argwhere(Y != ref)
			pytest.fail(f"{_dt(dtype)}: {len(bad)} of {Y.size} entries differ, first at row {bad[0][0]}, column {bad[0][1]}: got {Y[tuple(bad[0])]}, exact {ref[tuple(bad[0])]}")
	finally:
		op.close()
	print(f"[csr-edges] check=d dtype={_dt(dtype)} operator=gram worst=exact")
