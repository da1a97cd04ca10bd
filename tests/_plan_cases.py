"""The cases of the plan-shape tests (tests/test_plan_shape_cpu.py, tests/test_gpu_plan_shape.py, tests/golden/make_golden_plan_shape.py):
the array orders of csrc/slq_plan_shape.hpp by name, the CPU grid of facts, the live operators of the GPU grid, and the ctypes calls.

The CPU grid. The full product of every operator, dtype, kind, probe count, deg, orth, CU count and switch is what
scripts/plan_shape_check.cpp runs (8e5 cases, a host program); one ctypes call each is too slow here and its golden too large, so
the grid is three products that share every assertion and together turn every branch:
 * "geometry": every operator x dtype x kind x probe count x CU count at deg 30, orth 3 (grids, tile stream, flags, T);
 * "depth": three operators x dtype x three probe counts x kind x every (deg, orth) (ring slots, the carved blocks, the tables' sizes);
 * "switch": every switch setting x every operator x dtype x three probe counts x two kinds at deg 30, orth 3."""

import ctypes as C
import itertools
import os

import numpy as np

from primate_amd import _capi

OP_CSR, OP_DENSE, OP_CALLBACK, OP_DEVICE_CALLBACK, OP_GRAM = range(5)
F32, F64 = 0, 1
RING, KEEP, RECOMPUTE, CHEB, CHEB_ACTION = range(5)
KINDS = (RING, KEEP, RECOMPUTE, CHEB, CHEB_ACTION)
K_ACC_COLS, K_CHEB_ACC_COLS, K_FUSED_MAX_R, K_REORTH_CHUNK, K_MAX_DEG = 8, 16, 8, 16, 512

_X9 = tuple(range(9))
# order of plan_facts_to_array
FACTS = (("kind", "dtype", "n", "nnz", "nnz_u", "upper", "mrows", "lda", "has_tiles", "tiles_ringed", "tiles_max_cols", "upper_per_row", "upper_stream",
          "upper_padded", "far_per_row", "affine") + tuple(f"xcd_tile{x}" for x in _X9) + tuple(f"xcd_tile_u{x}" for x in _X9)
         + tuple(f"merged{i}_{k}" for i in (0, 1) for k in ("available", "upper", "u_padded") + tuple(f"xcd_tile{x}" for x in _X9))
         + ("num_cus", "nprobes", "deg", "orth", "plan"))  # fmt: skip
REGIONS = ("ring", "scal", "part", "acc_coef", "sweep_cols", "om_buf", "om_flags", "om_cnt", "om_census", "active", "quad", "cheb_mu", "cheb_out",
           "cheb_coef", "T", "T2")  # fmt: skip
SCAL = ("alpha", "nu_margin", "nu", "vnorm2", "coefA", "coefB", "cross", "gram", "gamma", "end")
# order of plan_shape_to_array
SHAPE = (("LPR", "PW", "NP", "bpad", "S", "acc_cols", "v_slot", "y_slot", "slot_stride", "rmax", "hist", "pipelined", "nblkA", "nblkS", "nblkU", "nblkF",
          "nblkT", "alpha_pad", "part_maxblk", "dense_ks", "t_slabs_bound", "dense_class", "ringR", "stream", "rs_upper", "rs_u_padded", "ring_staged")
         + tuple(f"rs_xcd{x}" for x in _X9) + tuple(f"rs_xcd_u{x}" for x in _X9)
         + ("omega_on", "ring_gen", "ring_deep", "gram", "gram_csr", "last_nostore")
         + tuple(f"ws_{r}_{k}" for r in REGIONS for k in ("id", "bytes", "zeroed", "counted"))
         + tuple(f"scal_{k}" for k in SCAL) + ("active_steps", "active_fail", "active_ring_fail", "active_fail2", "active_end"))  # fmt: skip
NF, NS = len(FACTS), len(SHAPE)
assert NF == 63 and NS == 27 + 18 + 6 + 4 * 16 + 10 + 5
COUNTED = ("ring", "scal", "part", "acc_coef", "quad", "cheb_mu", "T", "T2")  # the regions of slq_plan_workspace_bytes

# every switch the grid turns, and the settings it takes
SWITCH_NAMES = ("SLQ_LPR", "SLQ_PIPE", "SLQ_TILES", "SLQ_DENSE_KSPLIT", "SLQ_DENSE_TILE16", "SLQ_DENSE_MFMA", "SLQ_OMEGA")
SWITCHES = ({},) + tuple({"SLQ_LPR": str(v)} for v in (8, 16, 32, 64)) + ({"SLQ_PIPE": "0"}, {"SLQ_PIPE": "1"}, {"SLQ_TILES": "0"}) + tuple(
	{"SLQ_DENSE_KSPLIT": str(v)} for v in (1, 7, 16)) + ({"SLQ_DENSE_TILE16": "1"}, {"SLQ_DENSE_MFMA": "0"}, {"SLQ_OMEGA": "2"})  # fmt: skip
PROBES = (1, 8, 16, 17, 32, 64, 128, 256, 257)  # every LPR of both dtypes, and a ragged last panel
DEGS, CHEB_DEGS, ORTHS = (1, 8, 9, 30, 512), (1, 8, 9, 30, 512, 16384), (0, 3, 6, None)  # (None: orth = deg)


def switch_label(sw: dict) -> str:
	return ",".join(f"{k}={v}" for k, v in sorted(sw.items())) or "default"


class switches:
	"""The environment with exactly `sw` of SWITCH_NAMES set, for the block (the library reads it at each call)."""

	def __init__(self, sw: dict):
		self.sw = sw

	def __enter__(self):
		self.had = {k: os.environ.get(k) for k in SWITCH_NAMES}
		for k in SWITCH_NAMES:
			os.environ.pop(k, None)
		os.environ.update(self.sw)

	def __exit__(self, *exc):
		for k, v in self.had.items():
			os.environ.pop(k, None)
			if v is not None:
				os.environ[k] = v


def _xcd(per_xcd: int) -> dict:
	return {x: x * per_xcd for x in _X9}


def _op(**kw) -> dict:
	f = dict.fromkeys(FACTS[:-5], 0)
	f.update(kind=OP_CSR)
	for k, v in kw.items():
		if isinstance(v, dict):  # a table of nine
			f.update({f"{k}{x}": t for x, t in v.items()})
		else:
			assert k in f, k
			f[k] = v
	return f


def _csr(n: int, nnz: int, upper: bool, **kw) -> dict:
	return _op(n=n, nnz=nnz, upper=int(upper), nnz_u=(nnz + n) // 2 if upper else 0, **kw)


def operators() -> dict:
	"""label -> operator facts. The same operators as scripts/plan_shape_check.cpp."""
	n2, n3 = 96 * 96, 20**3
	nnz5, nnz7 = 5 * n2 - 4 * 96, 7 * n3 - 6 * 400
	ops = {
		"csr5": _csr(n2, nnz5, True),  # no tiles; nnz / n < 5.5, upper gathers < 3.2
		"csr5_full": _csr(n2, nnz5, False),  # ... full rows: gathers > 3.2
		"csr7": _csr(n3, nnz7, True),  # nnz / n > 5.5 (pipelined), upper gathers > 3.2
		"csr5_far": _csr(n2, nnz5, True, far_per_row=6.0),  # gathers not served from cache
		"csr5_affine": _csr(n2, nnz5, True, affine=1),
	}
	for per_xcd in (48, 3):
		ops[f"barrier_{per_xcd}"] = _csr(n2, nnz5, True, has_tiles=1, tiles_max_cols=72, xcd_tile=_xcd(per_xcd))
	for us, upr, merged, per_xcd in itertools.product((0, 1), (2.0, 3.0), (0, 1), (83, 2)):  # upr: both sides of SLQ_RING_ALPHA_MAX_X100 / 100
		if not us and upr != 2.0:
			continue
		kw = dict(has_tiles=1, tiles_ringed=1, tiles_max_cols=36, xcd_tile=_xcd(per_xcd), upper_stream=us, upper_padded=us, upper_per_row=upr if us else 0.0)
		if us:
			kw["xcd_tile_u"] = _xcd((per_xcd + 1) // 2)
		if merged:
			for i in (0, 1):
				kw.update({f"merged{i}_available": 1, f"merged{i}_upper": us, f"merged{i}_u_padded": us, f"merged{i}_xcd_tile": _xcd(-(-per_xcd // (2 << i)))})
		ops[f"ringed_u{us}_upr{upr:g}_m{merged}_{per_xcd}"] = _csr(n2, nnz5, True, **kw)
	for lda in (300, 301):
		ops[f"dense_lda{lda}"] = _op(kind=OP_DENSE, n=300, nnz=300 * 300, lda=lda)
	ops["dense_5000"] = _op(kind=OP_DENSE, n=5000, nnz=5000 * 5000, lda=5000)
	ops["gram"] = _op(kind=OP_GRAM, n=200, mrows=350, nnz=1400)
	ops["callback"] = _op(kind=OP_CALLBACK, n=500)
	return ops


def request(op: dict, dtype: int, num_cus: int, nprobes: int, deg: int, orth, plan: int) -> dict:
	"""The facts of a plan on `op`: deg and orth as the library normalises them (Chebyshev plans: deg as given, orth 0)."""
	f = dict(op, dtype=dtype, num_cus=num_cus, nprobes=nprobes, plan=plan)
	cheb = plan in (CHEB, CHEB_ACTION)
	f["deg"] = deg if cheb else min(deg, op["n"])
	f["orth"] = 0 if cheb else min(f["deg"] if orth is None else orth, f["deg"])
	return f


def cpu_grid():
	"""Yields (label, switch dict, facts dict) of every case, grouped by switch setting."""
	ops = operators()
	dt = {F64: "f64", F32: "f32"}
	for sw in SWITCHES:
		sl = switch_label(sw)
		for (on, op), dtype in itertools.product(ops.items(), (F64, F32)):
			if not sw:
				for plan, nprobes, cus in itertools.product(KINDS, PROBES, (256, 8)):
					yield f"geometry/{on}/{dt[dtype]}/k{plan}/p{nprobes}/cu{cus}", sw, request(op, dtype, cus, nprobes, 30, 3, plan)
				if on in ("csr5", "ringed_u1_upr2_m1_83", "dense_lda300"):
					for plan, nprobes in itertools.product(KINDS, (8, 64, 257)):
						pairs = [(d, 0) for d in CHEB_DEGS] if plan in (CHEB, CHEB_ACTION) else sorted({(d, d if o is None else min(o, d)) for d in DEGS for o in ORTHS})
						for deg, orth in pairs:
							yield f"depth/{on}/{dt[dtype]}/k{plan}/p{nprobes}/d{deg}/o{orth}", sw, request(op, dtype, 256, nprobes, deg, orth, plan)
			else:
				for plan, nprobes in itertools.product((RING, CHEB), (16, 64, 257)):
					yield f"switch/{sl}/{on}/{dt[dtype]}/k{plan}/p{nprobes}", sw, request(op, dtype, 256, nprobes, 30, 3, plan)


def facts_array(f: dict) -> np.ndarray:
	return np.array([f[k] for k in FACTS], dtype=np.float64)


def shape_call():
	"""facts array -> shape array through slq_debug_plan_shape (under the environment's switches)."""
	L = _capi.lib()
	fn = L.slq_debug_plan_shape
	out = np.empty(NS, dtype=np.float64)
	dp = C.POINTER(C.c_double)

	def call(fa: np.ndarray) -> np.ndarray:
		fa = np.ascontiguousarray(fa, dtype=np.float64)
		rc = fn(fa.ctypes.data_as(dp), NF, out.ctypes.data_as(dp), NS)
		assert rc == _capi.SLQ_OK, L.slq_last_error().decode()
		return out.copy()

	return call


def shape_of_plan(plan) -> tuple:
	"""(facts array, shape array) a live plan was created from (slq_debug_plan_shape_of)."""
	L = _capi.lib()
	fa, sa = np.empty(NF, dtype=np.float64), np.empty(NS, dtype=np.float64)
	dp = C.POINTER(C.c_double)
	rc = L.slq_debug_plan_shape_of(plan._h, fa.ctypes.data_as(dp), NF, sa.ctypes.data_as(dp), NS)
	assert rc == _capi.SLQ_OK, L.slq_last_error().decode()
	return fa, sa


# ---- the live operators and plans of the GPU grid ----------------------------------------------------------------------
def laplacian(m: int, dim: int):
	import scipy.sparse as sp

	T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
	eye = sp.identity(m)
	if dim == 2:
		return (sp.kron(eye, T) + sp.kron(T, eye)).tocsr()
	return (sp.kron(sp.kron(T, eye), eye) + sp.kron(sp.kron(eye, T), eye) + sp.kron(sp.kron(eye, eye), T)).tocsr()


def dense_matrix(n: int) -> np.ndarray:
	rng = np.random.default_rng(7)
	M = rng.standard_normal((n, n))
	return (M + M.T) / np.sqrt(2 * n)


def gram_matrix():
	import scipy.sparse as sp

	return sp.random(350, 200, density=0.02, random_state=np.random.default_rng(11), format="csr")


# label -> (operator, SLQ_TILES or None, dtype, plan kind, nprobes); every plan has 12 steps, Lanczos plans orth 3
GPU_CASES = {
	"lap96_t2_p128": ("lap96", "2", "f64", RING, 128),
	"lap96_t2_p64": ("lap96", "2", "f64", RING, 64),
	"lap96_t2_p32": ("lap96", "2", "f64", RING, 32),
	"lap96_t2_p16": ("lap96", "2", "f64", RING, 16),
	"lap96_t1_p128": ("lap96", "1", "f64", RING, 128),
	"lap96_t0_p128": ("lap96", "0", "f64", RING, 128),
	"lap20c_p128": ("lap20c", None, "f64", RING, 128),
	"dense300_f64_p64": ("dense300", None, "f64", RING, 64),
	"dense300_f64_p16": ("dense300", None, "f64", RING, 16),
	"dense300_f32_p64": ("dense300", None, "f32", RING, 64),
	"gram_p32": ("gram", None, "f64", RING, 32),
	"lap96_t2_recompute": ("lap96", "2", "f64", RECOMPUTE, 128),
	"lap96_t2_cheb": ("lap96", "2", "f64", CHEB, 128),
	"lap96_t2_cheb_action": ("lap96", "2", "f64", CHEB_ACTION, 128),
}
GPU_STEPS, GPU_ORTH = 12, 3


def gpu_matrix(name: str):
	if name == "lap96":
		return laplacian(96, 2)
	if name == "lap20c":
		return laplacian(20, 3)
	if name == "dense300":
		return dense_matrix(300)
	from primate_amd.operators import GramOperator

	return GramOperator(gram_matrix())


def gpu_probes(n: int, nprobes: int) -> np.ndarray:
	rng = np.random.default_rng(1234)
	return np.asfortranarray(np.floor(rng.random((n, nprobes)) * 2) * 2 - 1)


class tiles_env:
	"""SLQ_TILES set to `value` (None: as it is) while an operator and its plans are created."""

	def __init__(self, value):
		self.value = value

	def __enter__(self):
		self.had = os.environ.get("SLQ_TILES")
		if self.value is not None:
			os.environ["SLQ_TILES"] = self.value

	def __exit__(self, *exc):
		if self.value is not None:
			os.environ.pop("SLQ_TILES", None)
			if self.had is not None:
				os.environ["SLQ_TILES"] = self.had


def gpu_plan(op, kind: int, nprobes: int):
	from primate_amd.engine import ChebyshevPlan, LanczosPlan

	if kind in (CHEB, CHEB_ACTION):
		return ChebyshevPlan(op, nprobes, GPU_STEPS, action=kind == CHEB_ACTION)
	return LanczosPlan(op, nprobes, GPU_STEPS, GPU_ORTH, basis="recompute" if kind == RECOMPUTE else None)


DESCRIBE = ("panel_width", "panels", "ring_slots", "sequence", "pipelined", "reordered", "upper_alpha", "far_per_row", "tiles", "omega", "dense_kernel", "dense_ksplit")
_SEQUENCE = {"sweeps": 0, "fused": 1, "fused_stored_u": 2, "fused_gram": 4}


def describe_array(plan) -> np.ndarray:
	"""describe() in the order of DESCRIBE (the sequence by its number)."""
	d = plan.describe()
	return np.array([_SEQUENCE[d[k]] if k == "sequence" else d[k] for k in DESCRIBE], dtype=np.float64)


def action_record(Y: np.ndarray) -> dict:
	"""An n x P action as the golden keeps it (9 MB would not fit a committed file): the sha256 of all its bytes - equality of the
	whole array - and every 256th row as numbers, to show what moved when the digest differs."""
	import hashlib

	Y = np.asfortranarray(Y)
	return {"action_sha256": np.frombuffer(hashlib.sha256(Y.tobytes(order="F")).digest(), dtype=np.uint8), "action_rows": np.ascontiguousarray(Y[::256])}


def gpu_run(plan, kind: int, V: np.ndarray) -> dict:
	"""One 12-step run's results, as arrays: Lanczos plans the tridiagonals and the log quadrature, a Chebyshev plan its moments,
	an action plan the action of sum_k c_k T_k, c from 1 down to 0.1 (bounds [0, 8.1] hold the Laplacian's spectrum), as action_record keeps it."""
	plan.set_probes(V)
	if kind == CHEB_ACTION:
		return action_record(np.asarray(plan.action((0.0, 8.1), np.linspace(1.0, 0.1, GPU_STEPS + 1))))
	if kind == CHEB:
		plan.run((0.0, 8.1))
		return {"moments": np.asarray(plan.moments())}
	plan.run()
	t = plan.tridiag()
	return {"alpha": np.asarray(t[0]), "beta": np.asarray(t[1]), "quad_log": np.asarray(plan.quadrature("log"))}
