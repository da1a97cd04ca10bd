"""What a Lanczos step launches, decided without a device: `slq_debug_step_shape` (csrc/slq_sequence.hpp: step_shape) enumerated
over the facts of a plan and its operator, and the conditions the launch code states checked on every answer.

Every fact combination of a product is an input; none is skipped. The full product of all facts has 2.8e7 cases - too many
for one ctypes call each - so it is covered in two products that share every assertion:
 * `test_structure_product`: operator kind, far_per_row side, tiles, ringR, upper triangle, orth, nstale, fused, merged, mgs,
   gram, ring_gen and j in full; fixed at their defaults there: basis mode 0, stored_u 1, nt 1, gram_csr 1, ring_deep 1,
   last_store 0 (the facts that only gate one sequence or one bit each);
 * `test_gates_product`: those six in full, over tiles, ringR, far_per_row side, orth and j in full, on a symmetric CSR operator
   with the remaining switches at their defaults.
The stand-alone scripts/sequence_enum.cpp runs the one full product with the same assertions (host compiler, sanitizers).
The facts that select no sequence (upper-triangle stream and its padding, dense kernel class, pipelined loop, cross, ring_alpha,
ring_rev, omega_on) are set as a plan would derive them; `test_bits_follow_their_switches` turns each of them."""

import ctypes as C
import itertools

import pytest

from primate_amd import _capi

DEG = 20
KMAX, RINGMAX = 8, 3
ORTHS = (0, 1, 3, 8, 9, 20)
STEPS = (0, 1, 2, 8, 9, DEG - 2, DEG - 1)
GRAM_RING, GRAM_CSR, MERGED, SEPARATE, STORED_U, SW_CGS, SW_MGS, SW_PLAIN = range(8)
SWEEPS = (SW_CGS, SW_MGS, SW_PLAIN)
DESCRIBE = {GRAM_RING: 4, GRAM_CSR: 4, MERGED: 1, SEPARATE: 1, STORED_U: 2, SW_CGS: 0, SW_MGS: 0, SW_PLAIN: 0}
NF, NS = 27, 18
# order of the facts (seq::facts_from_array) and of the answer (seq::shape_to_array)
FACTS = ("csr", "far_le4", "tiles", "upper", "ringR", "rs_desc_u", "rs_u_padded", "deg", "orth", "nstale", "basis", "dense_class", "pipelined",
         "omega_on", "fused", "merged", "mgs", "stored_u", "nt", "cross", "gram", "gram_csr", "ring_gen", "ring_deep", "last_store", "ring_alpha",
         "ring_rev")  # fmt: skip
SHAPE = ("seq", "r", "tiled", "gen", "alpha_tiled", "alpha_upper", "half", "pipe_on", "xt_alpha", "xt_dots", "xt_update", "omega", "est_prev", "product",
         "blk_alpha", "blk_dots", "blk_beta", "prev_xt")  # fmt: skip
assert len(FACTS) == NF and len(SHAPE) == NS


@pytest.fixture(scope="module")
def shape_of():
	L = _capi.lib()
	fa, out = (C.c_int * NF)(), (C.c_int * (NS + 1))()
	fn = L.slq_debug_step_shape

	def call(facts, j, prev_xt):
		fa[:] = facts
		assert fn(fa, NF, j, prev_xt, out, NS + 1) == _capi.SLQ_OK
		return out[:]

	return call


def facts_of(**kw):
	f = dict(csr=1, far_le4=1, tiles=0, upper=1, ringR=0, deg=DEG, orth=3, nstale=0, basis=0, dense_class=0, pipelined=0, omega_on=1, fused=1,
	         merged=1, mgs=0, stored_u=1, nt=1, cross=1, gram=1, gram_csr=1, ring_gen=1, ring_deep=1, last_store=0, ring_alpha=2, ring_rev=1)  # fmt: skip
	f.update(kw)
	f.setdefault("rs_desc_u", int(f["upper"] and f["tiles"] == 2 and f["ringR"] > 0))
	f.setdefault("rs_u_padded", f["rs_desc_u"])
	if not f["csr"] and "dense_class" not in kw:
		f["dense_class"] = 4
	return f


def describe_today(f):
	"""slq_plan_describe().sequence as the parent commit computes it: plan_create's derived flags, then plan_sequence()."""
	ringed = f["tiles"] == 2 and f["ringR"] > 0  # (a plan only has ringR > 1 on ring-fed tiles)
	ring_gen = ringed and (f["ringR"] > 1 or (f["nt"] and f["ring_gen"]))
	ring_deep = ringed and (f["ringR"] > 1 or f["nt"]) and f["ring_deep"]
	gram = ring_gen and ring_deep and f["merged"] and not f["mgs"] and f["upper"] and f["gram"]
	gram_csr = f["csr"] and f["ringR"] == 0 and f["upper"] and f["merged"] and not f["mgs"] and f["nt"] and f["gram"] and f["gram_csr"]
	if not f["csr"] or f["fused"] == 0 or f["mgs"] or f["nstale"] > 0:
		return 0
	if f["fused"] == 2 or f["far_le4"]:
		return 4 if ((gram and f["ringR"] > 0) or gram_csr) and f["orth"] >= 1 else 1
	return 2 if f["orth"] >= 1 and f["stored_u"] and f["merged"] and f["ringR"] == 0 else 0


def check(f, j, prev_xt, out):
	s = dict(zip(SHAPE, out))
	seq, r = s["seq"], s["r"]
	mgs = f["mgs"] or f["nstale"] > 0
	assert 0 <= seq <= 7  # exactly one sequence
	assert r == (min(j + 1 + f["nstale"], f["orth"]) if f["orth"] > 0 else 0)
	if seq in (GRAM_RING, GRAM_CSR):
		assert r >= 1 and f["nstale"] == 0 and not mgs and f["upper"] and f["gram"]
	if seq == GRAM_RING:
		assert s["gen"] and s["tiled"]
	if seq == GRAM_CSR:
		assert not s["tiled"]
	if seq == STORED_U:
		assert f["csr"] and not s["tiled"] and 1 <= r <= KMAX and f["merged"] and f["stored_u"]
		assert s["xt_dots"] & 2 and s["xt_update"] & 2
	else:
		assert not (s["xt_dots"] & 2) and not (s["xt_update"] & 2)
	if r > KMAX or mgs or not f["csr"] or f["fused"] == 0:
		assert seq in SWEEPS
	if seq in SWEEPS:
		assert seq == (SW_PLAIN if r == 0 else SW_MGS if mgs else SW_CGS)
		assert s["xt_update"] == 0 and s["xt_alpha"] == 0
	if s["gen"] or s["alpha_upper"]:
		assert f["tiles"] == 2 and f["ringR"] > 0
	if s["alpha_tiled"]:
		assert s["tiled"]
	# bit 16: the run's last step stores nothing
	nostore = bool(s["xt_update"] & 16)
	if nostore:
		assert j == DEG - 1 and f["basis"] != 1 and f["last_store"] == 0 and seq not in (STORED_U,) + SWEEPS
		assert not (s["tiled"] and not s["gen"])  # never the barrier-tile kernels (nor k_csr_ring_pass)
		assert not (s["tiled"] and f["tiles"] != 2)
	elif seq in (GRAM_RING, GRAM_CSR, MERGED, SEPARATE) and j == DEG - 1 and f["basis"] != 1 and f["last_store"] == 0:
		assert s["tiled"] and not s["gen"]
	if s["xt_update"] & 4:
		assert s["tiled"] and f["tiles"] == 2 and f["ring_rev"]
	if s["xt_alpha"] & 8:
		assert s["gen"] and s["alpha_upper"] and f["rs_u_padded"]
	if s["omega"]:
		assert r == 3 == f["orth"] and seq == GRAM_RING and f["omega_on"]
		assert s["est_prev"] == int(j >= 3)
	else:
		assert not s["est_prev"]
	if s["prev_xt"]:
		assert seq == SEPARATE and f["cross"] and s["xt_update"] & 1
	else:
		assert not (s["xt_update"] & 1)
	if seq == SEPARATE:
		assert (s["xt_alpha"] & 1) == int(bool(prev_xt) and j > 0)
	assert out[NS] == describe_today(f)
	if r <= KMAX:
		assert DESCRIBE[seq] == out[NS]


def run_product(shape_of, names, values, **fixed):
	n = 0
	for combo in itertools.product(*values):
		f = facts_of(**fixed, **dict(zip(names, combo)))
		fl = [f[k] for k in FACTS]
		for j in STEPS:
			for prev_xt in ((0, 1) if j in (1, DEG - 1) and not f["merged"] else (0,)):
				check(f, j, prev_xt, shape_of(fl, j, prev_xt))
				n += 1
	return n


def test_structure_product(shape_of):
	names = ("csr", "far_le4", "tiles", "ringR", "upper", "orth", "nstale", "fused", "merged", "mgs", "gram", "ring_gen")
	values = ((0, 1), (0, 1), (0, 1, 2), (0, 1, 2), (0, 1), ORTHS, (0, 2), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1))
	n = run_product(shape_of, names, values)
	assert n >= 2 * 2 * 3 * 3 * 2 * 6 * 2 * 3 * 2 * 2 * 2 * 2 * len(STEPS)


def test_gates_product(shape_of):
	names = ("basis", "stored_u", "nt", "gram_csr", "ring_deep", "last_store", "tiles", "ringR", "far_le4", "orth")
	values = ((0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1, 2), (0, 1), ORTHS)
	n = run_product(shape_of, names, values)
	assert n >= 96 * 9 * 2 * 6 * len(STEPS)


def test_bits_follow_their_switches(shape_of):
	"""The facts that select no sequence, each turned on the plan it matters to (ring-fed wide panels, orth 3; a dense operator)."""
	ring = dict(tiles=2, ringR=1)

	def at(j, prev_xt=0, **kw):
		f = facts_of(**kw)
		out = shape_of([f[k] for k in FACTS], j, prev_xt)
		check(f, j, prev_xt, out)
		return dict(zip(SHAPE, out))

	s = at(5, **ring)
	assert s["seq"] == GRAM_RING and s["omega"] and s["est_prev"] and s["alpha_upper"] and s["xt_alpha"] == 1 | 8 and s["xt_update"] == 4
	assert at(DEG - 1, **ring)["xt_update"] == 4 | 16
	assert at(5, ring_rev=0, **ring)["xt_update"] == 0
	assert at(5, rs_u_padded=0, **ring)["xt_alpha"] == 1
	assert not at(5, omega_on=0, **ring)["omega"]
	s = at(5, rs_desc_u=0, rs_u_padded=0, **ring)  # no upper-triangle stream: the generic upper-triangle alpha pass
	assert not s["alpha_tiled"] and s["half"] and s["xt_alpha"] == 1
	s = at(5, ring_alpha=1, **ring)
	assert s["alpha_tiled"] and not s["alpha_upper"] and not s["half"] and s["xt_alpha"] == 1
	assert not at(5, ring_alpha=0, **ring)["alpha_tiled"]
	s = at(5, ring_gen=0, **ring)  # k_csr_ring_pass: merged sequence, no Gram, never bit 16
	assert s["seq"] == MERGED and s["tiled"] and not s["gen"]
	assert at(DEG - 1, ring_gen=0, **ring)["xt_update"] == 4
	assert at(DEG - 1, tiles=1, ringR=1)["xt_update"] == 0  # barrier tiles
	assert at(5, pipelined=1)["pipe_on"] == 1 and at(5, pipelined=1, **ring)["pipe_on"] == 0
	s = at(5, orth=0, prev_xt=1)
	assert s["seq"] == SEPARATE and s["xt_alpha"] == 1 and s["xt_update"] == 1 and s["prev_xt"] == 1
	s = at(5, orth=0, cross=0, prev_xt=0)
	assert s["xt_update"] == 0 and s["prev_xt"] == 0
	# the sweeps' product by operator kind
	assert at(5, csr=0, dense_class=4)["product"] == 2 and at(5, csr=0, dense_class=1)["product"] == 3 and at(5, csr=0, dense_class=0)["product"] == 3
	assert at(5, fused=0)["product"] == 1 and at(5, fused=0, **ring)["product"] == 0


def test_wrong_lengths_are_refused(shape_of):
	L = _capi.lib()
	fa, out = (C.c_int * NF)(), (C.c_int * (NS + 1))()
	assert L.slq_debug_step_shape(fa, NF - 1, 0, 0, out, NS + 1) == _capi.SLQ_EINVAL
	assert L.slq_debug_step_shape(fa, NF, 0, 0, out, NS) == _capi.SLQ_EINVAL
