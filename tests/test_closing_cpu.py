"""Which plans leave the closing tail of a run to its first request, decided without a device: `slq_debug_lazy_tail`
(csrc/slq_sequence.hpp: has_lazy_tail) over the fact grid tests/test_sequence_cpu.py walks.

The rule: a plan has a lazy tail exactly where the update pass of step deg - 1 carries the no-store bit (xt_update & 16 in
step_shape's answer) AND the plan is a plain quadrature plan (basis mode 0: a recompute plan's runs stay whole) AND
the plan was not created under SLQ_LAST_STORE=2 (`lazy_close` = 0 below), which keeps the pass in the run, AND nothing rewrites
the operator's values under a live plan (`values_fixed` = 0: the affine operator A + t B - a deferred pass would read the
values of another t). step_shape's own answers are not touched by any of this (test_sequence_cpu.py holds them)."""

import ctypes as C
import itertools
import re
from pathlib import Path

import pytest

import test_sequence_cpu as ts
from primate_amd import _capi

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lazy_of():
	L = _capi.lib()
	fa, out, sh = (C.c_int * ts.NF)(), C.c_int(), (C.c_int * (ts.NS + 1))()

	def call(facts, lazy_close, values_fixed=1):
		fa[:] = facts
		assert L.slq_debug_lazy_tail(fa, ts.NF, lazy_close, values_fixed, C.byref(out)) == _capi.SLQ_OK
		assert L.slq_debug_step_shape(fa, ts.NF, ts.DEG - 1, 0, sh, ts.NS + 1) == _capi.SLQ_OK
		return out.value, dict(zip(ts.SHAPE, sh[:]))

	return call


def walk(lazy_of, names, values, **fixed):
	n = n_lazy = 0
	for combo in itertools.product(*values):
		f = ts.facts_of(**fixed, **dict(zip(names, combo)))
		fl = [f[k] for k in ts.FACTS]
		for lazy_close, values_fixed in ((0, 1), (1, 1), (1, 0), (0, 0)):
			got, s = lazy_of(fl, lazy_close, values_fixed)
			nostore = bool(s["xt_update"] & 16)
			assert got == int(bool(lazy_close) and bool(values_fixed) and nostore and f["basis"] == 0), (f, lazy_close, values_fixed, s)
			if got:  # what the launch code relies on: a closing step that can be cut in front of its update pass
				assert s["seq"] in (ts.GRAM_RING, ts.GRAM_CSR, ts.MERGED, ts.SEPARATE) and f["nstale"] == 0 and f["last_store"] == 0
			n += 1
			n_lazy += got
	return n, n_lazy


def test_structure_product(lazy_of):
	names = ("csr", "far_le4", "tiles", "ringR", "upper", "orth", "nstale", "fused", "merged", "mgs", "gram", "ring_gen")
	values = ((0, 1), (0, 1), (0, 1, 2), (0, 1, 2), (0, 1), ts.ORTHS, (0, 2), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1))
	n, n_lazy = walk(lazy_of, names, values)
	assert n == 4 * 2 * 2 * 3 * 3 * 2 * 6 * 2 * 3 * 2 * 2 * 2 * 2 and 0 < n_lazy < n // 4


def test_gates_product(lazy_of):
	names = ("basis", "stored_u", "nt", "gram_csr", "ring_deep", "last_store", "tiles", "ringR", "far_le4", "orth")
	values = ((0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1, 2), (0, 1), ts.ORTHS)
	n, n_lazy = walk(lazy_of, names, values)
	assert n == 4 * 96 * 9 * 2 * 6 and 0 < n_lazy < n // 4


def test_the_plans_named_in_the_design(lazy_of):
	ring = dict(tiles=2, ringR=1)

	def lazy(lazy_close=1, values_fixed=1, **kw):
		f = ts.facts_of(**kw)
		return lazy_of([f[k] for k in ts.FACTS], lazy_close, values_fixed)[0]

	assert lazy(**ring) == 1 and lazy(0, **ring) == 0  # the flagship's plan: ring-fed Gram, orth 3
	assert lazy(orth=0, **ring) == 1 and lazy(orth=8, **ring) == 1 and lazy(tiles=2, ringR=2) == 1
	assert lazy() == 1 and lazy(orth=0) == 1 and lazy(gram=0) == 1  # the generic passes: Gram, separate, merged
	assert lazy(basis=1, **ring) == 0 and lazy(basis=2, **ring) == 0 and lazy(last_store=1, **ring) == 0
	assert lazy(orth=9, **ring) == 0 and lazy(orth=ts.DEG, **ring) == 0  # more than 8 ring columns at the closing step: sweeps
	assert lazy(nstale=2, **ring) == 0 and lazy(fused=0, **ring) == 0 and lazy(csr=0) == 0
	assert lazy(far_le4=0) == 0  # the stored-u sequence has no such bit
	## an affine operator is a CSR without the upper copy: merged / separate on the generic passes, the bit set - and still whole
	assert lazy(upper=0) == 1 and lazy(upper=0, orth=0) == 1 and lazy(values_fixed=0, upper=0) == 0 and lazy(values_fixed=0, upper=0, orth=0) == 0
	assert lazy(tiles=1, ringR=1) == 0 and lazy(ring_gen=0, **ring) == 0  # barrier tiles, k_csr_ring_pass


def test_wrong_length_is_refused():
	fa, out = (C.c_int * ts.NF)(), C.c_int()
	assert _capi.lib().slq_debug_lazy_tail(fa, ts.NF - 1, 1, 1, C.byref(out)) == _capi.SLQ_EINVAL


def test_switch_and_entries_are_declared():
	table = (ROOT / "primate_amd" / "csrc" / "slq_switches.hpp").read_text()
	m = re.search(r'PLAN\(last_store, "SLQ_LAST_STORE", (-?\d+), "([^"]*)"', table)
	assert m and int(m.group(1)) == 0 and "first asked for" in m.group(2) and "2 stores nothing, launched with the run" in m.group(2)
	design = (ROOT / "DESIGN.md").read_text()
	row = [l for l in design[design.index("### 5.4") :].splitlines() if l.startswith("| `SLQ_LAST_STORE` | 0 |")]
	assert len(row) == 1 and "closing tail" in row[0] and "2:" in row[0]
	hdr = (ROOT / "include" / "slq.h").read_text()
	for sym in ("slq_plan_closing_state", "slq_debug_lazy_tail"):
		assert sym in _capi.EXPORTED_SYMBOLS and re.search(rf"\bint {sym}\(", hdr), sym
	from primate_amd import engine

	assert callable(engine.LanczosPlan.closing)
