"""Decoy keys: an O(1) error for an off-by-one, under random q (the complement of tests/test_gpu_census.py).  Background k = 0.1 randn, v = randn;
for chosen (entry, token, head) rows a NEEDLE k[j*] = 2 q_row at an admitted position — its probability is above 1 - 1e-4, the row's output is
v[j*] (tests/test_census_model.py asserts that of the oracle, within 1e-3) — and DECOYS with the larger score, 3 q_row, at the positions the
contract excludes: hi (a real, finite row: the next draft token's appended row, or the next cache row), lo - 1, the same position under
another kv head, the same position in another slot.  A kernel that admits one of them answers with the wrong value row: an error of order 1.

Needles: hi - 1 for every token of a multi-token call, lo, key 0, 31 / 32, 63 / 64, and 95 / 96, 159 / 160 — the last / first key of a piece
under host items of three tiles and forced grids.  Forms: one-token decode (stream, uniform split, host items), multi-token (R = 16, 32, 64),
prefill tilings 1, 4 and 7; windowed and not.  Expectation: the fp64 oracle through the project's `_check`, both bounds."""
import pytest
import torch

from tests import census as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = C.decoy_cases()
_refs = {}


def _inputs_and_refs(c):
    key = C.inputs_key(c)
    if key not in _refs:
        _refs.clear()                  # (cases that share inputs are neighbours in the table)
        q, kc, vc, plants = C.decoy_inputs(c)
        _refs[key] = (q, kc, vc, plants, C.reference(c, q, kc, vc, "f64"), C.reference(c, q, kc, vc, "f32"))
    return _refs[key]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_decoy_keys(case):
    q, kc, vc, plants, ref64, ref32 = _inputs_and_refs(case)
    out, _, d = C.launch(case, q, kc, vc, DEV)
    what = "%s %s" % (case["name"], d)
    o = out.double().cpu()
    for b, t, h, slot, hk, j in plants:          # named first: the row that took a decoy says which one
        dev = float((o[b, t, h] - vc[slot, j, hk].double()).abs().max())
        assert dev < 2e-2, "%s: entry %d token %d head %d does not return the value row of its needle (key %d, kv head %d, slot %d): off by %.3g" % (what, b, t, h, j, hk, slot, dev)
    C.check(out, ref64, ref32, C.DT[case["dt"]], what)
