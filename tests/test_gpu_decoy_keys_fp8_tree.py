"""Decoy keys (tests/test_gpu_decoy_keys.py) for the FP8-cache and tree-masked builds: an O(1) error for an off-by-one, under random q — the
complement of tests/test_gpu_census_fp8_tree.py.  A NEEDLE k[j*] = 2 q_row sits at an admitted key, so the row's output is the value row of j*
(tests/test_census_fp8_tree_model.py asserts that of the references, within 1e-3); DECOYS 3 q_row, the larger score, sit where the contract
excludes a key.  For a tree row: every draft key base + s whose bit is clear in the row's word, base + sq (a real finite row behind the
draft), the needle's position under another kv head and in another slot; needles at each set draft bit in turn, at base - 1, at keys 0,
31 / 32 and at the last / first key of a piece under forced grids.  For the interval forms: hi, the other kv head, the other slot.

FP8 caches are quantised with amax scales that are no powers of two; the reference is tests/fp8kv_ref.py / tests/fp8kv_tree_ref.py on the
stored bytes, the needle's row the dequantised one.  Forms: FP8 one-token (stream, grid), FP8 multi-token (R = 16, 32, 64), FP8 prefill
(tilings 1, 4), tree over 2-byte and FP8 caches (default plan, forced stream grid).  Expectation: 2e-2 against the needle's row, named first,
then the project's `_check`, both bounds."""
import pytest
import torch

from tests import census_fp8_tree as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = C.xdecoy_cases()
_refs = {}


def _inputs_and_refs(c):
    key = C.xinputs_key(c)
    if key not in _refs:
        _refs.clear()                  # (cases that share inputs are neighbours in the table)
        q, kc, vc, scales, plants = C.xdecoy_inputs(c)
        _refs[key] = (q, kc, vc, scales, plants, C.xdecoy_reference(c, q, kc, vc, scales, "f64"), C.xdecoy_reference(c, q, kc, vc, scales, "f32"))
    return _refs[key]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_decoy_keys_fp8_tree(case):
    q, kc, vc, scales, plants, ref64, ref32 = _inputs_and_refs(case)
    raw = (lambda t: t.view(torch.uint8)) if case["fp8"] else (lambda t: t)
    # (the rows an appending call fills hold 0.5 / -0.25 before it: as bytes 0x30 / 0xB4, finite either way)
    fill = (0x30, 0xB4) if case["fp8"] else (0.5, -0.25)
    out, _, d = C.launch_ext(case, q, raw(kc).to(DEV), raw(vc).to(DEV), DEV, *fill, scales=scales)
    what = "%s %s" % (case["name"], d)
    o = out.double().cpu()
    for b, t, h, slot, hk, j in plants:          # named first: the row that took a decoy says which one
        row = vc[slot, j, hk].double() * (scales[1][hk].double() if scales is not None else 1.0)
        dev = float((o[b, t, h] - row).abs().max())
        word = " (mask word 0x%08x, base %d)" % (case["masks"][b][t], case["lens"][b] - case["sq"]) if case["form"] == "tree" else ""
        assert dev < 2e-2, "%s: entry %d token %d head %d%s does not return the value row of its needle (key %d, kv head %d, slot %d): off by %.3g" % (
            what, b, t, h, word, j, hk, slot, dev)
    C.check(out, ref64, ref32, C.DT[case["dt"]], what)
